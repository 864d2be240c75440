"""Cases and the launch helper of the skinny fp8-weight GEMM (``ops.linear_skinny_w8``,
csrc/kernels/gemm_skinny_w8.hip) for test_skinny_w8_cpu.py and test_skinny_w8_gpu.py. Inputs, float64
references and checks are those of gemm_cases.py / gemm_checks.py with ``C_BOUND`` unchanged: the
reference is taken on ``q.double() * scale``, the fp8 -> bf16 conversion is exact and the scale is one
fp32 multiply in the epilogue, inside the K * 2^-24 term. Shapes (N, K): (16, 32) a quarter slice;
(48, 160) a slice and a quarter, empty waves; (50, 128) ragged strip, odd ldc; (272, 2112) 16.5
slices, uneven runs at every W; (1041, 512); (64, 8320)."""
import functools

import torch

import gemm_cases as gc
import gemm_checks as gk
from distributed_llm_scheduler_amd import ops

BF = torch.bfloat16
MS = (1, 2, 5, 16)
WAVES = (4, 8, 16)
PLAIN = ((16, 32), (48, 160), (50, 128), (272, 2112), (1041, 512), (64, 8320))
SWIGLU = ((64, 160), (96, 2112), (256, 512))
# (name, family of gemm_checks.C_BOUND, bias, act, residual, alpha)
EPIS = (("none", "linear", False, None, False, 1.0), ("bias", "linear", True, None, False, 1.0),
        ("bias_gelu_res", "gelu", True, "gelu", True, 1.0), ("half_silu", "silu", False, "silu", False, 0.5))
EXACT_SHAPES = ((16, 16, 32), (5, 50, 128), (16, 272, 2112))


def launch(fn, dev, x, q, s, bias=None, act=None, res=None, alpha=1.0, waves=None, what=""):
    """fn on NaN-padded strided operands (q: ldw = K + 16 bytes of the e4m3 NaN code, three extra
    rows) into a NaN-filled output inside canary rows and columns."""
    (M, K), N = x.shape, q.shape[0]
    n_out = N // 2 if act == "swiglu" else N
    pd = gc.padded(x, torch.zeros(1, K, dtype=BF), None, dev)
    qbuf = torch.full((N + gc.PAD_ROWS, K + 16), 0x7f, dtype=torch.uint8)
    qbuf[:N, :K] = q.view(torch.uint8)
    rbuf = None
    if res is not None:
        rbuf = torch.full((M + gc.PAD_ROWS, gc.out_ld(n_out)), float("nan"), dtype=BF)
        rbuf[:M, :n_out] = res
        rbuf = rbuf.to(dev)
    obuf = torch.full((M + gc.PAD_ROWS, gc.out_ld(n_out)), gc.CANARY, dtype=BF, device=dev)
    out = obuf[:M, :n_out]
    out.fill_(float("nan"))
    pd = pd._replace(res=None if rbuf is None else rbuf[:M, :n_out], rbuf=rbuf, out=out, obuf=obuf)
    y = fn(pd.a, qbuf.to(dev)[:N, :K].view(torch.float8_e4m3fn), s.to(dev), bias=None if bias is None else bias.to(dev),
           act=act, residual=pd.res, alpha=alpha, out=out, waves=waves)
    assert y is out
    gk.check_canary(pd, M, n_out, res, what)
    return out.cpu()


@functools.lru_cache(maxsize=None)
def operands(M, N, K, arbitrary=False):
    """random_operands with the weight quantised: (c, q, scale, the reference's float64 weight).
    ``arbitrary``: the scales replaced by positive fp32 values in [2^-12, 2^-2], no powers of two."""
    c = gc.random_operands(M, N, K)
    q, s = ops.quantize_fp8(c["w"])
    if arbitrary:
        s = (2.0 ** -12 * 1024.0 ** torch.rand(N, generator=torch.Generator().manual_seed(N + K))).float()
    return c, q, s, q.float().double() * s.double()[:, None]


def run_plain(fn, dev, M, N, K, waves=WAVES, arbitrary=False):
    c, q, s, w64 = operands(M, N, K, arbitrary)
    ap = gk.absprod64(c["x"], w64)
    for name, fam, has_bias, act, has_res, alpha in EPIS:
        bias, res = (c["bias"] if has_bias else None), (c["res"] if has_res else None)
        pre, ref = gk.ref64(c["x"], w64, bias, act, res, alpha)
        for W in waves:
            what = f"w8 {name} {(M, N, K)} W {W}" + (" arbitrary scales" if arbitrary else "")
            gk.check_bound(launch(fn, dev, c["x"], q, s, bias, act, res, alpha, W, what), pre, ref, ap, K, fam, what)


def run_swiglu(fn, dev, M, N, K, waves=WAVES):
    c, q, s, w64 = operands(M, N, K)
    for bias in (None, c["bias"]):
        pre, ap = gk.ref64_swiglu(c["x"], w64, bias)
        for W in waves:
            what = f"w8 swiglu bias {bias is not None} {(M, N, K)} W {W}"
            gk.check_bound(launch(fn, dev, c["x"], q, s, bias, "swiglu", waves=W, what=what), pre, pre, ap, K, "swiglu", what)


def run_exact(fn, dev, kind, M, N, K, waves=WAVES):
    """The integer / scaled probes survive quantize_fp8 bit for bit (asserted): torch.equal."""
    p = gc.probe(kind, M, N, K)
    q, s = ops.quantize_fp8(p.w)
    assert torch.equal(ops.dequantize_fp8(q, s), p.w), "the probe's weight does not survive quantize_fp8"
    for epi in (gc.EPI_NONE, gc.EPI_FULL):
        want = gk.expected_exact(p, epi)
        bias, res, act, alpha = gc.operands(p, epi)
        for W in waves:
            what = f"w8 {kind} {epi.name} {(M, N, K)} W {W}"
            gk.check_exact(launch(fn, dev, p.x, q, s, bias, act, res, alpha, W, what), want, what)


def run_codes(fn, dev, K, ks, W, N=50):
    """One-hot code probe: q[n][k] = byte (n K + k) mod 256 (NaN codes -> 0), power-of-two scales,
    x row m one-hot at ks[m]: out[m][n] == float(q[n][ks[m]]) * scale[n] exactly. Pins the byte
    order of the conversion and the k-permutation between the weight bytes and the x fragment."""
    b = ((torch.arange(N)[:, None] * K + torch.arange(K)[None, :]) % 256).to(torch.uint8)
    b[(b == 0x7f) | (b == 0xff)] = 0
    q = b.view(torch.float8_e4m3fn)
    s = torch.pow(2.0, (torch.arange(N) % 5 - 3).float())
    for i in range(0, len(ks), 16):
        sel = torch.tensor(ks[i:i + 16])
        x = torch.zeros(len(sel), K, dtype=BF)
        x[torch.arange(len(sel)), sel] = 1.0
        want = (q.float()[:, sel] * s[:, None]).T.contiguous()
        assert torch.equal(want.to(BF).float(), want)
        what = f"w8 codes K {K} k {ks[i]}.. W {W}"
        gk.check_exact(launch(fn, dev, x, q, s, waves=W, what=what), want.to(BF), what)


def run_start_k(W, K=2112):
    """The first k of every wave's run of 128-wide slices and the last 16 k."""
    nk = -(-K // 128)
    return [k for k in range(0, nk * 128, -(-nk // W) * 128)] + list(range(K - 16, K))
