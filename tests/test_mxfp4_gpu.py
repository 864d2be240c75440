"""MXFP4 weights on the GPU: the W4A8 GEMM (csrc/kernels/gemm_w4a8.hip: fp4 x fp8 on the
block-scaled MFMA with the stored e8m0 block scales), the device run of the quantiser, and the
executor with ``weight_dtype="mxfp4", act_dtype="fp8"``. The kernel's lane maps (nibble order,
the e4m3 operand's k order, which scale byte a lane group uses) are proved by the exact tests:
one-hot activations pick single weights, so a wrong pairing gives a wrong value, not a small
error."""
import pytest
import torch

from distributed_llm_scheduler_amd import ops
from distributed_llm_scheduler_amd.models import reference
from distributed_llm_scheduler_amd.parallel import runtime
from distributed_llm_scheduler_amd.parallel.executor import synthetic_tokens

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-2  # the tolerance of tests/test_w8_gpu.py
F8 = torch.float8_e4m3fn
E2M1 = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float32)


def _configs():
    return [(c, s) for c in range(ops.w4a8_configs()) for s in ops.W4A8_SPLITS]


def _close(a, b, tol=TOL):
    err = (a.float() - b.float()).abs().max().item()
    ref = b.float().abs().max().item() + 1e-6
    assert err <= tol * ref, f"max abs err {err:.4g} vs ref max {ref:.4g} (rel tol {tol})"


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(torch.bfloat16).to(DEV)


def _pack(codes):
    """e2m1 codes [N, K] -> bytes [N, K/2]: even k in the low nibble."""
    codes = codes.to(torch.uint8)
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def _one_hot(K):
    """K activation rows, row m is e4m3 1.0 at k = m and zero elsewhere; row scales 1."""
    return torch.eye(K).to(F8).to(DEV), torch.ones(K, device=DEV)


def _same(y, want, what):
    """Exact equality of every value (a zero of either sign equals a zero)."""
    assert y.shape == want.shape, what
    assert torch.equal(y.float().cpu(), want.float().cpu()), what


# -------------------------------------------------------------------------- exact lane maps
def test_all_codes_identity():
    """Row n of W holds code (n + k) % 16 at k: all 16 codes at each of the 32 nibble positions
    of a lane's 16 bytes (and at every k of the slice). With one-hot activations the output
    [k][n] is the decoded code, bit for bit: the nibble order and the k pairing for k = 0..127."""
    N, K = 32, 128
    codes = (torch.arange(N)[:, None] + torch.arange(K)[None, :]) % 16
    q = _pack(codes).to(DEV)
    s = torch.full((N, K // 32), 127, dtype=torch.uint8, device=DEV)
    xq, xs = _one_hot(K)
    want = E2M1[codes].t().to(torch.bfloat16)  # [k][n]
    for cfg in [None] + _configs():
        _same(ops.linear_w4a8(xq, xs, q, s, config=cfg), want, f"config {cfg}")


def test_scale_placement():
    """Weights 1.0 everywhere, scale code 120 + (3n + b) % 15 at (row n, block b): distinct over a
    row's eight blocks and over neighbouring rows, so a wrong scale byte, lane group, slice or
    row gives another power of two. K = 256 is two slices, N = 48 is not a whole tile."""
    N, K = 48, 256
    q = torch.full((N, K // 2), 0x22, dtype=torch.uint8, device=DEV)
    sc = 120 + (3 * torch.arange(N)[:, None] + torch.arange(K // 32)[None, :]) % 15
    s = sc.to(torch.uint8).to(DEV)
    xq, xs = _one_hot(K)
    want = torch.ldexp(torch.ones(K, N), (sc.t().repeat_interleave(32, 0) - 127).int()).to(torch.bfloat16)
    for cfg in [None] + _configs():
        _same(ops.linear_w4a8(xq, xs, q, s, config=cfg), want, f"config {cfg}")


def test_extreme_scale_codes():
    """Any scale code 0..254 (checkpoints quantised elsewhere): weights 1.0, one block per code,
    one-hot activations with row scales that bring 2^(code - 127) into the normal bf16 range."""
    sc = torch.tensor([0, 1, 2, 64, 126, 127, 128, 190, 253, 254])
    N, K = 16, 32 * len(sc)
    q = torch.full((N, K // 2), 0x22, dtype=torch.uint8, device=DEV)
    s = sc.to(torch.uint8)[None, :].repeat(N, 1).to(DEV)
    e = (sc - 127).repeat_interleave(32)  # per k
    xe = torch.where(e < -100, 40, torch.where(e > 100, -40, 0))
    xq = torch.eye(K).to(F8).to(DEV)
    xs = torch.ldexp(torch.ones(K), xe.int()).to(DEV)
    want = torch.ldexp(torch.ones(K, N), (e + xe).int()[:, None].expand(K, N)).to(torch.bfloat16)
    for cfg in [None] + _configs():
        _same(ops.linear_w4a8(xq, xs, q, s, config=cfg), want, f"config {cfg}")


def test_exact_integers_asymmetric():
    """W in {+-0.5 .. +-6} with block scales 2^{0,1,2}, integer activations in [-8, 8],
    power-of-two row scales: every partial sum is a multiple of 0.5 below 2^20, so fp32
    accumulation in any order (split-K included) is exact and the output is bit-equal to the
    fp32 product rounded to bf16. K = 416 ends in a slice of one block; M and N are no tile
    multiples."""
    M, N, K = 77, 130, 416
    g = torch.Generator().manual_seed(5)
    mag = torch.randint(1, 8, (N, K), generator=g)
    codes = mag + 8 * torch.randint(0, 2, (N, K), generator=g)
    sc = 127 + torch.randint(0, 3, (N, K // 32), generator=g)
    xi = torch.randint(-8, 9, (M, K), generator=g).float()
    q, s = _pack(codes).to(DEV), sc.to(torch.uint8).to(DEV)
    wd = E2M1[codes] * torch.ldexp(torch.ones(N, K // 32), (sc - 127).int()).repeat_interleave(32, 1)
    assert torch.equal(ops.dequantize_mxfp4(q.cpu(), s.cpu(), torch.float32), wd)
    xq = xi.to(F8).to(DEV)
    assert torch.equal(xq.float().cpu(), xi)
    xs = 2.0 ** ((torch.arange(M) % 7) - 3).float()
    want = ((xi @ wd.t()) * xs[:, None]).to(torch.bfloat16)
    for cfg in [None] + _configs():
        _same(ops.linear_w4a8(xq, xs.to(DEV), q, s, config=cfg), want, f"config {cfg}")


# ----------------------------------------------------------------------------------- random
def _problem(M, N, K, seed=0):
    """xq e4m3 [M, K] (quantised N(0, 1) rows) with arbitrary fp32 row scales in [1e-3, 10], an
    MXFP4 weight (quantised N(0, 0.02)), and the fp32 product of the same dequantised values."""
    g = torch.Generator(device="cpu").manual_seed(400 + seed)
    xq, _ = ops.quantize_fp8(torch.randn(M, K, generator=g).to(torch.bfloat16))
    q, s = ops.quantize_mxfp4((0.02 * torch.randn(N, K, generator=g)).to(torch.bfloat16))
    xs = torch.exp(torch.empty(M).uniform_(-6.9077, 2.3026, generator=g)).clamp_(1e-3, 10.0)
    ref = (xq.float() @ ops.dequantize_mxfp4(q, s, torch.float32).t()) * xs[:, None]
    return xq.to(DEV), xs.to(DEV), q.to(DEV), s.to(DEV), ref.to(DEV)


@pytest.mark.parametrize("N", [48, 208])
@pytest.mark.parametrize("M", [1, 77, 200])
def test_shapes_every_config(M, N):
    """K = 32 and 160 end in a partial slice, 416 in a slice of one block (scale rows of 1, 5 and
    13 bytes: the byte-wise scale loads), 1024 is whole slices (scale rows of 32 bytes: the
    dword loads); N = 48 and 208 are no tile multiples."""
    for K in (32, 160, 416, 1024):
        xq, xs, q, s, ref = _problem(M, N, K, seed=K)
        for cfg in [None] + _configs():
            y = ops.linear_w4a8(xq, xs, q, s, config=cfg)
            assert y.shape == (M, N)
            _close(y, ref)


def test_refusals():
    xq, xs, q, s, _ = _problem(8, 32, 64)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.linear_w4a8(xq[:, :48].contiguous(), xs, q[:, :24].contiguous(), s)
    with pytest.raises(TypeError):
        ops.linear_w4a8(xq.float().to(torch.bfloat16), xs, q, s)
    with pytest.raises(TypeError):
        ops.linear_w4a8(xq, xs, q.view(F8), s)
    with pytest.raises(ValueError, match="expected q"):
        ops.linear_w4a8(xq, xs, q, s[:, :1])
    with pytest.raises(RuntimeError, match="xscale"):
        ops.linear_w4a8(xq, xs[:4], q, s)


@pytest.mark.parametrize("act", [None, "gelu", "silu", "relu"])
def test_epilogue(act):
    """Bias, activation, residual and alpha, into a strided ``out`` inside a buffer of
    sentinels (8-byte aligned and unaligned column offsets: vector and scalar stores)."""
    M, N, K = 200, 208, 416
    xq, xs, q, s, ref = _problem(M, N, K, seed=1)
    bias, res = _rand(N, seed=2), _rand(M, N, seed=3)
    alpha = 0.37
    want = ops._act_ref(alpha * ref + bias.float(), act) + res.float()
    for col0 in (8, 3):
        for cfg in [None] + _configs():
            big = torch.full((M + 5, N + 22), 1000.0, dtype=torch.bfloat16, device=DEV)
            out = big[2:2 + M, col0:col0 + N]
            ops.linear_w4a8(xq, xs, q, s, bias, act=act, residual=res, alpha=alpha, out=out, config=cfg)
            _close(out, want)
            mask = torch.ones_like(big, dtype=torch.bool)
            mask[2:2 + M, col0:col0 + N] = False
            assert (big[mask] == 1000.0).all(), f"config {cfg}"


@pytest.mark.parametrize("N", [64, 224])
def test_swiglu_interleaved_rows(N):
    """The gate/up interleave moves a row's nibble bytes and its block scales together."""
    M, K = 130, 160
    xq, xs, q, s, ref = _problem(M, N, K, seed=6)
    bias = _rand(N, seed=7)
    F = N // 2
    y = ref + bias.float()
    want = torch.nn.functional.silu(y[:, :F]) * y[:, F:]
    qi, si, bi = ops.interleave_gate_up(q), ops.interleave_gate_up(s), ops.interleave_gate_up(bias)
    for cfg in [None] + _configs():
        out = ops.linear_w4a8(xq, xs, qi, si, bi, act="swiglu", config=cfg)
        assert out.shape == (M, F)
        _close(out, want)


@pytest.mark.parametrize("M,N,K,col0", [(77, 130, 224, 8), (77, 130, 224, 3), (200, 48, 832, 8), (1, 64, 64, 5)])
def test_no_stray_writes(M, N, K, col0):
    """``out`` is a view inside a larger buffer of sentinels: nothing outside it changes (row
    and column tails, K no multiple of a slice; 8-byte aligned and unaligned views: vector and
    scalar stores)."""
    xq, xs, q, s, ref = _problem(M, N, K, seed=8)
    sentinel = 1000.0  # a bf16 value
    for cfg in [None] + _configs():
        big = torch.full((M + 5, N + 22), sentinel, dtype=torch.bfloat16, device=DEV)
        out = big[2:2 + M, col0:col0 + N]
        ops.linear_w4a8(xq, xs, q, s, out=out, config=cfg)
        _close(out, ref)
        mask = torch.ones_like(big, dtype=torch.bool)
        mask[2:2 + M, col0:col0 + N] = False
        assert (big[mask] == sentinel).all(), f"config {cfg}"


def test_two_runs_are_bitwise_equal():
    xq, xs, q, s, ref = _problem(200, 208, 1024, seed=9)
    bias, res = _rand(208, seed=10), _rand(200, 208, seed=11)
    for cfg in [None] + _configs():
        a = ops.linear_w4a8(xq, xs, q, s, bias, act="gelu", residual=res, config=cfg)
        b = ops.linear_w4a8(xq, xs, q, s, bias, act="gelu", residual=res, config=cfg)
        assert torch.equal(a, b), f"config {cfg}"


def test_caller_workspace():
    M, N, K = 64, 128, 1024
    xq, xs, q, s, ref = _problem(M, N, K, seed=12)
    ws = torch.empty(4 * M * N, dtype=torch.float32, device=DEV)
    _close(ops.linear_w4a8(xq, xs, q, s, config=(2, 4), workspace=ws), ref)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.linear_w4a8(xq, xs, q, s, config=(2, 4), workspace=ws[:M * N])
    # the helper sizes the automatic config's slabs: Llama's down projection splits K, gate/up does not
    _, sk = ops.ext().gemm_w4a8_pick(512, 4096, 14336)
    assert sk > 1 and ops.w4a8_workspace_elems(512, 4096, 14336) == sk * 512 * 4096
    assert ops.w4a8_workspace_elems(512, 28672, 4096) == 0


# -------------------------------------------------------------------------------- quantiser
def test_device_quantiser_matches_host():
    g = torch.Generator().manual_seed(21)
    w = (0.02 * torch.randn(200, 416, generator=g)).to(torch.bfloat16)
    w[3, 32:64] = 0  # an all-zero block
    w[5] *= 2.0 ** 20
    w[7] *= 2.0 ** -20
    q, s = ops.quantize_mxfp4(w)
    qd, sd = ops.quantize_mxfp4(w.to(DEV))
    assert qd.is_cuda and qd.dtype == torch.uint8 and sd.dtype == torch.uint8
    assert torch.equal(qd.cpu(), q) and torch.equal(sd.cpu(), s)
    assert torch.equal(ops.dequantize_mxfp4(qd, sd).cpu(), ops.dequantize_mxfp4(q, s))


# --------------------------------------------------------------------------------- executor
# Measured on the CPU (the project's CPU executor backend with weight_dtype="mxfp4",
# act_dtype="fp8" against reference.forward(act_dtype="fp8") on the same store, seq=64, batch=2),
# as (max-abs error / max |logit|, rms-relative error): mini-gpt2 0.0599 and 0.0507, mini-llama
# 0.0614 and 0.0592. Both backends are held to 2 x those values (tests/test_mxfp4_cpu.py holds the
# CPU executor to the same rule): an upstream bf16 step can flip an e4m3 rounding of a GEMM input,
# so the bound catches plumbing errors; the arithmetic rests on the exact kernel tests above.
EXEC_CPU = {"mini-gpt2": (0.0599, 0.0507), "mini-llama": (0.0614, 0.0592)}


def _check(p, ex, store):
    out = ex.output("output_projection").float().cpu()
    B, S = out.shape[0], out.shape[1]
    tok = synthetic_tokens("@tokens", B * S, p.cfg.vocab_size).view(B, S)
    ref = reference.forward(p.cfg, store, tok, act_dtype="fp8")
    d = out - ref
    maxrel = d.abs().max().item() / ref.abs().max().item()
    rmsrel = (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    print(f"{p.cfg.name}: max-abs / max-|logit| {maxrel:.4f}, rms-relative {rmsrel:.4f}")
    cmax, crms = EXEC_CPU[p.cfg.name]
    assert maxrel <= 2 * cmax and rmsrel <= 2 * crms, (maxrel, rmsrel)


@pytest.mark.parametrize("model", ["mini-gpt2", "mini-llama"])
@pytest.mark.parametrize("graph", [False, True])
def test_mxfp4_dag_on_gpu_matches_reference(model, graph):
    p = runtime.plan(model, world=1, seq=64, batch=2, weight_dtype="mxfp4", act_dtype="fp8")
    assert p.completed == p.total and p.args["weight_dtype"] == "mxfp4"
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, torch.device("cuda:0"), store, use_graph=graph)
    ex.step()
    if graph:
        assert ex.capture()  # the whole step is one captured graph, nothing allocated inside
        ex.step()
        first = ex.output("output_projection").clone()
        ex.step()
        assert torch.equal(ex.output("output_projection"), first)  # a second replay is bitwise equal
    torch.cuda.synchronize()
    _check(p, ex, store)


def test_mxfp4_memory_capped_reloads_on_gpu():
    """A cap below the parameter bytes forces refills into other arena regions (mini-llama: the
    SwiGLU interleave of q and s must have reached the host image the refills copy)."""
    full = runtime.plan("mini-llama", world=1, seq=64, batch=2, weight_dtype="mxfp4", act_dtype="fp8")
    need = sum(runtime.make_store(full).nbytes(g) for g in full.groups) / 1e9
    p = runtime.plan("mini-llama", world=1, seq=64, batch=2, cap_gb=need * 0.6, weight_dtype="mxfp4",
                     act_dtype="fp8")
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, torch.device("cuda:0"), store, use_graph=False)
    for _ in range(2):
        st = ex.step()
    assert st.param_fills > 0
    torch.cuda.synchronize()
    _check(p, ex, store)
