"""The fp8-weight GEMM (csrc/kernels/gemm_w8.hip) and the fp8 executor mode on the GPU.

Kernel reference: ``(x.float() @ q.float().T) * scale`` in fp32 — the same e4m3 values the
kernel multiplies, so quantisation error cancels and what remains is bf16 output rounding
(2^-9 relative) plus fp32 summation order: far inside the 2e-2 of ``_close`` (the measure of
tests/test_kernels_gpu.py)."""
import pytest
import torch

from distributed_llm_scheduler_amd import ops
from distributed_llm_scheduler_amd.models import reference
from distributed_llm_scheduler_amd.parallel import runtime
from distributed_llm_scheduler_amd.parallel.executor import synthetic_tokens

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-2


def _configs():
    return [(c, s) for c in range(ops.w8_configs()) for s in ops.W8_SPLITS]


def _close(a, b, tol=TOL):
    err = (a.float() - b.float()).abs().max().item()
    ref = b.float().abs().max().item() + 1e-6
    assert err <= tol * ref, f"max abs err {err:.4g} vs ref max {ref:.4g} (rel tol {tol})"


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(torch.bfloat16).to(DEV)


def _problem(M, N, K, seed=0):
    """x bf16 [M, K], q e4m3 [N, K] (quantised N(0, 0.02) weights), arbitrary fp32 scales in
    [1e-3, 10] (a checkpoint quantised elsewhere), and the fp32 reference product."""
    g = torch.Generator(device="cpu").manual_seed(100 + seed)
    x = _rand(M, K, seed=seed)
    q, _ = ops.quantize_fp8((0.02 * torch.randn(N, K, generator=g)).to(torch.bfloat16))
    scale = torch.exp(torch.empty(N).uniform_(-6.9077, 2.3026, generator=g)).clamp_(1e-3, 10.0)
    q, scale = q.to(DEV), scale.to(DEV)
    ref = (x.float() @ q.float().t()) * scale
    return x, q, scale, ref


def test_all_codes_bit_exact():
    """x = I: the output is the dequantised weight, transposed, bit for bit — every finite e4m3
    code (subnormals, +-0, +-448) through the conversion, for every config."""
    M = K = 256
    N = 272  # a tail for the 64- and 128-wide tiles
    codes = torch.arange(256, dtype=torch.uint8)
    codes = codes[(codes & 0x7F) != 0x7F]
    assert codes.numel() == 254
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    qb = codes[(3 * n + k) % 254]  # asymmetric: q[n][k] != q[k][n]; every row holds every code
    assert all(set(qb[r].tolist()) == set(codes.tolist()) for r in (0, N - 1))
    q = qb.contiguous().view(torch.float8_e4m3fn).to(DEV)
    scale = (2.0 ** ((torch.arange(N) % 13) - 8).float()).to(DEV)  # 2^-8 .. 2^4
    x = torch.eye(M, dtype=torch.bfloat16, device=DEV)
    want = ops.dequantize_fp8(q, scale).t().contiguous()
    assert torch.equal(want.float(), (q.float() * scale[:, None]).t())  # exactly bf16 values

    def bits(t):
        # the sign of a zero is the one thing a sum cannot keep: the accumulator starts at +0 and
        # (+0) + (-0) = +0 in round-to-nearest, whatever the conversion gives for code 0x80
        return torch.where(t == 0, torch.zeros_like(t), t).view(torch.int16)

    assert (want == 0).sum().item() >= 2 * N  # both zero codes are in every row
    for cfg in [None] + _configs():
        y = ops.linear_w8(x, q, scale, config=cfg)
        assert y.dtype == torch.bfloat16 and y.shape == (M, N)
        assert torch.equal(bits(y), bits(want)), f"config {cfg}"


SHAPES = [(1, 64, 64), (77, 130, 208), (200, 48, 832), (512, 2304, 768), (512, 768, 3072)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_shapes_every_config(M, N, K):
    x, q, scale, ref = _problem(M, N, K)
    for cfg in [None] + _configs():
        y = ops.linear_w8(x, q, scale, config=cfg)
        assert y.shape == (M, N)
        _close(y, ref)


def test_k_not_a_multiple_of_16_is_refused():
    x, q, scale, _ = _problem(8, 32, 208)
    with pytest.raises(RuntimeError, match="K % 16"):
        ops.linear_w8(x[:, :200].contiguous(), q[:, :200].contiguous(), scale)
    with pytest.raises(TypeError):
        ops.linear_w8(x, q.float().to(torch.bfloat16), scale)


@pytest.mark.parametrize("act", [None, "gelu", "silu"])
def test_epilogue(act):
    M, N, K = 256, 384, 512
    x, q, scale, ref = _problem(M, N, K, seed=1)
    bias, res = _rand(N, seed=2), _rand(M, N, seed=3)
    alpha = 0.37
    want = ops._act_ref(alpha * ref + bias.float(), act) + res.float()
    for cfg in [None] + _configs():
        _close(ops.linear_w8(x, q, scale, bias, act=act, residual=res, alpha=alpha, config=cfg), want)


def test_epilogue_relu_and_plain_bias():
    x, q, scale, ref = _problem(64, 96, 128, seed=4)
    bias = _rand(96, seed=5)
    for cfg in _configs():
        _close(ops.linear_w8(x, q, scale, bias, act="relu", config=cfg), torch.relu(ref + bias.float()))


def test_swiglu_interleaved_rows():
    M, N, K = 130, 256, 192
    x, q, scale, ref = _problem(M, N, K, seed=6)
    bias = _rand(N, seed=7)
    F = N // 2
    y = ref + bias.float()
    want = torch.nn.functional.silu(y[:, :F]) * y[:, F:]
    qi = ops.interleave_gate_up(q.view(torch.uint8)).view(torch.float8_e4m3fn)
    si, bi = ops.interleave_gate_up(scale), ops.interleave_gate_up(bias)
    for cfg in [None] + _configs():
        out = ops.linear_w8(x, qi, si, bi, act="swiglu", config=cfg)
        assert out.shape == (M, F)
        _close(out, want)


@pytest.mark.parametrize("M,N,K,col0", [(77, 130, 208, 8), (77, 130, 208, 3), (200, 48, 832, 8), (1, 64, 64, 5)])
def test_no_stray_writes(M, N, K, col0):
    """``out`` is a view inside a larger buffer of sentinels: nothing outside it changes (row
    and column tails; 8-byte aligned and unaligned views: vector and scalar stores)."""
    x, q, scale, ref = _problem(M, N, K, seed=8)
    sentinel = 1000.0  # a bf16 value
    for cfg in [None] + _configs():
        big = torch.full((M + 5, N + 22), sentinel, dtype=torch.bfloat16, device=DEV)
        out = big[2:2 + M, col0:col0 + N]
        ops.linear_w8(x, q, scale, out=out, config=cfg)
        _close(out, ref)
        mask = torch.ones_like(big, dtype=torch.bool)
        mask[2:2 + M, col0:col0 + N] = False
        assert (big[mask] == sentinel).all(), f"config {cfg}"


def test_split_k_is_deterministic():
    x, q, scale, ref = _problem(512, 768, 3072, seed=9)
    bias, res = _rand(768, seed=10), _rand(512, 768, seed=11)
    for cfg in [c for c in _configs() if c[1] > 1]:
        a = ops.linear_w8(x, q, scale, bias, act="gelu", residual=res, config=cfg)
        b = ops.linear_w8(x, q, scale, bias, act="gelu", residual=res, config=cfg)
        assert torch.equal(a, b), f"config {cfg}"


def test_caller_workspace():
    M, N, K = 64, 128, 1024
    x, q, scale, ref = _problem(M, N, K, seed=12)
    ws = torch.empty(4 * M * N, dtype=torch.float32, device=DEV)
    _close(ops.linear_w8(x, q, scale, config=(2, 4), workspace=ws), ref)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.linear_w8(x, q, scale, config=(2, 4), workspace=ws[:M * N])


def test_device_quantiser_matches_host():
    w = _rand(200, 96, scale=0.02, seed=13)
    w[3] = 0
    q, s = ops.quantize_fp8(w)
    qc, sc = ops.quantize_fp8(w.cpu())
    assert torch.equal(q.cpu().view(torch.uint8), qc.view(torch.uint8)) and torch.equal(s.cpu(), sc)


# ------------------------------------------------------------------------------ executor
def _check(p, ex, store, tol):
    out = ex.output("output_projection").float().cpu()
    B, S = out.shape[0], out.shape[1]
    tok = synthetic_tokens("@tokens", B * S, p.cfg.vocab_size).view(B, S)
    ref = reference.forward(p.cfg, store, tok)
    err, scale = (out - ref).abs().max().item(), ref.abs().max().item()
    assert err < tol * scale, (err, scale)


@pytest.mark.parametrize("model", ["mini-gpt2", "mini-llama"])
@pytest.mark.parametrize("graph", [False, True])
def test_fp8_dag_on_gpu_matches_reference(model, graph):
    p = runtime.plan(model, world=1, seq=64, batch=2, weight_dtype="fp8")
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, torch.device("cuda:0"), store, use_graph=graph)
    ex.step()
    if graph:
        assert ex.capture()
        ex.step()
    torch.cuda.synchronize()
    _check(p, ex, store, 0.03)


def test_fp8_memory_capped_reloads_on_gpu():
    full = runtime.plan("mini-gpt2", world=1, seq=64, weight_dtype="fp8")
    need = sum(runtime.make_store(full).nbytes(g) for g in full.groups) / 1e9
    p = runtime.plan("mini-gpt2", world=1, seq=64, cap_gb=need * 0.6, weight_dtype="fp8")
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, torch.device("cuda:0"), store, use_graph=False)
    for _ in range(2):
        st = ex.step()
    assert st.param_fills > 0
    torch.cuda.synchronize()
    _check(p, ex, store, 0.03)
