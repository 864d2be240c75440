"""Epilogues of the LDS-DMA GEMM as a model step attaches them, on the tile configs the steps run.

The K-group configs (45: four groups, 17: two, 20: four groups of 16 waves) sum their groups'
accumulators through LDS and request every epilogue operand (external row statistics, bias,
column sums, residual) in one batch right after the main loop, from clamped addresses; config 13
(no K groups, split rings) keeps the in-place loads. Shapes are the smallest that reach every
path: ragged M (a tile with idle rows, more than one M tile), N = 144 (aligned 16-byte segments,
several 48-column tiles), 100 (rows 8-byte aligned, an 8-column chunk straddles N) and 130
(unaligned rows: scalar stores and scalar operand requests), K = 4 K-steps (the ring wraps and
every K group runs more than one step). References are fp32 PyTorch on the CPU, computed once
per shape.
"""
import functools

import pytest
import torch

from distributed_llm_scheduler_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

CONFIGS = [45, 17, 13, 20]
MS = [77, 300]
NS = [144, 100, 130]
EPILOGUES = ["bias", "bias_res", "bias_res_stats", "ln_ext", "ln_ext_gelu", "ln_in", "rms_ext"]


def _rand(*shape, scale=1.0, dtype=torch.bfloat16, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(dtype)


def _close(a, b, tol):
    err = (a.float() - b.float()).abs().max().item()
    ref = b.float().abs().max().item() + 1e-6
    assert err <= tol * ref, f"max abs err {err:.4g} vs ref max {ref:.4g} (rel tol {tol})"


@functools.lru_cache(maxsize=None)
def _operands(M, N, K):
    """CPU operands (random, asymmetric, rows with a non-zero mean) and device copies."""
    cpu = {
        "x": _rand(M, K, scale=2.0, seed=200) + 0.4,
        "w": _rand(N, K, scale=0.04, seed=201),
        "bias": _rand(N, scale=0.2, seed=202),
        "res": _rand(M, N, seed=203),
        "nw": (1 + 0.2 * _rand(K, seed=204).float()).to(torch.bfloat16),
        "nb": _rand(K, scale=0.1, seed=205),
    }
    xf = cpu["x"].float()
    cpu["stats"] = torch.stack([xf.sum(1), (xf * xf).sum(1)], 1)
    dev = {k: v.to(DEV) for k, v in cpu.items()}
    for mode in ("layernorm", "rmsnorm"):
        dev[mode] = ops.derive_norm_gemm(dev["w"], dev["nw"], dev["nb"] if mode == "layernorm" else None, dev["bias"])
    return cpu, dev


@functools.lru_cache(maxsize=None)
def _reference(M, N, K, epi):
    c, _ = _operands(M, N, K)
    if epi == "bias":
        return ops.ref_linear(c["x"], c["w"], c["bias"])
    if epi in ("bias_res", "bias_res_stats"):
        return ops.ref_linear(c["x"], c["w"], c["bias"], None, c["res"])
    if epi == "rms_ext":
        xn = ops.ref_rmsnorm(c["x"], c["nw"])
    else:
        xn = ops.ref_layernorm(c["x"], c["nw"], c["nb"])
    return ops.ref_linear(xn, c["w"], c["bias"], "gelu" if epi == "ln_ext_gelu" else None)


def _run(config, M, N, K, epi, out=None, res=None):
    """One launch of ``epi`` on ``config``; returns (output, emitted statistics or None)."""
    _, d = _operands(M, N, K)
    g = ops.ext().gemm
    if epi == "bias":
        return g(d["x"], d["w"], d["bias"], None, 0, 1.0, out, config, 1), None
    if epi == "bias_res":
        return g(d["x"], d["w"], d["bias"], d["res"] if res is None else res, 0, 1.0, out, config, 1), None
    if epi == "bias_res_stats":
        st = torch.zeros(M, 2, dtype=torch.float32, device=DEV)
        y = g(d["x"], d["w"], d["bias"], d["res"] if res is None else res, 0, 1.0, out, config, 1, None, 0, 1e-5,
              None, False, None, None, 1, 2, 0, st, None)
        return y, st
    mode = "rmsnorm" if epi == "rms_ext" else "layernorm"
    wd, cs, bd = d[mode]
    ext = None if epi == "ln_in" else d["stats"]
    act = 1 if epi == "ln_ext_gelu" else 0
    y = g(d["x"], wd, bd, None, act, 1.0, out, config, 1, cs, 2 if mode == "rmsnorm" else 1, 1e-5, None, False, None,
          None, 1, 2, 0, None, ext)
    return y, None


def _check_stats(st, y):
    yf = y.cpu().float()
    ref = torch.stack([yf.sum(1), (yf * yf).sum(1)], 1)
    assert torch.allclose(st.cpu(), ref, rtol=1e-4, atol=1e-2), (st.cpu() - ref).abs().max()


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("config", CONFIGS)
def test_gemm_step_epilogues(config, M, N, epi):
    K = 4 * ops.ext().gemm_glds_kstep(config)
    y, st = _run(config, M, N, K, epi)
    torch.cuda.synchronize()
    _close(y.cpu(), _reference(M, N, K, epi), 3e-2 if epi in ("ln_ext", "ln_ext_gelu", "ln_in", "rms_ext") else 2e-2)
    if st is not None:
        _check_stats(st, y)


# ldc (= ldr) of the padded buffers: 16-byte rows for N = 144 and 100 (whole 16-B segments, and a
# segment that straddles N), odd for N = 130 (scalar stores and scalar operand requests)
PADDED_LD = {144: 152, 100: 104, 130: 133}


@pytest.mark.parametrize("epi", ["bias_res_stats", "ln_ext_gelu"])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("config", CONFIGS)
def test_gemm_epilogue_keeps_the_canary(config, N, epi):
    """Output (and residual) as views into padded buffers: rows past M and the bytes after each
    row's N-th column must stay as they were — the clamped operand requests are loads only."""
    M, PAD_ROWS, CANARY = 77, 9, -7.0
    K = 4 * ops.ext().gemm_glds_kstep(config)
    ld = PADDED_LD[N]
    _, d = _operands(M, N, K)
    buf = torch.full((M + PAD_ROWS, ld), CANARY, dtype=torch.bfloat16, device=DEV)
    rbuf = torch.full((M + PAD_ROWS, ld), CANARY, dtype=torch.bfloat16, device=DEV)
    rbuf[:M, :N] = d["res"]
    y, st = _run(config, M, N, K, epi, out=buf[:M, :N], res=rbuf[:M, :N])
    torch.cuda.synchronize()
    _close(buf[:M, :N].cpu(), _reference(M, N, K, epi), 3e-2 if epi == "ln_ext_gelu" else 2e-2)
    if st is not None:
        _check_stats(st, buf[:M, :N])
    assert bool((buf[M:] == CANARY).all()), "rows past M were written"
    assert bool((buf[:M, N:] == CANARY).all()), "bytes past column N were written"
    assert bool((rbuf[M:] == CANARY).all()) and bool((rbuf[:M, N:] == CANARY).all()), "the residual was written"
    assert torch.equal(rbuf[:M, :N], d["res"]), "the residual was written"
