"""The one-pass finish of the K-grouped GEMM tiles (configs 16, 17, 20, 27, 45).

After the K loop every K group writes its fp32 fragments to an LDS region of its own; after one
barrier each thread sums its 16-byte row segment over the regions, applies the epilogue and
stores it. tests/test_gemm_epilogue_gpu.py holds configs 45, 17 and 20 to seven epilogues on
ragged M and the three N alignments; this file adds what the new pass can get wrong on top of
that: the two configs that file lacks, the edges of the thread <-> segment mapping (one row, one
segment, a second row tile with a single row), the launches that walk several tiles per workgroup
(row range, persistent, grouped) and run-to-run determinism (the output path has no atomics, so
a missed barrier shows as a difference between two runs).

Shapes: K = 4 K-steps of the config (the ring wraps, every K group runs more than one step);
N = 144 (whole 16-byte segments), 100 (8-byte rows, a segment straddles N) and 130 (unaligned
rows: scalar stores, scalar operand requests). References are fp32 PyTorch on the CPU, computed
once per shape; tolerances are those of tests/test_gemm_epilogue_gpu.py (bf16 output rounding,
2^-8 relative, plus the bf16 rounding of the folded weights on the norm epilogues).
"""
import functools

import pytest
import torch

from distributed_llm_scheduler_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"

ONE_PASS = [16, 17, 20, 27, 45]
TOL = {"bias": 2e-2, "bias_res": 2e-2, "bias_res_stats": 2e-2, "ln_ext": 3e-2, "ln_ext_gelu": 3e-2, "ln_in": 3e-2}


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
        "x": _rand(M, K, scale=2.0, seed=300) + 0.4,
        "w": _rand(N, K, scale=0.04, seed=301),
        "bias": _rand(N, scale=0.2, seed=302),
        "res": _rand(M, N, seed=303),
        "nw": (1 + 0.2 * _rand(K, seed=304).float()).to(torch.bfloat16),
        "nb": _rand(K, scale=0.1, seed=305),
    }
    xf = cpu["x"].float()
    cpu["stats"] = torch.stack([xf.sum(1), (xf * xf).sum(1)], 1)
    dev = {k: v.to(DEV) for k, v in cpu.items()}
    dev["layernorm"] = ops.derive_norm_gemm(dev["w"], dev["nw"], dev["nb"], dev["bias"])
    return cpu, dev


@functools.lru_cache(maxsize=None)
def _reference(M, N, K, epi):
    c, _ = _operands(M, N, K)
    if epi == "bias":
        return ops.ref_linear(c["x"], c["w"], c["bias"])
    if epi in ("bias_res", "bias_res_stats"):
        return ops.ref_linear(c["x"], c["w"], c["bias"], None, c["res"])
    xn = ops.ref_layernorm(c["x"], c["nw"], c["nb"])
    return ops.ref_linear(xn, c["w"], c["bias"], "gelu" if epi == "ln_ext_gelu" else None)


def _run(config, M, N, K, epi):
    """One launch of ``epi`` on ``config``; returns (output, emitted statistics or None)."""
    _, d = _operands(M, N, K)
    g = ops.ext().gemm
    if epi == "bias":
        return g(d["x"], d["w"], d["bias"], None, 0, 1.0, None, config, 1), None
    if epi == "bias_res":
        return g(d["x"], d["w"], d["bias"], d["res"], 0, 1.0, None, config, 1), None
    if epi == "bias_res_stats":
        st = torch.zeros(M, 2, dtype=torch.float32, device=DEV)
        y = g(d["x"], d["w"], d["bias"], d["res"], 0, 1.0, None, config, 1, None, 0, 1e-5, None, False, None, None, 1, 2,
              0, st, None)
        return y, st
    wd, cs, bd = d["layernorm"]
    ext = None if epi == "ln_in" else d["stats"]
    y = g(d["x"], wd, bd, None, 1 if epi == "ln_ext_gelu" else 0, 1.0, None, config, 1, cs, 1, 1e-5, None, False, None,
          None, 1, 2, 0, None, ext)
    return y, None


def _check(config, M, N, epi):
    K = 4 * ops.ext().gemm_glds_kstep(config)
    y, st = _run(config, M, N, K, epi)
    torch.cuda.synchronize()
    assert y.shape == (M, N)
    _close(y.cpu(), _reference(M, N, K, epi), TOL[epi])
    if st is not None:
        yf = y.cpu().float()
        ref = torch.stack([yf.sum(1), (yf * yf).sum(1)], 1)
        assert torch.allclose(st.cpu(), ref, rtol=1e-4, atol=1e-2), (st.cpu() - ref).abs().max()


@pytest.mark.parametrize("epi", ["bias_res_stats", "ln_ext_gelu", "ln_in"])
@pytest.mark.parametrize("N", [144, 100, 130])
@pytest.mark.parametrize("config", [16, 27])
def test_onepass_configs_16_and_27(config, N, epi):
    _check(config, 77, N, epi)


# M = 1: one row of one tile; N = 8: one segment, most threads idle; M = 33, N = 48: one column
# tile (a whole one for the 48-column configs), a second row tile with one row on the 32-row ones
@pytest.mark.parametrize("epi", ["bias_res_stats", "ln_ext_gelu"])
@pytest.mark.parametrize("M,N", [(1, 144), (77, 8), (33, 48)])
@pytest.mark.parametrize("config", ONE_PASS)
def test_onepass_edges(config, M, N, epi):
    _check(config, M, N, epi)


@pytest.mark.parametrize("N", [144, 130])
@pytest.mark.parametrize("config", [45, 17])
def test_onepass_ln_in_several_row_tiles(config, N):
    """A folded norm without handed-over statistics, on more than one M tile. (K-grouped tiles
    take no in-kernel row statistics: the launcher hands such a launch to config 3, so no
    statistics area sits next to the fragment regions — this holds that routing.)"""
    _check(config, 300, N, "ln_in")


def test_onepass_row_range():
    """A device-side row range on config 17: each workgroup walks the range's M tiles of its
    column panel (three tiles, the last one ragged), one barrier between tiles."""
    M, N, K, r0, r1 = 256, 128, 256, 37, 200
    x, w = _rand(M, K, seed=310), _rand(N, K, scale=0.05, seed=311)
    xd, wd = x.to(DEV), w.to(DEV)
    out = torch.full((M, N), 7.0, dtype=torch.bfloat16, device=DEV)
    rows = torch.tensor([r0, r1], dtype=torch.int32, device=DEV)
    ops.ext().gemm(xd, wd, None, None, 0, 1.0, out, 17, 1, None, 0, 1e-5, rows)
    torch.cuda.synchronize()
    o = out.cpu().float()
    assert (o[:r0] == 7.0).all() and (o[r1:] == 7.0).all(), "rows outside the range were written"
    _close(o[r0:r1], ops.ref_linear(x[r0:r1], w).float(), 2e-2)


def test_onepass_persistent_more_tiles_than_workgroups():
    """Config 17 persistent (two resident workgroups per CU at most: 512 on 256 CUs) over
    6 x 176 = 1056 tiles with bias and residual: every workgroup finishes a tile, passes the
    barrier between tiles and refills the staging buffers that held the fragments."""
    M, N, K = 330, 11264, 256
    x, w = _rand(M, K, seed=320), _rand(N, K, scale=0.05, seed=321)
    bias, res = _rand(N, scale=0.2, seed=322), _rand(M, N, seed=323)
    y = ops.ext().gemm(x.to(DEV), w.to(DEV), bias.to(DEV), res.to(DEV), 0, 1.0, None, 17 + ops.ext().PERSIST, 1)
    torch.cuda.synchronize()
    _close(y.cpu(), ops.ref_linear(x, w, bias, None, res), 2e-2)


def test_onepass_grouped_two_groups():
    """Two groups in one grouped launch on config 17: 70 rows (two row tiles, the second with 6
    rows) and 33 rows, each with its own weight, into the rows' own positions."""
    K, N, counts = 256, 144, [70, 33]
    R = sum(counts)
    x = _rand(R, K, seed=330)
    ws = [_rand(N, K, scale=0.05, seed=331 + e) for e in range(2)]
    xd, wd = x.to(DEV), [w.to(DEV) for w in ws]
    off = torch.tensor([0, counts[0], R], dtype=torch.int32, device=DEV)
    wp = torch.tensor([w.data_ptr() for w in wd], dtype=torch.int64, device=DEV)
    out = torch.full((R, N), 5.0, dtype=torch.bfloat16, device=DEV)
    ops.ext().gemm_grouped(xd, wd, wp, off, 0, out, [], None, 17)
    torch.cuda.synchronize()
    o = out.cpu()
    _close(o[:70], ops.ref_linear(x[:70], ws[0]).float(), 2e-2)
    _close(o[70:], ops.ref_linear(x[70:], ws[1]).float(), 2e-2)


@pytest.mark.parametrize("epi", ["bias_res", "ln_ext_gelu"])
@pytest.mark.parametrize("config", [45, 17])
def test_onepass_is_deterministic(config, epi):
    M, N = 300, 144
    K = 4 * ops.ext().gemm_glds_kstep(config)
    y1, _ = _run(config, M, N, K, epi)
    y2, _ = _run(config, M, N, K, epi)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)
    _close(y1.cpu(), _reference(M, N, K, epi), TOL[epi])
