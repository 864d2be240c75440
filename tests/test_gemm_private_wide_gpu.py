"""The wave-private rings on 64-row tiles (config ids 130..133, csrc/kernels/gemm_private.hip:
gemm_private_wide_kernel): 64 x 96 and 64 x 80 tiles whose W waves each multiply the whole tile
over a K slice of their own from an LDS ring of S slots of their own, meet at one barrier and
finish the tile's 16-byte segments in passes with the folded-norm epilogue (row statistics handed
over in ``ext_stats``), bias and no activation or GeLU.

Exact probes (gemm_cases.py: integer, scaled, selector — one right answer in every summation
order) run with a folded norm whose factors are exact: ``ext_stats`` rows are (mu K, 0) and
``ln_eps`` is 1, so the variance clamps to 0, rstd = rsqrt(1) = 1 and the kernel forms
``x - mu * colsum + bias`` from integers (LayerNorm mode; mu in {-2, -1, 1, 2}, colsum an integer in
[-3, 3], the test asserts that fp32 ``(mu K) * (1 / K)`` is mu exactly) or ``x + bias`` (RMSNorm
mode, which must ignore the handed-over sum). Without an activation the output is compared with
``torch.equal``. GeLU of these exact integers is not exact: the kernel's fp32 tanh form is rounded
to bf16 once, so it is held to one bf16 ulp (2^-7 relative) of the float64 GeLU of the exact value
v — plus 2^-21 |v| where that GeLU is next to zero: 0.5 v (1 + tanh) carries the fp32 rounding of
1 + tanh, a few ulps of 1 — and every repetition to bit-equality with the first. Shapes: one full
tile and the ragged ones of
profiles/epilogue_onepass/outputs.txt (M 64 / 77; N = BN, 144, 100 — unaligned rows — and 130 —
operands read in place), K = W x 64 x {1, S, S + 1, 2 S + 1}: every state of the ring. Every probe
runs from cold and from warm caches, and once on NaN-padded operands into a canary buffer.

Random asymmetric operands are held to the fp32 reference of ``ops`` at the tolerance
tests/test_kernels_gpu.py applies to the folded-norm GEMMs (3e-2 of the largest reference value),
at the ragged shapes and at the two flagship shapes. The family refuses — an error, nothing
launched — every launch it does not attach.
"""
import functools

import pytest
import torch

import gemm_cases as gc
import gemm_checks as gk
from distributed_llm_scheduler_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

WIDE = {130: (64, 96, 4, 2), 131: (64, 96, 3, 2), 132: (64, 80, 4, 2), 133: (64, 80, 3, 2)}  # id -> (BM, BN, W, S)
TOL = 3e-2  # tests/test_kernels_gpu.py: test_gemm_folded_norm_external_stats and the linear_norm tests
REPS = 4    # launches 0 and 2 follow a 64 MB device fill (cold operands), 1 and 3 run warm
GELU, NONE = 1, 0


def _tsteps(S):
    return sorted({1, S, S + 1, 2 * S + 1})


def _shapes(BN):
    return [(M, N) for M in (64, 77) for N in (BN, 144, 100, 130)]


@functools.lru_cache(maxsize=None)
def _flush():
    return torch.empty(64 << 20, dtype=torch.uint8, device=DEV)


def _gemm(config, x, w, bias, cs, st, mode, act=NONE, eps=1e-5, out=None, **kw):
    return ops.ext().gemm(x, w, bias, None, act, 1.0, out, config, 1, cs, mode, float(eps), None, False, None, None, 1,
                          2, 0, None, st, **kw)


def test_wide_table_matches_the_library():
    e = ops.ext()
    assert e.PRIVATE_WIDE == min(WIDE) and e.PRIVATE_WIDE_COUNT == len(WIDE)
    for c, v in WIDE.items():
        assert tuple(e.gemm_private_wide_cfg(c)) == v


# ---------------------------------------------------------------------------------------------
# Exact probes

@functools.lru_cache(maxsize=None)
def _exact_norm(M, N, K):
    """(stats, colsum, mu): ext_stats rows (mu K, 0) with mu in {-2, -1, 1, 2}, integer column sums."""
    g = torch.Generator().manual_seed(9000 + M + 3 * N + 5 * K)
    mu = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (M,), generator=g)]
    cs = torch.randint(-3, 4, (N,), generator=g).float()
    st = torch.stack([mu * K, torch.zeros(M)], 1)
    # what the kernel computes in fp32: mu = sum * (1 / K), var = max(0 / K - mu^2, 0) = 0
    inv_k = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(K), dtype=torch.float32)
    assert torch.equal(st[:, 0] * inv_k, mu), f"fp32 (mu K) * (1 / K) is not mu at K = {K}"
    return st, cs, mu


@functools.lru_cache(maxsize=None)
def _probe_dev(kind, M, N, K):
    p = gc.probe(kind, M, N, K)
    return p, tuple(None if t is None else t.to(DEV) for t in (p.x, p.w, p.bias))


def _expected(p, bias, mode, cs, mu, act):
    """(value before the activation in float64 — exact —, bf16 expectation)."""
    v = gk.acc64(p.x, p.w)
    if mode == 1:
        v = v - mu.double()[:, None] * cs.double()[None, :]
    if bias is not None:
        v = v + bias.double()
    return v, gk.act64(v, "gelu" if act == GELU else None).to(BF)


def _exact_probes(config, M, N, K):
    st, cs, mu = _exact_norm(M, N, K)
    st_d, cs_d = st.to(DEV), cs.to(DEV)
    for kind in ("integer", "scaled", "selector"):
        p, (x, w, b) = _probe_dev(kind, M, N, K)
        gk.check_probe_preconditions(p, gc.EPI_NONE)
        # bias exists on the integer probe only (gemm_cases.py); the others carry mu = 0: the RMSNorm
        # mode, and the LayerNorm mode on zero sums
        combos = [(1, NONE), (2, NONE), (1, GELU), (2, GELU)] if kind == "integer" else [(2, NONE), (1, NONE)]
        for mode, act in combos:
            integer = kind == "integer"
            bias = p.bias if integer else None
            stats = st_d if (integer or mode == 2) else torch.zeros_like(st_d)
            v, want = _expected(p, bias, mode if integer else 2, cs, mu, act)
            if integer:
                assert v.abs().max().item() <= 256 and bool((v % 1 == 0).all()), "a value bf16 cannot hold"
            what = f"config {config} {kind} mode {mode} act {act} ({M}, {N}, {K})"
            outs = []
            for i in range(REPS):
                if i % 2 == 0:
                    _flush().fill_(i & 255)  # the operands leave the caches before every other launch
                outs.append(_gemm(config, x, w, b if integer else None, cs_d, stats, mode, act, eps=1.0))
            pd = gc.padded(p.x, p.w, None, DEV)
            gk.check_poison_placement(pd, M, N, K)
            _gemm(config, pd.a, pd.w, b if integer else None, cs_d, stats, mode, act, eps=1.0, out=pd.out)
            torch.cuda.synchronize()
            o = pd.obuf.cpu()
            outs.append(o[:M, :N])
            gk.check_canary(pd, M, N, None, what)
            for i, y in enumerate(outs):
                if act == NONE:
                    gk.check_exact(y, want, f"{what} run {i}")
                else:
                    yd, wd = y.cpu().double(), gk.act64(v, "gelu")
                    err, lim = (yd - wd).abs(), 2.0 ** -7 * wd.abs() + 2.0 ** -21 * v.abs()
                    assert bool((err <= lim).all()), f"{what} run {i}: GeLU off by {(err - lim).max().item():.4g}"
                    assert torch.equal(y.cpu(), outs[0].cpu()), f"{what}: run {i} differs from run 0"


def test_wide_exact_probes_cold_and_warm():
    # (one case for the four ids: every message names its config, shape and run)
    for config, (BM, BN, W, S) in sorted(WIDE.items()):
        for t in _tsteps(S):
            for M, N in _shapes(BN):
                _exact_probes(config, M, N, W * 64 * t)


# ---------------------------------------------------------------------------------------------
# fp32 reference, random operands

@functools.lru_cache(maxsize=None)
def _random(M, N, K, mode):
    c = gc.random_operands(M, N, K)
    nb = c["nb"] if mode == "layernorm" else None
    xn = ops.ref_layernorm(c["x"], c["nw"], nb) if mode == "layernorm" else ops.ref_rmsnorm(c["x"], c["nw"])
    ref = {act: ops.ref_linear(xn, c["w"], c["bias"], act=act).float() for act in (NONE, GELU)}
    wd, cs, bd = ops.derive_norm_gemm(c["w"].to(DEV), c["nw"].to(DEV), None if nb is None else nb.to(DEV),
                                      c["bias"].to(DEV))
    return (c["x"].to(DEV), wd, cs, bd, c["stats"].to(DEV)), ref


def _close(y, ref, what):
    err = (y.float() - ref).abs().max().item()
    lim = TOL * (ref.abs().max().item() + 1e-6)
    print(f"{what}: max abs err {err:.4g}, allowed {lim:.4g}")
    assert bool(torch.isfinite(y.float()).all()) and err <= lim, f"{what}: max abs err {err:.4g} > {lim:.4g}"


def test_wide_random_against_fp32_reference():
    for config, (BM, BN, W, S) in sorted(WIDE.items()):
        K = W * 64 * (S + 1)
        for mode in ("layernorm", "rmsnorm"):
            for M, N in [(77, 144), (77, 100), (64 + 77, 130), (64, BN)]:
                (x, wd, cs, bd, st), ref = _random(M, N, K, mode)
                for act in (NONE, GELU):
                    y = _gemm(config, x, wd, bd, cs, st, 1 if mode == "layernorm" else 2, act)
                    torch.cuda.synchronize()
                    assert y.shape == (M, N)
                    _close(y.cpu(), ref[act], f"config {config} {mode} act {act} ({M}, {N}, {K})")


def test_wide_flagship_shapes():
    """512 x 2304 x 768 with QKV's operands and 512 x 3072 x 768 with fc1's (LayerNorm folded in,
    handed-over statistics, bias; GeLU on fc1), under every store policy; twice: bit-identical."""
    for N, act in [(2304, NONE), (3072, GELU)]:
        (x, wd, cs, bd, st), ref = _random(512, N, 768, "layernorm")
        for config in sorted(WIDE):
            ys = [_gemm(config, x, wd, bd, cs, st, 1, act, stream_pol=pol) for pol in (0, 0, 2, 4)]
            torch.cuda.synchronize()
            _close(ys[0].cpu(), ref[act], f"config {config} (512, {N}, 768)")
            for y in ys[1:]:
                assert torch.equal(y, ys[0]), f"config {config} (512, {N}, 768)"


# ---------------------------------------------------------------------------------------------
# Refusals

def test_wide_refuses_what_it_does_not_attach():
    for config in sorted(WIDE):
        _refusals(config)


def _refusals(config):
    """Each of these raises instead of launching: the output buffer keeps its fill."""
    BM, BN, W, S = WIDE[config]
    M, N, K = 40, 64, W * 64 * 2
    g = ops.ext().gemm
    x = torch.ones(M, K, dtype=BF, device=DEV)
    w = torch.ones(N, K, dtype=BF, device=DEV)
    out = torch.full((M, N), 7.0, dtype=BF, device=DEV)
    out_half = torch.full((M, N // 2), 7.0, dtype=BF, device=DEV)
    res = torch.zeros(M, N, dtype=BF, device=DEV)
    cs = torch.zeros(N, dtype=torch.float32, device=DEV)
    st = torch.zeros(M, 2, dtype=torch.float32, device=DEV)
    so = torch.zeros(M, 2, dtype=torch.float32, device=DEV)
    rows = torch.tensor([0, M], dtype=torch.int32, device=DEV)
    cos_t, sin_t = ops.rope_tables(M, 16, 10000.0, DEV)
    xk = torch.ones(M, K + 64, dtype=BF, device=DEV)
    wk = torch.ones(N, K + 64, dtype=BF, device=DEV)
    refused = {
        "k tiles not divisible by W": lambda: g(xk, wk, None, None, 0, 1.0, out, config, 1, cs, 1, 1.0, None, False,
                                                None, None, 1, 2, 0, None, st),
        "no folded norm": lambda: g(x, w, None, None, 0, 1.0, out, config, 1),
        "no ext_stats": lambda: g(x, w, None, None, 0, 1.0, out, config, 1, cs, 1, 1.0),
        "silu": lambda: g(x, w, None, None, 2, 1.0, out, config, 1, cs, 1, 1.0, None, False, None, None, 1, 2, 0, None, st),
        "rope": lambda: g(x, w, None, None, 0, 1.0, out, config, 1, cs, 1, 1.0, None, False, cos_t, sin_t, M, 16, 16,
                          None, st),
        "swiglu": lambda: g(x, w, None, None, 4, 1.0, out_half, config, 1, cs, 1, 1.0, None, False, None, None, 1, 2, 0,
                            None, st),
        "split-K": lambda: g(x, w, None, None, 0, 1.0, out, config, 2, cs, 1, 1.0, None, False, None, None, 1, 2, 0, None,
                             st),
        "row range": lambda: g(x, w, None, None, 0, 1.0, out, config, 1, cs, 1, 1.0, rows, False, None, None, 1, 2, 0,
                               None, st),
        "plain row range": lambda: g(x, w, None, None, 0, 1.0, out, config, 1, None, 0, 1e-5, rows),
        "residual": lambda: g(x, w, None, res, 0, 1.0, out, config, 1, cs, 1, 1.0, None, False, None, None, 1, 2, 0, None,
                              st),
        "stats_out": lambda: g(x, w, None, None, 0, 1.0, out, config, 1, cs, 1, 1.0, None, False, None, None, 1, 2, 0,
                               so, st),
    }
    for what, launch in refused.items():
        with pytest.raises(RuntimeError):
            launch()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((out_half == 7.0).all()), f"{config} {what}: something was launched"
    # and the folded-norm launch of the same operands is taken: rstd = 1, mu = 0 -> K
    g(x, w, None, None, 0, 1.0, out, config, 1, cs, 2, 1.0, None, False, None, None, 1, 2, 0, None, st)
    torch.cuda.synchronize()
    assert bool((out == float(K)).all())
