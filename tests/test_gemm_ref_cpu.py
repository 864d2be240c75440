"""The bf16 GEMM checks, checked on the CPU: the float64 reference against the project's own fp32
one, every precondition of the exact probes at every shape the GPU tests run, a torch model of an
honest kernel that passes every check, and mutants of it that each named check rejects. No GPU,
no native library: the tile table of gemm_cases.py stands in for the binding's accessors (the GPU
tests hold the two to each other).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as C  # noqa: E402
import gemm_checks as K  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

BF = torch.bfloat16
SHAPES = C.probe_shapes()
# the model runs on one shape per tile family: no K groups, two and four K groups (largest K)
MODEL_CONFIGS = [3, 24, 17, 45, 38]


def test_probe_shapes_cover_the_stated_range():
    assert len(C.TILES) == 48 and sorted(C.TILES) == list(range(48))
    assert max(k for _, _, k in SHAPES) == 3072 and min(m for m, _, _ in SHAPES) == 37
    for c in C.ALL_CONFIGS:
        bm, bn, ks = C.tile(c)
        for kind in C.N_KINDS:
            M, N, Kk = C.shape(c, kind)
            assert -(-M // bm) == 2 and M - bm == 5 and -(-N // bn) == 2 and Kk % (ks * 12) == 0
            assert (N % 8 == 0) == (kind == "seg")


@pytest.mark.parametrize("M,N,Kk", SHAPES)
def test_probe_preconditions(M, N, Kk):
    """Integer range, exactness of every intermediate value, full-range selector weights: what
    makes torch.equal the metric. The largest value an integer probe's epilogue forms stays far
    below the 256 bf16 holds for half-integers' neighbours."""
    for kind in C.PROBES:
        p = C.probe(kind, M, N, Kk)
        for epi in (C.EPI_NONE, C.EPI_FULL):
            worst = K.check_probe_preconditions(p, epi)
            if kind == "integer":
                assert worst <= 256
            want = K.expected_exact(p, epi)
            assert want.shape == (M, N)
            if kind == "selector" and epi is C.EPI_NONE:
                assert torch.equal(want, p.w[:, C.selector_k(M, Kk)].T.contiguous())


def test_integer_probe_magnitudes():
    worst = max(K.check_probe_preconditions(C.integer_probe(*s), e) for s in SHAPES for e in (C.EPI_NONE, C.EPI_FULL))
    print(f"largest value of an integer probe: {worst}")
    assert worst <= 200  # |acc| grows like sqrt(0.56 K): 4.3 sigma at K = 3072 is about 180


def test_poison_placement():
    M, N, Kk = C.shape(24, "odd")
    p = C.integer_probe(M, N, Kk)
    pd = C.padded(p.x, p.w, p.res)
    K.check_poison_placement(pd, M, N, Kk)
    assert torch.equal(pd.a, p.x) and torch.equal(pd.w, p.w) and torch.equal(pd.res, p.res)
    assert pd.out.stride(0) == N + 3 and C.out_ld(C.shape(24, "seg")[1]) % 8 == 0


@pytest.mark.parametrize("act", [None, "relu", "gelu", "silu"])
def test_ref64_agrees_with_ref_linear(act):
    """The independent float64 reference, ops.ref_linear and the CPU path of ops.linear agree
    within the bf16 rounding of the output (the two fp32 ones: bit for bit)."""
    M, N, Kk = 77, 130, 256
    c = C.random_operands(M, N, Kk)
    pre, out = K.ref64(c["x"], c["w"], c["bias"], act, c["res"], 0.5)
    mine = ops.ref_linear(c["x"], c["w"], c["bias"], act, c["res"], 0.5)
    assert torch.equal(mine, ops.linear(c["x"], c["w"], c["bias"], act, c["res"], 0.5))
    # one rounding of the fp32 result (ref_linear keeps the sum unrounded): half a bf16 ulp is at
    # most 2^-8 of the value; plus the fp32 accumulation
    err = (mine.double() - out).abs()
    assert bool((err <= 2.0 ** -8 * out.abs() + Kk * 2.0 ** -24 * K.absprod64(c["x"], c["w"])).all())
    K.check_bound(mine, pre, out, K.absprod64(c["x"], c["w"]), Kk, "linear", f"ref_linear {act}", C=2.0)


def test_ref64_folded_norm_and_swiglu_and_rope_agree_with_ops():
    M, N, Kk = 70, 96, 128
    c = C.random_operands(M, N, Kk)
    for mode in ("layernorm", "rmsnorm"):
        wd, cs, bd = ops.derive_norm_gemm(c["w"], c["nw"], c["nb"] if mode == "layernorm" else None, c["bias"])
        for stats in (None, c["stats"]):
            pre, out = K.ref64_folded(c["x"], wd, cs, bd, mode, "gelu", stats)
            xn = ops.ref_layernorm(c["x"], c["nw"], c["nb"]) if mode == "layernorm" else ops.ref_rmsnorm(c["x"], c["nw"])
            mine = ops.ref_linear(xn, c["w"], c["bias"], "gelu")
            assert K.close_global(mine, out.float(), 3e-2)  # (the folded weights are rounded: not one rounding apart)
    sw, _ = K.ref64_swiglu(c["x"], c["w"], c["bias"])
    assert K.close_global(ops.ref_linear(c["x"], c["w"], c["bias"], "swiglu"), sw.float(), 2.0 ** -7)
    cos_t, sin_t = ops.rope_tables(16, 32, 10000.0)
    rp, _ = K.ref64_rope(c["x"], c["w"], c["bias"], cos_t, sin_t, 16, 32, 64)
    assert K.close_global(ops.ref_linear(c["x"], c["w"], c["bias"], rope=(cos_t, sin_t, 16, 32, 64)), rp.float(), 2.0 ** -7)


def _kgroups(config):
    return C.tile(config)[2] // 64


def _model_case(config, kind="odd"):
    M, N, Kk = C.shape(config, kind)
    return M, N, Kk, C.integer_probe(M, N, Kk)


@pytest.mark.parametrize("splitk", [1, 3])
@pytest.mark.parametrize("config", MODEL_CONFIGS)
def test_honest_model_passes_every_check(config, splitk):
    M, N, Kk = C.shape(config, "seg")
    kw = dict(tile=C.tile(config), kgroups=_kgroups(config), splitk=splitk)
    for kind in C.PROBES:
        p = C.probe(kind, M, N, Kk)
        for epi in (C.EPI_NONE, C.EPI_FULL):
            bias, res, act, alpha = C.operands(p, epi)
            y = K.honest_model(p.x, p.w, bias, act, res, alpha, **kw)
            K.check_exact(y, K.expected_exact(p, epi), f"model {kind} {epi.name}")
    p = C.integer_probe(M, N, Kk)
    bias, res, act, alpha = C.operands(p, C.EPI_FULL)
    pd = C.padded(p.x, p.w, res)
    K.check_poison_placement(pd, M, N, Kk)
    K.honest_model(pd.a, pd.w, bias, act, pd.res, alpha, out=pd.out, **kw)
    K.check_exact(pd.out.contiguous(), K.expected_exact(p, C.EPI_FULL), "model poisoned")
    K.check_canary(pd, M, N, res, "model poisoned")
    c = C.random_operands(M, N, Kk)
    pre, out = K.ref64(c["x"], c["w"], c["bias"], "relu", c["res"], 0.5)
    y = K.honest_model(c["x"], c["w"], c["bias"], "relu", c["res"], 0.5, **kw)
    assert K.check_bound(y, pre, out, K.absprod64(c["x"], c["w"]), Kk, "linear", "model random", C=2.0) <= 2.0


def _caught_by(mutant, config):
    """The checks that reject ``mutant`` on ``config``'s integer probe with the full epilogue."""
    M, N, Kk, p = _model_case(config)
    bias, res, act, alpha = C.operands(p, C.EPI_FULL)
    kw = dict(tile=C.tile(config), kgroups=_kgroups(config), splitk=2, mutant=mutant)
    want = K.expected_exact(p, C.EPI_FULL)
    caught = set()
    try:
        K.check_exact(K.honest_model(p.x, p.w, bias, act, res, alpha, **kw), want, mutant)
    except AssertionError:
        caught.add("exact")
    pd = C.padded(p.x, p.w, res)
    K.honest_model(pd.a, pd.w, bias, act, pd.res, alpha, out=pd.out, **kw)
    try:
        K.check_exact(pd.out.contiguous(), want, mutant)
    except AssertionError:
        caught.add("poison")
    try:
        K.check_canary(pd, M, N, res, mutant)
    except AssertionError:
        caught.add("canary")
    return caught


@pytest.mark.parametrize("config", [24, 17, 45])
@pytest.mark.parametrize("mutant", sorted(K.MUTANTS))
def test_mutant_is_caught(mutant, config):
    caught = _caught_by(mutant, config)
    print(f"{mutant}: caught by {sorted(caught)}")
    assert K.MUTANTS[mutant] in caught, f"{mutant} passes the {K.MUTANTS[mutant]} check (caught by {sorted(caught)})"
    if K.MUTANTS[mutant] != "exact":
        assert "exact" not in caught  # visible only through the padded operands / the canary


def test_one_ulp_is_caught_by_every_exact_probe():
    M, N, Kk = C.shape(24, "odd")
    for kind in C.PROBES:
        p = C.probe(kind, M, N, Kk)
        bias, res, act, alpha = C.operands(p, C.EPI_NONE)
        y = K.honest_model(p.x, p.w, bias, act, res, alpha, tile=C.tile(24), mutant="one_ulp")
        with pytest.raises(AssertionError, match="1 of"):
            K.check_exact(y, K.expected_exact(p, C.EPI_NONE), kind)


def test_bound_catches_one_dropped_k_element_that_the_global_metric_passes():
    """(77, 130, 200), the last K element missing from one output row: the error stays inside
    2e-2 * max|ref|, the metric of the older tests, and outside the per-element bound."""
    M, N, Kk = 77, 130, 200
    c = C.random_operands(M, N, Kk)
    x, w = c["x"], c["w"]
    pre, out = K.ref64(x, w)
    ap = K.absprod64(x, w)
    good = out.to(BF)
    row = int((x[:, Kk - 1].float().abs() - 0.5).abs().argmin())  # a row whose last element is about 0.5
    xm = x.clone()
    xm[row, Kk - 1] = 0
    bad = K.ref64(xm, w)[1].to(BF)
    err = (bad.double() - out).abs().max().item()
    print(f"dropped element: max err {err:.4g}, global allowance {2e-2 * out.abs().max().item():.4g}")
    assert K.close_global(good, out.float()) and K.close_global(bad, out.float()), "the global metric passes both"
    assert K.check_bound(good, pre, out, ap, Kk, "linear", "honest", C=1.0) <= 1.0
    with pytest.raises(AssertionError, match="derived bound"):
        K.check_bound(bad, pre, out, ap, Kk, "linear", "one K element dropped", C=4.0)


def test_bound_constants():
    """C is 1.5 x the measured ratio rounded up to a power of two, and never above 4."""
    assert K.C_BOUND == {"linear": 4.0, "gelu": 4.0, "silu": 2.0, "swiglu": 2.0, "rope": 4.0, "layernorm": 2.0,
                         "rmsnorm": 2.0, "postnorm": 2.0}
    for fam, m in K.MEASURED.items():
        assert 1.5 * m <= K.C_BOUND[fam] < 3.0 * m
