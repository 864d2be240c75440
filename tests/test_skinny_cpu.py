"""``ops.linear_skinny`` on the CPU back end over the cases of skinny_cases.py, its refusals, the
wave rule, and the ORACLE SELF-CHECK: a torch model of the kernel passes the checks the GPU kernel
is held to and seven models of subtly wrong kernels fail them."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as gc  # noqa: E402
import skinny_cases as S  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

BF = torch.bfloat16
ONE_W = (8,)  # the CPU path has no waves: one value, to keep the file quick


@pytest.mark.parametrize("case", S.PLAIN_CASES, ids=S.case_id)
def test_plain(case):
    S.run_plain(ops.linear_skinny, "cpu", case, waves=ONE_W)


@pytest.mark.parametrize("case", S.SWIGLU_CASES, ids=S.case_id)
def test_swiglu(case):
    S.run_swiglu(ops.linear_skinny, "cpu", case, waves=ONE_W)


@pytest.mark.parametrize("case", S.ROPE_CASES, ids=S.case_id)
def test_rope(case):
    S.run_rope(ops.linear_skinny, "cpu", case, waves=ONE_W)


@pytest.mark.parametrize("case", S.FOLDED_CASES, ids=S.case_id)
def test_folded_norm(case):
    S.run_folded(ops.linear_skinny, "cpu", case, waves=ONE_W)


@pytest.mark.parametrize("case", S.EXACT_CASES, ids=S.case_id)
def test_exact(case):
    S.run_exact(ops.linear_skinny, "cpu", case, waves=ONE_W)


def test_onehot():
    S.run_onehot(ops.linear_skinny, "cpu", waves=ONE_W)


def test_refusals():
    x = torch.zeros(2, 64, dtype=BF)
    w = torch.zeros(32, 64, dtype=BF)
    assert ops.linear_skinny(x, w).shape == (2, 32)
    assert ops.linear_skinny(x, w, act="swiglu").shape == (2, 16)
    bad = [
        dict(x=torch.zeros(17, 64, dtype=BF)),  # M = 17
        dict(x=torch.zeros(2, 48, dtype=BF), w=torch.zeros(32, 48, dtype=BF)),  # K = 48
        dict(w=torch.zeros(48, 64, dtype=BF), act="swiglu"),  # SwiGLU N = 48
        dict(stats_out=torch.zeros(2, 2)),
        dict(ext_stats=torch.zeros(2, 2)),
        dict(rows=torch.zeros(2, dtype=torch.int32)),
        dict(compact=True),
        dict(post_norm=(x, x, x, "rmsnorm", 1e-5)),
        dict(x=x.float()),
        dict(w=w.float()),
        dict(x=torch.zeros(2, 68, dtype=BF)[:, :64]),  # row stride 68
        dict(w=torch.zeros(32, 72, dtype=BF)[:, 4:68]),  # rows not 16-byte aligned
        dict(waves=2),
        dict(act="tanh"),
        dict(rope=(torch.zeros(1, 3), torch.zeros(1, 3), 1, 6, 6)),  # D % 4
        dict(rope=(torch.zeros(1, 8), torch.zeros(1, 8), 1, 16, 32), act="gelu"),
        dict(norm=(torch.zeros(32), "batchnorm", 1e-5)),
        dict(norm=(torch.zeros(31), "rmsnorm", 1e-5)),
        dict(bias=torch.zeros(31, dtype=BF)),
        dict(residual=torch.zeros(2, 16, dtype=BF)),
        dict(out=torch.zeros(2, 16, dtype=BF)),
    ]
    for kw in bad:
        args = dict(x=x, w=w)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.linear_skinny(**args)
    with pytest.raises(TypeError):
        ops.linear_skinny(x, w, colour="red")
    assert ops.skinny_ok(1, 50257, 768) and ops.skinny_ok(16, 28672, 4096, "swiglu")
    assert not ops.skinny_ok(17, 768, 768) and not ops.skinny_ok(1, 768, 48) and not ops.skinny_ok(1, 48, 64, "swiglu")
    assert 1 <= ops.SKINNY_MAX_ROWS <= ops.SKINNY_ROWS_LIMIT == 16 and isinstance(ops.SKINNY_LMHEAD, bool)


def test_waves_rule():
    for act in (None, "gelu", "swiglu"):
        for N in (32, 768, 2304, 4096, 6144, 28672, 50272, 128256):
            for K in (32, 96, 768, 3072, 4096, 14336):
                W = ops.skinny_waves(N, K, act)
                assert W in S.WAVES
                assert W < 16 or -(-K // 64) >= 2 * W  # sixteen waves only where each keeps two slices
    # the measured choices (profiles/skinny_gemm/waves_rule.txt)
    assert ops.skinny_waves(28672, 4096, "swiglu") == 4 and ops.skinny_waves(768, 3072) == 8
    assert ops.skinny_waves(128256, 4096) == 16 and ops.skinny_waves(50257, 768) == 8


# ---- oracle self-check -----------------------------------------------------------------------

def test_model_passes():
    """The honest model — per-wave partial sums in the kernel's order — passes everything."""
    fn = S.model()
    S.run_plain(fn, "cpu", (5, 272, 1056))
    S.run_plain(fn, "cpu", (16, 50, 64))
    S.run_swiglu(fn, "cpu", (5, 96, 160))
    S.run_rope(fn, "cpu", (5, 4))
    S.run_folded(fn, "cpu", ("layernorm", "gelu", 5, 80, 1056))
    S.run_folded(fn, "cpu", ("rmsnorm", "swiglu", 5, 96, 96))
    S.run_exact(fn, "cpu", ("integer", 16, 272, 1056))
    S.run_exact(fn, "cpu", ("selector", 16, 50, 64))
    S.run_onehot(fn, "cpu")


MUTANT_RUNS = {
    "first_wave_only": [lambda f: S.run_exact(f, "cpu", ("integer", 16, 272, 1056)), lambda f: S.run_onehot(f, "cpu"),
                        lambda f: S.run_plain(f, "cpu", (1, 64, 4160))],
    "last_slice_dropped": [lambda f: S.run_exact(f, "cpu", ("integer", 5, 48, 96)), lambda f: S.run_onehot(f, "cpu"),
                           lambda f: S.run_plain(f, "cpu", (2, 16, 32))],
    "ragged_row_n": [lambda f: S.run_plain(f, "cpu", (2, 50, 64)), lambda f: S.run_exact(f, "cpu", ("scaled", 2, 1041, 256))],
    "gate_up_off_by_one": [lambda f: S.run_swiglu(f, "cpu", (5, 96, 160)), lambda f: S.run_swiglu(f, "cpu", (1, 512, 256))],
    # (position 0 rotates by nothing: S = 1 cannot see the partner, rows at positions >= 1 do)
    "rope_partner_next_lane": [lambda f: S.run_rope(f, "cpu", (2, 4)), lambda f: S.run_rope(f, "cpu", (5, 4))],
    "ln_mean_skipped": [lambda f: S.run_folded(f, "cpu", ("layernorm", "gelu", 2, 80, 96))],
    "residual_before_act": [lambda f: S.run_exact(f, "cpu", ("integer", 16, 50, 64)),
                            lambda f: S.run_plain(f, "cpu", (5, 48, 96), epis=S.EPIS[3:4])],
}


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_oracle_rejects(mutant):
    assert MUTANT_RUNS[mutant]
    for run in MUTANT_RUNS[mutant]:
        with pytest.raises(AssertionError):
            run(S.model(mutant))
