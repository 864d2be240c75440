"""``ops.gemm_grouped_skinny`` on the CPU back end over the cases of moe_skinny_cases.py, its
argument checks, and the ORACLE SELF-CHECK: two stand-ins for subtly wrong kernels must be
rejected by the very checks the GPU kernel is held to (these two tests show the checks bite; they
do not exercise new project code beyond the op's CPU path)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import moe_skinny_cases as S  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

BF = torch.bfloat16


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_bounded(case):
    S.run_case(ops.gemm_grouped_skinny, case, "cpu")


@pytest.mark.parametrize("case", S.EXACT_CASES, ids=S.case_id)
def test_exact(case):
    S.run_case(ops.gemm_grouped_skinny, case, "cpu", exact=True)


def test_argument_checks():
    x = torch.zeros(4, 64, dtype=BF)
    w = [torch.zeros(32, 64, dtype=BF)] * 2
    off = torch.tensor([0, 2, 4], dtype=torch.int32)
    out = torch.zeros(4, 32, dtype=BF)
    ops.gemm_grouped_skinny(x, w, off, out=out)
    bad = [
        dict(x=torch.zeros(4, 48, dtype=BF), weights=[torch.zeros(32, 48, dtype=BF)] * 2, out=out),  # K % 32
        dict(weights=[torch.zeros(24, 64, dtype=BF)] * 2, out=torch.zeros(4, 24, dtype=BF)),  # N % 16
        dict(weights=[torch.zeros(48, 64, dtype=BF)] * 2, act="swiglu", out=torch.zeros(4, 24, dtype=BF)),  # N % 32
        dict(act="gelu", out=out),
        dict(out=None),
        dict(out=out, outs=[out, out]),
        dict(out=torch.zeros(4, 16, dtype=BF)),
        dict(x=x.float(), out=out),
        dict(offsets=off.long(), out=out),
        dict(offsets=off[:2], out=out),
        dict(a_rows=torch.zeros(4, dtype=torch.int64), out=out),
        dict(weights=[w[0], torch.zeros(16, 64, dtype=BF)], out=out),
        dict(x=torch.zeros(4, 128, dtype=BF)[:, ::2], out=out),  # rows not contiguous
        dict(x=torch.zeros(4, 68, dtype=BF)[:, :64], out=out),  # row stride 68: rows not 16-byte aligned
        dict(weights=[torch.zeros(32, 128, dtype=BF)[:, :64]] * 2, out=out),  # weights not contiguous
    ]
    for kw in bad:
        args = dict(x=x, weights=w, offsets=off)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.gemm_grouped_skinny(**args)
    assert 1 <= ops.MOE_SKINNY_MAX_ROWS <= 16  # (a kernel pass is 16 rows)
    assert ops.grouped_skinny_ok(28672, 4096, "swiglu") and ops.grouped_skinny_ok(4096, 14336)
    assert not ops.grouped_skinny_ok(4096, 14336 + 16) and not ops.grouped_skinny_ok(48, 64, "swiglu")


# ---- oracle self-check -----------------------------------------------------------------------

def test_oracle_rejects_first_wave_only():
    """A kernel whose finish takes wave 0's fragment alone: caught by the exact probe and by the
    bound wherever K spans more than one wave's run."""
    with pytest.raises(AssertionError):
        S.run_case(S.mutant("first_wave_only"), ("none", (256, 256), (1, 0, 16, 7)), "cpu", exact=True)
    for case in (("none", (256, 14336), (1, 0, 16, 7)), ("swiglu", (512, 4096), (16, 16, 16, 16)),
                 ("swiglu", (96, 160), (0, 0, 0, 2))):
        with pytest.raises(AssertionError):
            S.run_case(S.mutant("first_wave_only"), case, "cpu")


def test_oracle_rejects_gate_up_off_by_one():
    for case in (("swiglu", (96, 160), (1, 0, 16, 7)), ("swiglu", (512, 4096), (0,) * 7 + (1,))):
        with pytest.raises(AssertionError):
            S.run_case(S.mutant("gate_up_off_by_one"), case, "cpu")
