"""Every launch variant of flash attention (csrc/kernels/attention.hip, attention_impl.h) against
the independent float64 reference (attn_checks.ref64) — per (row, head), to attn_checks.ROW_TOL —
and against exact expectations: selector cases whose output is one value row bit for bit, and
poisoned keys that replace a row if they leak through a mask. The cases (attn_cases.py) wrap
the deep K/V rings (S = 600 at D = 64, S = 400 at D = 128), are ragged for 64, 128 and 256 keys
per stage, put a batch boundary inside a query block, and run query chunks causal and not, at odd
offsets, with keys past the chunk. test_attn_ref_cpu.py shows that these checks reject mutants.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_cases as C  # noqa: E402
import attn_checks as K  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _to_dev(*tensors):
    """Device copies that keep the layout: the buffer a view looks into moves whole (once, when
    several views share it), and the view is taken again — so a packed buffer stays packed and
    the rows past a row view stay behind it."""
    moved, out = {}, []
    for t in tensors:
        base = t._base if t._base is not None else t
        assert base.is_contiguous() and base.storage_offset() == 0
        if base.data_ptr() not in moved:
            moved[base.data_ptr()] = base.to(DEV)
        out.append(moved[base.data_ptr()].as_strided(t.size(), t.stride(), t.storage_offset()))
    return out


def _launch(case, variant, qkv=None, out=None, flags=0):
    q, k, v = _to_dev(case.q, case.k, case.v) if qkv is None else qkv
    B, S, nh, nkv, D, causal, Sq, q_off = case.shape
    return ops.ext().attention(q, k, v, B, S, nh, nkv, D, causal, 1.0 / D ** 0.5, out, variant,
                               Sq if case.chunk else 0, q_off, flags)


@pytest.mark.parametrize("name,variant", C.case_variants(C.RANDOM_CASES))
def test_random(name, variant):
    c = C.case(name)
    o = _launch(c, variant)
    K.check_rows(o, K.reference(c), K.ROW_TOL, f"{name} variant {variant}", q_off=c.q_off)


@pytest.mark.parametrize("name,variant", C.case_variants(C.SELECTOR_CASES))
def test_selector(name, variant):
    """The output is the selected key's value row, bit for bit: the winning p is exp2 of a
    rounding residue near 1e-5 and rounds to bf16 1.0, every other p is below e^-56, and o / l
    perturbs v by about 1e-5 relative, far inside half a bf16 ulp."""
    c = C.case(name)
    o = _launch(c, variant)
    K.check_exact(o, c.want, f"{name} variant {variant}", c.Sq, c.q_off)


@pytest.mark.parametrize("name,variant", C.case_variants(C.POISON_CASES))
def test_poison(name, variant):
    c = C.case(name)
    o = _launch(c, variant)
    K.check_rows(o, K.reference(c), K.ROW_TOL, f"{name} variant {variant}", rows=c.rows, q_off=c.q_off)


GUARD_LAUNCHES = [(v, 0) for v in C.ALL_VARIANTS] + [(0, 1), (0, 2), (0, 3)]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("variant,flags", GUARD_LAUNCHES)
def test_strided_out_with_guards(D, variant, flags):
    """``out`` is a view into a wider and taller sentinel-filled buffer (ldo = nh * D + 64): the
    rows are right and nothing outside the view is written — neither by the padded query rows
    of a block (Sq = 50) nor by a store that takes the row stride for nh * D. flags 1: buffer
    stores with their own offset arithmetic; 2: XCD-grouped block order."""
    c = C.guard_case(D)
    rows, cols = c.B * c.Sq, c.nh * D
    buf = torch.full((rows + 2 * C.GUARD_ROWS, cols + 2 * C.GUARD_COLS), C.OUT_SENTINEL, dtype=torch.bfloat16,
                     device=DEV)
    view = buf[C.GUARD_ROWS:C.GUARD_ROWS + rows, C.GUARD_COLS:C.GUARD_COLS + cols]
    o = _launch(c, variant, out=view, flags=flags)
    assert o.data_ptr() == view.data_ptr() and o.stride() == view.stride()
    K.check_rows(view, K.reference(c), K.ROW_TOL, f"{c.name} variant {variant} flags {flags}", q_off=c.q_off)
    guard = buf.cpu()
    assert (guard[C.GUARD_ROWS:C.GUARD_ROWS + rows, C.GUARD_COLS:C.GUARD_COLS + cols] != C.OUT_SENTINEL).all()
    guard[C.GUARD_ROWS:C.GUARD_ROWS + rows, C.GUARD_COLS:C.GUARD_COLS + cols] = C.OUT_SENTINEL
    assert (guard == C.OUT_SENTINEL).all(), \
        f"written outside the output view at (row, column) {(guard != C.OUT_SENTINEL).nonzero()[:4].tolist()}"


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("kind", C.TWICE_KINDS)
def test_split_variant_twice(kind, D):
    """Variant 14 merges a query tile's key chunks by tickets in global memory that the last
    arriver resets. Two launches back to back, different inputs of one shape: both are right."""
    a, b = C.twice_cases(kind, D)
    qa, qb = _to_dev(a.q, a.k, a.v), _to_dev(b.q, b.k, b.v)
    oa = _launch(a, 14, qkv=qa)
    ob = _launch(b, 14, qkv=qb)
    K.check_rows(oa, K.reference(a), K.ROW_TOL, a.name, q_off=a.q_off)
    K.check_rows(ob, K.reference(b), K.ROW_TOL, b.name, q_off=b.q_off)
    assert not torch.equal(oa, ob)


TICKET_POOL, TICKET_GRAIN = 1 << 20, 64  # ops_binding.cpp: split_k_counters' pool and its granule


@pytest.mark.parametrize("D", [64, 128])
def test_split_variant_tickets_after_pool_wrap(D):
    """The binding hands ticket regions out round-robin from a pool zeroed once, so a launch
    meets tickets an earlier launch drew only after the pool has wrapped. One lap of launches of
    one small shape (one 64-counter granule each), then the launch that lands on the first one's
    region: a ticket the last arriver did not reset leaves its query tile unmerged."""
    a, b = C.twice_cases("wrap", D)
    assert a.B * a.nh * -(-a.S // 32) <= TICKET_GRAIN
    qa, qb = _to_dev(a.q, a.k, a.v), _to_dev(b.q, b.k, b.v)
    first = _launch(a, 14, qkv=qa)
    out = torch.empty_like(first)
    for _ in range(TICKET_POOL // TICKET_GRAIN - 1):
        _launch(a, 14, qkv=qa, out=out)
    ob = _launch(b, 14, qkv=qb)
    K.check_rows(first, K.reference(a), K.ROW_TOL, a.name)
    K.check_rows(out, K.reference(a), K.ROW_TOL, a.name + " (last of the lap)")
    K.check_rows(ob, K.reference(b), K.ROW_TOL, b.name + " (on reused tickets)")
