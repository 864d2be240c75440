"""The skinny grouped GEMM kernel (csrc/kernels/gemm_grouped_skinny.hip) over the cases of
moe_skinny_cases.py: per-element bound against the float64 reference, exact probes, NaN poison in
unowned rows and outputs, canaries, two launches bit-identical, and a captured launch replayed
after the routing was rewritten on the device."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import moe_skinny_cases as S  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("case", S.CASES, ids=S.case_id)
def test_bounded(case):
    S.run_case(ops.gemm_grouped_skinny, case, DEV)


@pytest.mark.parametrize("case", S.EXACT_CASES, ids=S.case_id)
def test_exact(case):
    S.run_case(ops.gemm_grouped_skinny, case, DEV, exact=True)


def test_refused_shapes():
    x = torch.zeros(4, 48, dtype=torch.bfloat16, device=DEV)
    off = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.gemm_grouped_skinny(x, [torch.zeros(16, 48, dtype=torch.bfloat16, device=DEV)], off,
                                out=torch.zeros(4, 16, dtype=torch.bfloat16, device=DEV))


@pytest.mark.parametrize("act,nk", [("none", (48, 96)), ("swiglu", (512, 256))])
@pytest.mark.parametrize("mode", ["out", "outs"])
def test_graph_replay_follows_device_routing(act, nk, mode):
    """One launch captured with the routing of one case, replayed after offsets and a_rows were
    overwritten on the device with another's: the grid depends on (groups, N) only."""
    first = S.build(act, nk, (16, 16, 16, 16))
    second = S.build(act, nk, (1, 0, 16, 7))
    run = S.make_run(first, True, mode, DEV)
    w = S.weights_on(first, DEV)
    w_ptrs = torch.tensor([t.data_ptr() for t in w], dtype=torch.int64, device=DEV)
    out_ptrs = None if run.outs is None else torch.tensor([o.data_ptr() for o in run.outs], dtype=torch.int64, device=DEV)
    kw = dict(act=None if act == "none" else act, out=run.out, outs=run.outs, w_ptrs=w_ptrs, out_ptrs=out_ptrs,
              a_rows=run.a_rows)
    ops.gemm_grouped_skinny(run.x, w, run.offsets, **kw)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.gemm_grouped_skinny(run.x, w, run.offsets, **kw)
    g.replay()
    torch.cuda.synchronize()
    S.verify(first, run, "captured, first routing")
    # the second routing over the same weights: rebuild its rows, a_rows and offsets in place
    second = second._replace(weights=first.weights)
    refs, pres, aps = [], [], []
    import gemm_checks as gk
    r = 0
    for e, n in enumerate(second.counts):
        x = second.rows[r:r + n]
        r += n
        if act == "swiglu":
            ref, ap = gk.ref64_swiglu(x, first.weights[e])
            pre = ref
        else:
            pre, ref = gk.ref64(x, first.weights[e])
            ap = gk.absprod64(x, first.weights[e])
        refs.append(ref), pres.append(pre), aps.append(ap)
    second = second._replace(refs=tuple(refs), pres=tuple(pres), aps=tuple(aps))
    R2 = sum(second.counts)
    assert R2 <= run.a_rows.numel() and R2 <= run.x.shape[0]
    run.x.fill_(float("nan"))
    run.x[:R2] = second.rows.to(DEV)
    run.a_rows.fill_(run.x.shape[0] - 1)  # a NaN row: sorted rows past the new total belong to no group
    run.a_rows[:R2] = torch.arange(R2, dtype=torch.int32, device=DEV)
    offs = [0]
    for n in second.counts:
        offs.append(offs[-1] + n)
    run.offsets.copy_(torch.tensor(offs, dtype=torch.int32, device=DEV))
    (run.out if run.outs is None else run.obuf).fill_(float("nan") if run.outs is None else S.gc.CANARY)
    if run.outs is not None:
        for o in run.outs:
            o.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    # the whole check of a launch: bounds, NaN where nobody owns a row, every canary row and column
    S.verify(second, run, "replay, second routing")
