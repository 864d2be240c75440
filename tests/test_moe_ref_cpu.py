"""The CPU paths of the MoE routing, pack and combine ops against the independent reference
(moe_ref.py): integers exactly, gates to 1e-6 absolute. The CPU paths are the routing of every
gloo rank and of the CPU harness and the comparison side of older GPU tests, so they must obey
the kernels' rules — first of all "ties go to the lower expert index" (csrc/kernels/moe.hip,
select_topk). Rows of all -inf logits and NaN logits are outside the routing contract.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import moe_cases as C  # noqa: E402
import moe_checks as K  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

GATE_TOL_CPU = 1e-6  # fp32 softmax of at most eight terms against float64


@pytest.mark.parametrize("name", list(C.ROUTE_CASES))
def test_route_case_is_what_it_claims(name):
    C.check_case_shape(name)


@pytest.mark.parametrize("name", list(C.ROUTE_CASES))
def test_router_align_cpu(name):
    logits, k, ref = C.route_case(name)
    E = logits.shape[1]
    idx, gate = ops.moe_router(logits, k)
    K.check_routing(logits, k, (idx, gate) + tuple(ops.moe_align(idx, E)), ref, GATE_TOL_CPU, f"router+align {name}")
    for g, r in zip(ops.moe_align(ref[0], E), ref[2:]):  # moe_align on its own, fed the reference's idx
        assert g.dtype == torch.int32 and torch.equal(g, r)


@pytest.mark.parametrize("name", list(C.ROUTE_CASES))
def test_route_cpu(name):
    logits, k, ref = C.route_case(name)
    K.check_routing(logits, k, ops.moe_route(logits, k, logits.shape[1]), ref, GATE_TOL_CPU, f"moe_route {name}")


def test_router_unchanged_on_tie_free_input():
    """Without ties the stable sort selects what torch.topk selects: same idx, same gate bits."""
    logits, k, _ref = C.route_case("tie_free_300x8k2")
    idx, gate = ops.moe_router(logits, k)
    val, tidx = torch.topk(logits.float(), k, dim=-1)
    assert torch.equal(idx, tidx.to(torch.int32)) and torch.equal(gate, torch.softmax(val, dim=-1))


@pytest.mark.parametrize("lname", K.PACK_LISTS)
@pytest.mark.parametrize("H", [64, 1032])
@pytest.mark.parametrize("kind", ["skewed", "random"])
def test_pack_unpack_cpu(kind, H, lname):
    K.check_pack_unpack(kind, H, lname, "cpu")


@pytest.mark.parametrize("M,k,H", C.COMBINE_SHAPES)
def test_combine_cpu(M, k, H):
    K.check_combine(M, k, H, "cpu")


@pytest.mark.parametrize("rows,H", C.PERMUTE_SHAPES)
def test_permute_cpu(rows, H):
    K.check_permute(rows, H, "cpu")


@pytest.mark.parametrize("name", C.XBATCH_CASES)
def test_xbatch_index_cpu(name):
    K.check_xbatch(name, "cpu")
    offs, reqs, experts, _bases = C.xbatch_case(name)
    counts = [int(offs[q][e + 1] - offs[q][e]) for q, e in zip(reqs, experts)]
    if name == "maxima_q16_g64":
        assert len(offs) == ops.XBATCH_MAX_REQ and len(reqs) == ops.XBATCH_MAX_GROUPS
    elif name == "empty_experts":
        assert counts.count(0) >= 4 and counts[0] == 0 and counts[-1] > 0
    elif name == "group_over_256_rows":
        assert max(counts) > 512 and 256 < counts[1] < 512
