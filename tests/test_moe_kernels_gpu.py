"""Every MoE routing, pack and combine kernel (csrc/kernels/moe.hip) against the independent
reference (moe_ref.py) — never against another kernel. Integers and moved rows are compared bit
for bit, gates with the float64 softmax to moe_checks.GATE_TOL, combine elementwise with a
derived bound. The cases (moe_cases.py) are the ones test_moe_ref_cpu.py runs through the CPU
paths: exact ties across the k-th boundary, constant rows, skewed routings with empty experts,
sizes around the 1024-thread chunk and the fused kernel's 16384-assignment limit, -inf masks
and +-60 logits. Rows of all -inf logits and NaN logits are outside the routing contract.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import moe_cases as C  # noqa: E402
import moe_checks as K  # noqa: E402
import moe_ref as R  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _over_limit(logits, k):
    return logits.shape[0] * k > C.ROUTE_MAX_ASSIGN


@pytest.mark.parametrize("name", list(C.ROUTE_CASES))
def test_router_then_align(name):
    """router_kernel, then align_kernel on its output (the c0 loop needs more than 1024 assignments)."""
    logits, k, ref = C.route_case(name)
    ld = logits.to(DEV)
    idx, w = ops.moe_router(ld, k)
    src, slot, off = ops.moe_align(idx, logits.shape[1])
    torch.cuda.synchronize()
    K.check_routing(logits, k, (idx, w, src, slot, off), ref, K.GATE_TOL, f"router+align {name}")
    assert torch.equal(ld.cpu(), logits)


@pytest.mark.parametrize("name", list(C.ROUTE_CASES))
def test_route_fused_kernel(name):
    """route_kernel (one workgroup) up to its limit; one assignment pair past it, it refuses."""
    logits, k, ref = C.route_case(name)
    if _over_limit(logits, k):
        with pytest.raises(RuntimeError, match="at most"):
            ops.ext().moe_route(logits.to(DEV), k)
        return
    got = ops.ext().moe_route(logits.to(DEV), k)
    torch.cuda.synchronize()
    K.check_routing(logits, k, got, ref, K.GATE_TOL, f"ext.moe_route {name}")


@pytest.mark.parametrize("name", list(C.ROUTE_CASES))
def test_route_entry_point(name):
    """ops.moe_route: the fused kernel, or past its limit the router + align pair."""
    logits, k, ref = C.route_case(name)
    got = ops.moe_route(logits.to(DEV), k, logits.shape[1])
    torch.cuda.synchronize()
    K.check_routing(logits, k, got, ref, K.GATE_TOL, f"ops.moe_route {name}")


# (M, E, k, H, fused): the one-launch kernel takes E even, E <= 16, H <= 4096
GATE_ROUTE_SHAPES = [(77, 8, 2, 128, True), (300, 16, 4, 4096, True), (1, 2, 1, 64, True),
                     (40, 6, 2, 4104, False), (40, 5, 2, 128, False), (40, 64, 2, 128, False)]


@pytest.mark.parametrize("M,E,k,H,fused", GATE_ROUTE_SHAPES)
def test_gate_route(M, E, k, H, fused):
    """Router GEMM + routing: the routing equals the reference applied to the bf16 logits the
    launch published. Repeated router-weight rows make every token tie (experts 1 == 5 and
    0 == 3; 0 == 1 for E = 2): identical rows give the same dot product in the same order."""
    g = torch.Generator().manual_seed(M + E + H)
    x = torch.randn(M, H, generator=g).to(torch.bfloat16).to(DEV)
    wg = (0.05 * torch.randn(E, H, generator=g)).to(torch.bfloat16)
    twins = [(1, 0)] if E == 2 else [(3, 0)] + ([(5, 1)] if E > 5 else [])
    for a, b in twins:
        wg[a] = wg[b]
    wg = wg.to(DEV)
    logits = torch.full((M, E), float("nan"), dtype=torch.bfloat16, device=DEV)
    for _ in range(3):  # repeated launches: every last workgroup must reset the ticket
        got = ops.moe_gate_route(x, wg, k, logits)
    torch.cuda.synchronize()
    took_fused = len(ops.ext().moe_gate_route(x, wg, k, torch.empty_like(logits))) > 0
    torch.cuda.synchronize()
    assert took_fused == fused
    pub = logits.cpu()
    want = ops.ref_linear(x.cpu(), wg.cpu()).float()
    err = (pub.float() - want).abs().max().item()
    assert err <= 2e-2 * (want.abs().max().item() + 1e-6), f"logits: max abs err {err:.4g}"
    if fused:
        for a, b in twins:
            assert torch.equal(pub[:, a], pub[:, b]), "identical router rows gave different logits"
    idx, gate = R.route_ref(pub, k)
    K.check_routing(pub, k, got, (idx, gate) + R.align_ref(idx, E), K.GATE_TOL, f"gate_route {M}x{E}k{k}H{H}")


@pytest.mark.parametrize("lname", K.PACK_LISTS)
@pytest.mark.parametrize("H", [64, 1032])
@pytest.mark.parametrize("kind", ["skewed", "random"])
def test_pack_unpack(kind, H, lname):
    K.check_pack_unpack(kind, H, lname, DEV)
    torch.cuda.synchronize()


def test_pack_refusals():
    x, src, off = K.pack_inputs("random", 64)
    xd, srcd, offd = x.to(DEV), src.to(DEV), off.to(DEV)
    ovf = torch.zeros(4, dtype=torch.int32, device=DEV)

    def buf(H=64):
        return torch.zeros(4, H, dtype=torch.bfloat16, device=DEV)

    one = (4, (0,), 0, [4], [-1])
    ops.moe_pack(xd, srcd, offd, [(buf(),) + one], ovf)  # the accepted form of what follows
    bad = {
        "H % 8": (xd[:, :60].contiguous(), [(buf(60),) + one]),
        "nine destinations": (xd, [(buf(),) + one] * 9),
        "nine experts": (xd, [(buf(), 4, (0,) * 9, 0, [4] * 9, [-1] * 9)]),
        "expert id >= E": (xd, [(buf(), 4, (C.PACK_E,), 0, [4], [-1])]),
        "flag >= ovf.numel()": (xd, [(buf(), 4, (0,), 4, [4], [-1])]),
        "expert flag >= ovf.numel()": (xd, [(buf(), 4, (0,), 0, [4], [4])]),
        "buffer below cap rows": (xd, [(buf(), 5, (0,), 0, [4], [-1])]),
    }
    for what, (xx, dests) in bad.items():
        with pytest.raises(RuntimeError):
            ops.moe_pack(xx, srcd, offd, dests, ovf)
            pytest.fail(f"moe_pack accepted: {what}")
    torch.cuda.synchronize()
    assert ovf.cpu().tolist() == [1, 0, 0, 0]  # the accepted launch alone wrote (expert 0 has more than 4 rows)


@pytest.mark.parametrize("M,k,H", C.COMBINE_SHAPES)
def test_combine(M, k, H):
    K.check_combine(M, k, H, DEV)


@pytest.mark.parametrize("rows,H", C.PERMUTE_SHAPES)
def test_permute(rows, H):
    K.check_permute(rows, H, DEV)


@pytest.mark.parametrize("name", C.XBATCH_CASES)
def test_xbatch_index(name):
    rest = K.check_xbatch(name, DEV)
    assert rest.numel() == C.XBATCH_SLACK and (rest == C.XBATCH_CANARY).all(), "a_rows written past offsets[G]"
