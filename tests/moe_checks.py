"""Assertions shared by the CPU and GPU tests of the MoE ops (test_moe_ref_cpu.py,
test_moe_kernels_gpu.py): each runs an ``ops`` entry point on a device and compares it with
the independent reference (moe_ref.py) on the shared cases (moe_cases.py)."""
import torch

import moe_cases as C
import moe_ref as R
from distributed_llm_scheduler_amd import ops

# Absolute tolerance of a GPU gate against the float64 softmax. select_topk uses the fast __expf,
# whose error has no bound to derive from, so it is measured: the largest deviation over every
# routing case of moe_cases.ROUTE_CASES through all three paths on an MI355X is 7.725e-08
# (past_limit_8193x8k2); four times that is 3.09e-07, rounded up to a power of two: 2^-21 =
# 4.77e-07. (moe_gate_route's cases, held to the same constant, reach 1.397e-07.) Whatever is
# measured, the tolerance may not exceed 2^-16: the gates multiply bf16 rows of precision 2^-9.
GATE_TOL = 2.0 ** -21
assert GATE_TOL <= 2.0 ** -16
ROUTE_FIELDS =("idx", "gate", "src_rows", "slot_of", "offsets")
gate_deviation = {}  # "what case" -> largest |gate - reference| seen (reported by the GPU tests)


def check_routing(logits, k, got, ref, gate_tol, what):
    """got = (idx, gate, src_rows, slot_of, offsets) on any device against the reference's."""
    got = [t.cpu() for t in got]
    for g, r, field in zip(got, ref, ROUTE_FIELDS):
        if field == "gate":
            assert g.dtype == torch.float32 and g.shape == r.shape, f"{what}: gate shape / dtype"
            assert torch.isfinite(g).all(), f"{what}: a gate is not finite"
            dev = (g.double() - r).abs().max().item()
            gate_deviation[what] = max(dev, gate_deviation.get(what, 0.0))
            print(f"gate deviation {what}: {dev:.4g}")
            assert dev <= gate_tol, f"{what}: gate deviates from the float64 reference by {dev:.3g} > {gate_tol:.3g}"
            srow = (g.double().sum(-1) - 1).abs().max().item()
            assert srow <= k * gate_tol, f"{what}: gates of a row sum to 1 +- {srow:.3g}"
        else:
            assert g.dtype == torch.int32 and g.numel() == r.numel(), f"{what}: {field} shape / dtype"
            g = g.reshape(r.shape)
            if not torch.equal(g, r):
                first = int((g != r).reshape(-1).nonzero()[0])
                raise AssertionError(f"{what}: {field} differs from the reference in {int((g != r).sum())} of "
                                     f"{r.numel()} entries, first at flat index {first}: "
                                     f"{g.reshape(-1)[first].item()} != {r.reshape(-1)[first].item()}")
    picked = logits.cpu().float().gather(1, got[0].long())
    assert (picked[:, 1:] <= picked[:, :-1]).all(), f"{what}: idx is not in descending-logit order"


BUF_CANARY, X_CANARY = -77.0, 99.0  # no random row holds them
BUF_SLACK = 3  # buffer rows past cap


def pack_inputs(kind, H):
    src, off = C.pack_routing(kind)
    x = torch.randn(C.PACK_M, H, generator=torch.Generator().manual_seed(H)).to(torch.bfloat16)
    return x, src, off


def check_pack_unpack(kind, H, lname, dev):
    """Pack, then unpack, one destination list through ops.moe_pack on ``dev``; every output is
    compared bit for bit with the reference."""
    x, src, off = pack_inputs(kind, H)
    specs, preset = C.pack_dest_lists(kind)[lname]
    ovf0 = C.ovf_initial(specs, preset)
    n = (off[1:] - off[:-1]).tolist()

    def dests(bufs):
        return [(b,) + tuple(s) for b, s in zip(bufs, specs)]

    # ---- pack into canary-filled buffers
    bufs0 = [torch.full((cap + BUF_SLACK, H), BUF_CANARY, dtype=torch.bfloat16) for cap, *_ in specs]
    ref_bufs, ref_ovf = R.pack_ref(x, src, off, dests(bufs0), ovf0)
    xd, srcd, offd, ovfd = x.to(dev), src.to(dev), off.to(dev), ovf0.to(dev)
    bufsd = [b.to(dev) for b in bufs0]
    ops.moe_pack(xd, srcd, offd, dests(bufsd), ovfd)
    assert torch.equal(xd.cpu(), x) and torch.equal(srcd.cpu(), src) and torch.equal(offd.cpu(), off), \
        "pack wrote one of its inputs"
    assert torch.equal(ovfd.cpu(), ref_ovf), f"pack ovf {ovfd.cpu().tolist()} != {ref_ovf.tolist()}"
    for d, (b, rb, (cap, experts, *_)) in enumerate(zip(bufsd, ref_bufs, specs)):
        moved = min(sum(n[e] for e in experts), cap)
        assert (b.cpu()[moved:] == BUF_CANARY).all(), f"dest {d}: a row at or past min(total, cap) = {moved} was written"
        assert torch.equal(b.cpu(), rb), f"dest {d}: packed rows differ from the reference"
    # ---- unpack the packed buffers into canary-filled expert-sorted rows
    xs0 = torch.full((src.numel(), H), X_CANARY, dtype=torch.bfloat16)
    ref_xs, ref_ovf_u = R.unpack_ref(xs0, src, off, dests(ref_bufs), ovf0)
    xsd, ovfu = xs0.to(dev), ovf0.to(dev)
    bufsu = [b.to(dev) for b in ref_bufs]
    ops.moe_pack(xsd, srcd, offd, dests(bufsu), ovfu, unpack=True)
    assert torch.equal(ovfu.cpu(), ref_ovf_u), f"unpack ovf {ovfu.cpu().tolist()} != {ref_ovf_u.tolist()}"
    assert all(torch.equal(b.cpu(), rb) for b, rb in zip(bufsu, ref_bufs)), "unpack wrote a buffer"
    assert torch.equal(srcd.cpu(), src) and torch.equal(offd.cpu(), off)
    covered = sorted(j for cap, experts, *_ in specs for _c, j in R.pack_rows(off, experts, cap))
    rest = sorted(set(range(src.numel())) - set(covered))
    got = xsd.cpu()
    assert (got[rest] == X_CANARY).all(), "unpack wrote a row it does not cover"
    assert torch.equal(got[covered], x[src[covered].long()]), "pack + unpack does not reproduce x[src_rows[j]]"
    assert torch.equal(got, ref_xs)
    check_pack_flags(lname, ref_ovf, off, specs)


PACK_LISTS = ("one_expert_slack", "all8_cap_eq_total", "all8_cap_total_minus_1", "all8_cap_1", "eight_dests")


def check_pack_flags(lname, ref_ovf, off, specs):
    """The reference's own flags are the ones the case is built to produce."""
    n = (off[1:] - off[:-1]).tolist()
    if lname == "one_expert_slack":
        assert ref_ovf[0] == 0
    elif lname == "all8_cap_eq_total":
        assert ref_ovf[1] == 1 and ref_ovf[2:10].sum() == 0  # the pre-set word stays, nothing else is set
    elif lname == "all8_cap_total_minus_1":
        assert ref_ovf[1] == 1
        for (e, ef) in zip(C.PACK_ORDER, specs[0][4]):  # count - 1: flag, unless the expert is empty
            assert ef < 0 or ref_ovf[ef] == (1 if n[e] > 0 else 0)
    elif lname == "all8_cap_1":
        assert ref_ovf[1] == 1
    elif lname == "eight_dests":
        assert ref_ovf[4] == 1 and ref_ovf[1] == 1 and ref_ovf[16] == 1 and ref_ovf[0] == 0
    assert (ref_ovf[21:] == C.OVF_CANARY).all()  # words no destination names


def check_combine(M, k, H, dev):
    eo, slot_of, w, ranges = C.combine_case(M, k, H)
    eod, sld, wd = eo.to(dev), slot_of.to(dev), w.to(dev)
    for rname, rng in ranges.items():
        y64, mag = R.combine_ref(eo, slot_of, w, rng)
        rt = None if rng is None else torch.tensor(rng, dtype=torch.int32, device=dev)
        y = ops.moe_combine(eod, sld, wd, rt)
        assert y.dtype == torch.bfloat16 and tuple(y.shape) == (M, H)
        err = (y.cpu().double() - y64).abs()
        over = err > C.combine_bound(y64, mag)
        assert not over.any(), \
            f"range {rname} {rng}: {int(over.sum())} elements outside the bound, max err {err.max().item():.3g}"
        if rname == "empty":
            assert (y.cpu() == 0).all()
        out = torch.full((M, H), 5.0, dtype=torch.bfloat16, device=dev)  # the same values with out=
        ops.moe_combine(eod, sld, wd, rt, out=out)
        assert torch.equal(out, y)
    assert torch.equal(eod.cpu(), eo) and torch.equal(sld.cpu(), slot_of) and torch.equal(wd.cpu(), w)


def check_permute(rows, H, dev):
    x, src = C.permute_case(rows, H)
    ref = R.permute_ref(x, src)
    xd, sd = x.to(dev), src.to(dev)
    assert torch.equal(ops.moe_permute(xd, sd).cpu(), ref)
    out = torch.full((rows, H), 5.0, dtype=torch.bfloat16, device=dev)
    ops.moe_permute(xd, sd, out=out)
    assert torch.equal(out.cpu(), ref) and torch.equal(xd.cpu(), x)


def check_xbatch(name, dev):
    """offsets and a_rows[:offsets[G]] equal the reference; returns the words of a_rows past them."""
    offs, reqs, experts, bases = C.xbatch_case(name)
    ro, ra = R.xbatch_ref(offs, reqs, experts, bases)
    offsets = torch.full((len(reqs) + 1,), C.XBATCH_CANARY, dtype=torch.int32, device=dev)
    a_rows = torch.full((ra.numel() + C.XBATCH_SLACK,), C.XBATCH_CANARY, dtype=torch.int32, device=dev)
    ops.moe_xbatch_index([o.to(dev) for o in offs], reqs, experts, bases, offsets, a_rows)
    assert torch.equal(offsets.cpu(), ro)
    assert torch.equal(a_rows.cpu()[:ra.numel()], ra)
    return a_rows.cpu()[ra.numel():]
