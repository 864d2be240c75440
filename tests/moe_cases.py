"""Inputs shared by the CPU and GPU tests of the MoE routing kernels (test_moe_ref_cpu.py,
test_moe_kernels_gpu.py), with the reference results computed once per case (moe_ref.py).

Every routing case is a bf16 logits matrix [M][E] and a k; rows of all -inf logits and NaN
logits are outside the routing contract and appear nowhere.
"""
import functools

import torch

import moe_ref

NEG_INF = float("-inf")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _tie_free(M, E, seed):
    g = _gen(seed)
    v = torch.stack([torch.randperm(E, generator=g) for _ in range(M)]).float().mul(0.25)
    return (v + 0.01 * torch.randn(M, E, generator=g)).to(torch.bfloat16)


def _quantised(M, E, seed):
    levels = torch.tensor([-1.0, 0.0, 0.5, 1.0])
    return levels[torch.randint(0, 4, (M, E), generator=_gen(seed))].to(torch.bfloat16)


def _skewed(M, E, hot, cold, seed):
    """Every token prefers the ``hot`` experts (in that order); the ``cold`` ones are never chosen."""
    v = torch.randn(M, E, generator=_gen(seed)).clamp(-2, 2)
    for r, e in enumerate(hot):
        v[:, e] = 8.0 - r
    for e in cold:
        v[:, e] = -8.0
    return v.to(torch.bfloat16)


def _masked(M, E, finite_lo, finite_hi, seed):
    """Each row keeps between finite_lo and finite_hi finite logits; the rest are -inf."""
    g = _gen(seed)
    v = torch.randn(M, E, generator=g)
    for m in range(M):
        n_fin = int(torch.randint(finite_lo, finite_hi + 1, (1,), generator=g))
        v[m, torch.randperm(E, generator=g)[n_fin:]] = NEG_INF
    return v.to(torch.bfloat16)


def _wide(M, E, seed):
    g = _gen(seed)
    v = 60.0 * (2.0 * torch.randint(0, 2, (M, E), generator=g).float() - 1.0)
    v[: M // 4] = -60.0  # a quarter of the rows: exactly one +60, every other gate underflows
    v[torch.arange(M // 4), torch.randint(0, E, (M // 4,), generator=g)] = 60.0
    v[M // 2:] += torch.randn(M - M // 2, E, generator=g)
    return v.to(torch.bfloat16)


def _random(M, E, seed):
    return torch.randn(M, E, generator=_gen(seed)).to(torch.bfloat16)


# name -> (builder, k); the builders run on first use
ROUTE_CASES = {
    "tie_free_300x8k2": (lambda: _tie_free(300, 8, 1), 2),
    "quant_257x8k2": (lambda: _quantised(257, 8, 2), 2),
    "quant_200x16k4": (lambda: _quantised(200, 16, 3), 4),
    "quant_200x64k8": (lambda: _quantised(200, 64, 4), 8),
    "quant_64x5k5": (lambda: _quantised(64, 5, 5), 5),
    "quant_33x2k1": (lambda: _quantised(33, 2, 7), 1),  # a seed with 12 tied rows of 33
    "const_37x8k2": (lambda: torch.full((37, 8), 0.5).to(torch.bfloat16), 2),
    "const_9x64k8": (lambda: torch.full((9, 64), -3.0).to(torch.bfloat16), 8),
    "const_1x4k4": (lambda: torch.zeros(1, 4).to(torch.bfloat16), 4),
    "skew_last2_300x8k2": (lambda: _skewed(300, 8, (7, 6), (), 7), 2),
    "skew_first2_300x8k2": (lambda: _skewed(300, 8, (0, 1), (), 8), 2),
    "skew_middle_empty_300x8k2": (lambda: _skewed(300, 8, (), (3, 4), 9), 2),
    "one_token_1x8k2": (lambda: _random(1, 8, 10), 2),
    "chunk_1023x16k1": (lambda: _random(1023, 16, 11), 1),
    "chunk_1024x16k1": (lambda: _random(1024, 16, 12), 1),
    "chunk_1025x16k1": (lambda: _random(1025, 16, 13), 1),
    "fused_limit_8192x8k2": (lambda: _random(8192, 8, 14), 2),
    "past_limit_8193x8k2": (lambda: _random(8193, 8, 15), 2),
    "masked_100x8k2": (lambda: _masked(100, 8, 2, 7, 16), 2),
    "masked_short_50x8k4": (lambda: _masked(50, 8, 1, 3, 17), 4),
    "wide_100x8k2": (lambda: _wide(100, 8, 18), 2),
    "wide_64x16k4": (lambda: _wide(64, 16, 19), 4),
}
ROUTE_MAX_ASSIGN = 16384  # kRouteMaxAssign (kernels.h): the fused route kernel's limit


@functools.lru_cache(maxsize=None)
def route_case(name):
    """(logits bf16 [M][E], k, (idx, gate64, src_rows, slot_of, offsets)) — computed once, shared
    by every test; callers do not modify the tensors."""
    build, k = ROUTE_CASES[name]
    logits = build()
    idx, gate = moe_ref.route_ref(logits, k)
    return logits, k, (idx, gate) + moe_ref.align_ref(idx, logits.shape[1])


def boundary_ties(logits, k):
    """Rows whose k-th and (k+1)-th largest logits are equal: the selected SET depends on the tie rule."""
    s = logits.float().sort(-1, descending=True).values
    return int((s[:, k - 1] == s[:, k]).sum())


def inner_ties(logits, k):
    """Rows with two equal logits among the k largest: the ORDER of idx depends on the tie rule."""
    s = logits.float().sort(-1, descending=True).values[:, :k]
    return int((s[:, 1:] == s[:, :-1]).any(-1).sum())


def check_case_shape(name):
    """What each family claims about its own input — keeps a case from silently degenerating."""
    logits, k, (idx, gate, _src, _slot, off) = route_case(name)
    M, E = logits.shape
    counts = (off[1:] - off[:-1]).tolist()
    if name.startswith("tie_free"):
        assert k < E and boundary_ties(logits, k) == 0 and inner_ties(logits, k) == 0
    elif name == "quant_64x5k5":
        assert k == E and inner_ties(logits, k) * 4 >= M
    elif name.startswith("quant"):
        assert boundary_ties(logits, k) * 4 >= M, (name, boundary_ties(logits, k), M)
    elif name.startswith("const"):
        assert torch.equal(idx, torch.arange(k, dtype=torch.int32).expand(M, k))
        assert torch.equal(gate, torch.full((M, k), 1.0 / k, dtype=torch.float64))
    elif name == "skew_last2_300x8k2":
        assert counts == [0] * 6 + [M, M]
    elif name == "skew_first2_300x8k2":
        assert counts == [M, M] + [0] * 6
    elif name == "skew_middle_empty_300x8k2":
        assert counts[3] == 0 and counts[4] == 0 and min(counts[:3] + counts[5:]) > 0
    elif name == "fused_limit_8192x8k2":
        assert M * k == ROUTE_MAX_ASSIGN
    elif name == "past_limit_8193x8k2":
        assert M * k == ROUTE_MAX_ASSIGN + 2
    elif name == "masked_100x8k2":
        fin = torch.isfinite(logits.float())
        assert (fin.sum(-1) >= k).all() and (~fin).any() and fin.gather(1, idx.long()).all()
    elif name == "masked_short_50x8k4":
        fin = torch.isfinite(logits.float())
        assert (fin.sum(-1) < k).all() and (fin.sum(-1) >= 1).all()
        assert (gate[~fin.gather(1, idx.long())] == 0).all()  # selected -inf experts: gate exactly 0
    elif name.startswith("wide"):
        assert logits.float().abs().max() >= 60 and torch.isfinite(gate).all() and (gate < 1e-40).any()


# ------------------------------------------------------------------ pack / unpack
PACK_E, PACK_K, PACK_M = 8, 2, 400
# the eight experts out of order; under the skewed routing (only experts 1, 2, 4, 6 are used) the
# list starts with an empty expert, has empty ones in the middle and ends with one
PACK_ORDER = (7, 2, 5, 6, 3, 1, 4, 0)
OVF_WORDS = 24
OVF_CANARY = 7  # words no destination names


@functools.lru_cache(maxsize=None)
def pack_routing(kind):
    """(src_rows, offsets) of the reference routing of 400 tokens over 8 experts, k = 2."""
    if kind == "skewed":
        logits = _skewed(PACK_M, PACK_E, (), (0, 3, 5, 7), 30)
    else:
        logits = _random(PACK_M, PACK_E, 31)
    idx, _ = moe_ref.route_ref(logits, PACK_K)
    src, _slot, off = moe_ref.align_ref(idx, PACK_E)
    counts = (off[1:] - off[:-1]).tolist()
    if kind == "skewed":
        assert [c == 0 for c in counts] == [True, False, False, True, False, True, False, True]
    else:
        assert min(counts) > 1
    return src, off


def pack_dest_lists(kind):
    """name -> ([(cap, experts, flag, ecaps, eflags)], preset): the destination lists of one
    launch (buffers are the test's) and the ovf words that are 1 before it."""
    _src, off = pack_routing(kind)
    n = (off[1:] - off[:-1]).tolist()
    total = sum(n)
    big = max(range(PACK_E), key=lambda e: n[e])
    assert total == PACK_M * PACK_K > 256  # the all-experts lists take a second grid-stride pass
    none8 = [-1] * 8
    at_count = [n[e] for e in PACK_ORDER]  # ecap == count: no flag
    below = [max(n[e] - 1, 0) for e in PACK_ORDER]  # ecap == count - 1: flag (empty experts: 0, no flag)
    mixed_flags = [10, -1, 11, 12, -1, 13, -1, 14]
    # one launch, eight destinations (expert PACK_ORDER[d] each: disjoint rows): caps at, below and
    # above the count and cap 1; flags and expert flags present or -1. Destination 4 has cap ==
    # count and its word (4) is 1 before the launch: it must stay 1.
    eight = []
    for d, e in enumerate(PACK_ORDER):
        delta = (0, -1, 3, None, 0, 2, -2, 1)[d]
        cap = 1 if delta is None else max(n[e] + delta, 1)
        eight.append((cap, (e,), (0, 1, -1, 3, 4, -1, 6, 7)[d], [max(n[e] - d % 2, 0)],
                      [(-1, 16, 17, -1, 18, 19, -1, 20)[d]]))
    lists = {
        "one_expert_slack": ([(n[big] + 5, (big,), 0, [n[big] + 5], [-1])], ()),
        # word 1 is 1 before the launch and no count exceeds anything: it must stay 1
        "all8_cap_eq_total": ([(total, PACK_ORDER, 1, at_count, list(range(2, 10)))], (1,)),
        "all8_cap_total_minus_1": ([(total - 1, PACK_ORDER, 1, below, mixed_flags)], ()),
        "all8_cap_1": ([(1, PACK_ORDER, 1, at_count, none8)], ()),
        "eight_dests": (eight, (4,)),
    }
    return lists


def ovf_initial(dests, preset):
    ovf = torch.full((OVF_WORDS,), OVF_CANARY, dtype=torch.int32)
    for _cap, _experts, flag, _ecaps, eflags in dests:
        for f in [flag] + list(eflags):
            if f >= 0:
                ovf[f] = 0
    for f in preset:
        ovf[f] = 1
    return ovf


# ------------------------------------------------------- combine / permute / xbatch
COMBINE_SHAPES = [(M, k, H) for M in (1, 77) for k in (1, 2, 8) for H in (64, 520, 4096)]


@functools.lru_cache(maxsize=None)
def combine_case(M, k, H):
    """(expert_out bf16 [M*k][H], slot_of int32 [M*k], w fp32 [M][k], {range name: (r0, r1) or None})."""
    g = _gen(1000 * M + 10 * k + H)
    R = M * k
    eo = torch.randn(R, H, generator=g).to(torch.bfloat16)
    slot_of = torch.randperm(R, generator=g).to(torch.int32)
    w = torch.softmax(torch.randn(M, k, generator=g), -1)
    ranges = {"absent": None, "middle": (R // 3, max(2 * R // 3, R // 3 + 1)), "empty": (R // 2, R // 2),
              "full": (0, R)}
    return eo, slot_of, w, ranges


def combine_bound(y64, mag64):
    """Elementwise bound on |y - ref|: fp32 accumulation of at most eight products — eight
    products and eight additions, each rounded with a relative error of at most 2^-24 of a
    quantity no larger than S = sum |g_j v_j|, so at most 16 * 2^-24 * S = 2^-20 * S — then
    one rounding to bf16, at most one unit in the last place of the result (2^-8 relative)."""
    return 2.0 ** -8 * y64.abs() + 2.0 ** -20 * mag64


PERMUTE_SHAPES = [(rows, H) for rows in (1, 5, 1000) for H in (8, 520)]


@functools.lru_cache(maxsize=None)
def permute_case(rows, H):
    """(x bf16 [n][H], src int32 [rows]) with repeated source rows whenever rows > 1."""
    g = _gen(rows + H)
    n = max(1, rows // 2)
    return torch.randn(n, H, generator=g).to(torch.bfloat16), torch.randint(0, n, (rows,), generator=g).to(torch.int32)


def _offsets(counts):
    return torch.tensor([0] + torch.tensor(counts).cumsum(0).tolist(), dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def xbatch_case(name):
    """(offs: per request int32 [E+1], reqs, experts, bases) of one cross-request expert batch."""
    g = _gen(77)
    if name == "one_group":
        offs, pairs = [_offsets([3, 0, 5, 2])], [(0, 2)]
    elif name == "maxima_q16_g64":
        offs = [_offsets(torch.randint(0, 9, (8,), generator=g).tolist()) for _ in range(16)]
        order = torch.randperm(16 * 8, generator=g)[:64].tolist()
        pairs = [(p // 8, p % 8) for p in order]
    elif name == "empty_experts":
        offs = [_offsets([0, 4, 0, 0, 7, 0]), _offsets([0, 0, 0, 0, 0, 0]), _offsets([2, 0, 0, 1, 0, 0])]
        pairs = [(0, 0), (1, 3), (0, 4), (2, 1), (2, 0), (0, 5), (1, 0), (2, 3), (0, 1)]
    elif name == "group_over_256_rows":
        offs, pairs = [_offsets([10, 300, 4]), _offsets([1, 2, 600])], [(0, 2), (0, 1), (1, 2), (1, 0)]
    else:
        raise KeyError(name)
    rows = [int(o[-1]) for o in offs]
    bases = [sum(rows[:q]) for q in range(len(offs))]
    return offs, [p[0] for p in pairs], [p[1] for p in pairs], bases


XBATCH_CASES = ("one_group", "maxima_q16_g64", "empty_experts", "group_over_256_rows")
XBATCH_CANARY = -12345
XBATCH_SLACK = 16  # a_rows words past offsets[G]: they keep the canary
