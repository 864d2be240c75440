"""Cases, oracle and mutants of the chunk attention over the KV cache (``ops.attention_chunk``,
csrc/kernels/attn_chunk.hip), shared by test_attn_chunk_cpu.py and test_attn_chunk_gpu.py.

Everything is built with the builders of attn_decode_cases.py (and attn_decode_fp8_cases.py for the
e4m3 caches) at chunk widths the decode kernel does not take: B = 2, C = 640, T in {17, 40, 64} —
one past a 16-query wave, a 32-query tile plus eight rows, an exact 64-query tile — over D in
{64, 128}, the heads (4, 2), (4, 1), (2, 2) and the three position sets of ``pos_sets(T)``: an empty
cache beside a ragged one, both sides of a 128-key edge, a cache filled to capacity. The oracle is
attn_decode_cases.reference: ``attn_checks.ref64`` per sequence over the appended cache.

Poison cases: every cache row at or past ``pos[b]+T`` is NaN (K and V): the kernel may not read
them at all, and one that bounded its keys by C would turn its outputs into NaN. The later keys of
the chunk (tokens t' > t0 of the victim) and the other sequence hold attn_decode_cases' beacon rows,
which replace a row they leak into. The "later" cases add NaN in the later keys themselves: the K
rows of the tokens t' > t0 (``check_upto`` looks at rows 0 .. t0 only: the later rows see a NaN key
by right). Their V rows stay finite, and that is the contract ``ops.attention_chunk`` states: rows
of a loaded tile that the causal mask hides enter the second MFMA as 0 x v (``ops.attention`` has the
same property), so the V rows ``pos[b]+t < r < pos[b]+T`` — which the step's own append wrote —
must be finite. ``value_row_case`` pins that property on both paths. The fp8 poison cases keep
attn_decode_fp8_cases' form (NaN bytes and scales in the stale rows, beacon later rows): the chunk
kernel runs on the dequantised bf16 workspace, so the bf16 later-key cases are its cover.

Of the tests over these cases, the self-checks of the cases — the honest-kernel model, the poison
preconditions and the two mutant rejections in test_attn_chunk_cpu.py — exercise only this module
and the oracle, so they would pass without the feature; every other test calls the new ops.
"""
import dataclasses
import functools
import math

import torch

import attn_checks as K
import attn_decode_cases as C
import attn_decode_fp8_cases as F

CAP, B = C.CAP, C.B
STEPS = [17, 40, 64]
HEADS = C.HEADS
VARIANTS = (2, 8, 13)  # ops.CHUNK_VARIANTS: every configuration the launcher can choose

# Largest relative L2 error of one (row, head) of attention_chunk against ref64, as
# test_attn_chunk_gpu.py prints it on an MI355X over every random case here (bf16 and fp8 caches,
# the launcher's choice and each variant). The tolerance is three times the figure rounded up to a
# power of two, the rule of attn_decode_cases.ROW_TOL, and may not exceed its cap of 2^-6.
# Measured: 4.483e-3 in f8chunk_d64_h4x2_t40_edge (sequence 0) over the 54 bf16 and 54 fp8 random
# cases and the 54 variant runs; the bf16 cases alone reach 3.486e-3 (chunk_d64_h2x2_t40_full). The
# fp8 figure is the larger for the reason attn_decode_fp8_cases.py gives: its V rows span 2^-6 ..
# 2^6, so few keys carry a row. 3 x 4.483e-3 = 0.01345, so the tolerance is 2^-6.
MEASURED_ROW_ERR = 4.483e-3
ROW_TOL = 2.0 ** math.ceil(math.log2(3 * MEASURED_ROW_ERR))
assert ROW_TOL <= 2.0 ** -6

pos_sets = C.pos_sets


def _rname(D, nh, nkv, T, pname):
    return f"chunk_d{D}_h{nh}x{nkv}_t{T}_{pname}"


def _build_random(D, nh, nkv, T, pname):
    return dataclasses.replace(C._build_random(D, nh, nkv, T, pname), name=_rname(D, nh, nkv, T, pname))


def _build_selector(mname, D, T, pname):
    c = C._build_selector(mname, D, T, pname)
    return dataclasses.replace(c, name="chunk" + c.name[3:])


def _build_poison(D, T, pname, victim, t0):
    c = C._build_poison(D, T, pname, victim, t0)  # fresh tensors: changed in place
    for b, p in enumerate(c.pos):
        c.k_cache[b, p + T:] = math.nan
        c.v_cache[b, p + T:] = math.nan
    return dataclasses.replace(c, name="chunk" + c.name[3:])


def _build_poison_later_keys(D, T, pname, victim, t0):
    """NaN also in the LATER KEYS of the chunk: the K rows of the victim's tokens t' > t0 (their
    V rows keep the beacon's finite 2^14). The victim's rows t <= t0 are checked with
    ``check_upto``; its rows t > t0 see a NaN key and are NaN by right."""
    c = _build_poison(D, T, pname, victim, t0)
    c.k_new[victim * T + t0 + 1:(victim + 1) * T] = math.nan
    return dataclasses.replace(c, name="chunklater" + c.name[len("chunkpoison"):])


def check_upto(out, c, tol, what):
    """The checked rows of a later-keys case (rows 0 .. t0 of the victim) against the oracle; the
    other rows of the output are not looked at."""
    T = c.T
    victim = int(c.rows.any(dim=1).nonzero()[0])
    n = int(c.rows[victim].sum())
    ref = C.reference(c)
    assert torch.isfinite(ref[victim, :n]).all()
    return K.check_rows(out[victim * T:victim * T + n], ref[victim:victim + 1, :n], tol, what, q_off=c.pos[victim])


def value_row_case(D):
    """The contract's other half, pinned: a V row of a later key inside a loaded tile must be
    FINITE — it enters the second MFMA as 0 x v. T = 40 at pos 127 / 128, NaN in the V row of
    token t0 + 1 = 21 of the victim (sequence 0): key 148, inside query 20's 64-key tile."""
    c = _build_poison(D, 40, "edge", 0, 20)
    c.v_new[21] = math.nan
    return dataclasses.replace(c, name=f"chunkvalue_d{D}")


_BUILDERS = {}
for _D in (64, 128):
    for _nh, _nkv in HEADS:
        for _T in STEPS:
            for _p in pos_sets(_T):
                _BUILDERS[_rname(_D, _nh, _nkv, _T, _p)] = functools.partial(_build_random, _D, _nh, _nkv, _T, _p)
RANDOM_CASES = tuple(_BUILDERS)
for _m in C.SELECTOR_MAPS:
    for _D in (64, 128):
        for _T in STEPS:
            for _p in C.SELECTOR_POS:
                _BUILDERS[f"chunksel_{_m}_d{_D}_t{_T}_{_p}"] = functools.partial(_build_selector, _m, _D, _T, _p)
SELECTOR_CASES = tuple(n for n in _BUILDERS if n.startswith("chunksel_"))
for _D in (64, 128):
    for _T in STEPS:
        for _p in C.POISON_POS:
            for _v in range(B):
                for _t0 in C.poison_t0(_T):
                    _BUILDERS[f"chunkpoison_d{_D}_t{_T}_{_p}_v{_v}_upto{_t0}"] = functools.partial(
                        _build_poison, _D, _T, _p, _v, _t0)
POISON_CASES = tuple(n for n in _BUILDERS if n.startswith("chunkpoison_"))
for _D in (64, 128):
    for _T in STEPS:
        for _p in C.POISON_POS:
            for _v in range(B):
                for _t0 in C.poison_t0(_T)[:-1]:  # (t0 = T - 1 has no later key)
                    _BUILDERS[f"chunklater_d{_D}_t{_T}_{_p}_v{_v}_upto{_t0}"] = functools.partial(
                        _build_poison_later_keys, _D, _T, _p, _v, _t0)
LATER_KEY_CASES = tuple(n for n in _BUILDERS if n.startswith("chunklater_"))
EDGE_CASES = tuple(n for n in RANDOM_CASES if n.endswith("_edge"))


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of that name, built once per process; its tensors are shared and stay unchanged."""
    return _BUILDERS[name]()


check = C.check
appended = C.appended


# ---------------------------------------------------------------------------------------------
# a chunk that runs past the capacity: rows at positions >= C are unspecified but finite

@functools.lru_cache(maxsize=None)
def overflow_case(D):
    """T = 40 from pos = (C - 5, C): five rows of sequence 0 fit, none of sequence 1."""
    c = C._build_random(D, 4, 2, 40, "full", seed=4000 + D)
    rows = torch.zeros(B, 40, dtype=torch.bool)
    rows[0, :5] = True
    return dataclasses.replace(c, name=f"chunkover_d{D}", pos=(CAP - 5, CAP), rows=rows)


def overflow_reference(c):
    """ref64 with S = min(pos + T, C): attn_decode_cases.ref_step assumes pos + T <= C."""
    kc, vc = C.appended(c)
    T, nh, nkv, D = c.dims
    out = []
    for b, p in enumerate(c.pos):
        S = min(p + T, CAP)
        vis = torch.arange(S)[None, :] <= (p + torch.arange(T))[:, None]
        out.append(K.ref64(c.q[b * T:(b + 1) * T], kc[b, :S], vc[b, :S], 1, S, nh, nkv, D, True, Sq=T, q_off=p,
                           visible=vis))
    return torch.cat(out)


# ---------------------------------------------------------------------------------------------
# fp8 caches: attn_decode_fp8_cases' per-row power-of-two scaling at the chunk widths

def _f8name(D, nh, nkv, T, pname):
    return "f8" + _rname(D, nh, nkv, T, pname)


def _build_random8(D, nh, nkv, T, pname):
    return F._build_random(D, nh, nkv, T, pname, name=_f8name(D, nh, nkv, T, pname))


def _build_poison8(D, T, pname, victim, t0):
    c = F._build_poison(D, T, pname, victim, t0)
    name = "f8chunk" + c.name[5:]
    return dataclasses.replace(c, name=name, eq=dataclasses.replace(c.eq, name=name))


_BUILDERS8 = {}
for _D in (64, 128):
    for _nh, _nkv in HEADS:
        for _T in STEPS:
            for _p in pos_sets(_T):
                _BUILDERS8[_f8name(_D, _nh, _nkv, _T, _p)] = functools.partial(_build_random8, _D, _nh, _nkv, _T, _p)
RANDOM_CASES8 = tuple(_BUILDERS8)
for _D in (64, 128):
    for _p in ("edge", "ragged"):
        for _v in range(B):
            _BUILDERS8[f"f8chunkpoison_d{_D}_t40_{_p}_v{_v}_upto20"] = functools.partial(_build_poison8, _D, 40, _p, _v, 20)
POISON_CASES8 = tuple(n for n in _BUILDERS8 if n.startswith("f8chunkpoison_"))


@functools.lru_cache(maxsize=None)
def case8(name):
    return _BUILDERS8[name]()


def dequantized_rows_expected(c8, kq, ks, sentinel):
    """What kv_dequantize_rows leaves in a sentinel-filled bf16 buffer: the dequantised rows below
    pos[b]+T of the (appended) byte cache ``kq`` / ``ks``, the sentinel in every other row."""
    want = torch.full(kq.shape, sentinel, dtype=torch.bfloat16)
    dq = F.dequantize_cache(kq, ks)
    for b, p in enumerate(c8.pos):
        n = min(p + c8.T, CAP)
        want[b, :n] = dq[b, :n]
    return want


# ---------------------------------------------------------------------------------------------
# kv_advance: pos[b] = min(pos[b] + T, max(limit[b], pos[b])), limit < pos included
ADVANCE_CASES = [
    # (pos, limit, T)
    ((0, 5, 100, 639), (13, 4, 100, 640), 5),
    ((0, 0, 0), (64, 3, 0), 64),
    ((7, 7), (3, 1000), 48),
    ((10,), (12,), 1),
]


def advance_expected(pos, limit, T):
    return [min(p + T, max(l, p)) for p, l in zip(pos, limit)]


# ---------------------------------------------------------------------------------------------
# Mutants: what a wrong kernel entry would return, with attn_decode_cases' ref64 hooks.

def mutant_q_off_zero(c):
    """The entry hands attn_item q_off = 0: query t sees keys 0 .. t only. None where pos is 0."""
    if all(p == 0 for p in c.pos):
        return None
    return C.ref_hooks(c, visible=lambda b, p, T: C._visible(0, T))


def mutant_keys_bounded_by_capacity(c):
    """S = C in place of min(pos+T, C): the causal mask still hides the stale rows' scores, but the
    rows are loaded and enter the second MFMA as 0 x v — ref64 over the WHOLE caches multiplies
    the same zeros with them, so NaN stale rows turn the output into NaN. None where no row is stale."""
    if all(p + c.T >= CAP for p in c.pos):
        return None
    return C.ref_hooks(c)
