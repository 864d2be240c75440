"""Inputs, oracle and mutants shared by the CPU and GPU tests of the KV cache and decode attention
(test_attn_decode_cpu.py, test_attn_decode_gpu.py), built on the CPU from fixed seeds, once per
process.

A case is a step: caches [B][C][nkv*D] holding ``pos[b]`` rows per sequence (every other row is
stale), and T new tokens per sequence as a packed qkv buffer. The step appends the new K and V
rows at ``pos[b] .. pos[b]+T-1`` and attends query t of sequence b to cache rows ``0 .. pos[b]+t``.
The kernel (csrc/kernels/attn_decode.hip) gives one workgroup one chunk of KC keys of one
(sequence, KV head) and merges the chunks that hold keys by tickets. The capacity is C = 640 and
the tests pass chunk = 128, so these small caches span five chunks; at D = 64 a 128-key chunk is
half of the kernel's 256-key stage, at D = 128 a whole one.

The oracle is ``attn_checks.ref64`` per sequence with S = pos+T, Sq = T, q_off = pos over the
appended cache, which this module builds by plain indexing: neither uses the CPU path of ``ops``.

Three kinds of case, as in attn_cases.py: random (per row against ref64), selector (every query
selects one key; the output is that key's value row bit for bit) and poison (keys that must not
be seen replace the row if they leak).
"""
import dataclasses
import functools
import math
from typing import Optional

import torch

import attn_cases as AC
import attn_checks as K

CAP = 640  # cache capacity C
CHUNK = 128  # keys per workgroup the tests pass: five chunks
B = 2

# Largest relative L2 error of one (row, head) of attn_decode against ref64 over every random
# case below, as test_attn_decode_gpu.py prints it on an MI355X. The tolerance is three times the
# measured figure rounded up to a power of two, the rule attn_checks.ROW_TOL was made by, and may
# not exceed that file's cap of 2^-6. Measured: 2.933e-3 in dec_d64_h2x2_t4_edge over the 54 random
# cases with chunk = 128 and the sampled ones with the launcher's chunk (the poison and guard cases,
# held to the same constant, reach 3.013e-3), so the tolerance is 2^-6.
MEASURED_ROW_ERR = 2.933e-3
ROW_TOL = 2.0 ** math.ceil(math.log2(3 * MEASURED_ROW_ERR))
assert ROW_TOL <= 2.0 ** -6


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    kind: str  # "random" | "selector" | "poison"
    q: torch.Tensor  # [B*T][nh*D], k_new / v_new [B*T][nkv*D]: column views of one packed buffer
    k_new: torch.Tensor
    v_new: torch.Tensor
    k_cache: torch.Tensor  # [B][C][nkv*D] before the step
    v_cache: torch.Tensor
    pos: tuple
    T: int
    nh: int
    nkv: int
    D: int
    want: Optional[torch.Tensor] = None  # selector: the exact output [B*T][nh*D]
    rows: Optional[torch.Tensor] = None  # poison: [B][T] bool, the query rows that are checked

    @property
    def dims(self):
        return (self.T, self.nh, self.nkv, self.D)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _packed(T, nh, nkv, D, g):
    qkv = torch.randn(B * T, (nh + 2 * nkv) * D, generator=g).to(torch.bfloat16)
    return qkv[:, :nh * D], qkv[:, nh * D:(nh + nkv) * D], qkv[:, (nh + nkv) * D:]


def appended(case):
    """The caches after the step's append (rows at or past C dropped), by plain indexing."""
    kc, vc = case.k_cache.clone(), case.v_cache.clone()
    for b, p in enumerate(case.pos):
        n = max(0, min(case.T, CAP - p))
        kc[b, p:p + n] = case.k_new[b * case.T:b * case.T + n]
        vc[b, p:p + n] = case.v_new[b * case.T:b * case.T + n]
    return kc, vc


def ref_step(case):
    """[B][T][nh][D] float64: ref64 per sequence with S = pos+T, Sq = T, q_off = pos."""
    kc, vc = appended(case)
    T, nh, nkv, D = case.dims
    out = []
    for b, p in enumerate(case.pos):
        out.append(K.ref64(case.q[b * T:(b + 1) * T], kc[b, :p + T], vc[b, :p + T], 1, p + T, nh, nkv, D, True,
                           Sq=T, q_off=p))
    return torch.cat(out)


_references = {}


def reference(case):
    if case.name not in _references:
        _references[case.name] = ref_step(case)
    return _references[case.name]


def check(out, case, tol, what, ref=None):
    """Every checked (row, head) of ``out`` ([B*T][>= nh*D]) within ``tol`` of the oracle, per sequence."""
    ref = reference(case) if ref is None else ref
    worst = 0.0
    for b, p in enumerate(case.pos):
        rows = None if case.rows is None else case.rows[b]
        worst = max(worst, K.check_rows(out[b * case.T:(b + 1) * case.T], ref[b:b + 1], tol, f"{what} sequence {b}",
                                        rows=rows, q_off=p))
    return worst


# ---------------------------------------------------------------------------------------------
# random cases
HEADS = [(4, 2), (4, 1), (2, 2)]
STEPS = [1, 4, 16]  # rep*T: one used column of 16 up to four full column groups


def pos_sets(T):
    """An empty cache beside a ragged one; both sides of a chunk edge; a cache filled to capacity."""
    return {"empty": (0, 389), "edge": (127, 128), "full": (CAP - T, 63)}


def _rname(D, nh, nkv, T, pname):
    return f"dec_d{D}_h{nh}x{nkv}_t{T}_{pname}"


def _build_random(D, nh, nkv, T, pname, seed=None):
    seed = 11 + D + 7 * nh + 13 * nkv + 31 * T + len(pname) if seed is None else seed
    g = _gen(seed)
    q, k, v = _packed(T, nh, nkv, D, g)
    kc = torch.randn(B, CAP, nkv * D, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, CAP, nkv * D, generator=g).to(torch.bfloat16)
    return Case(_rname(D, nh, nkv, T, pname), "random", q, k, v, kc, vc, pos_sets(T)[pname], T, nh, nkv, D)


# ---------------------------------------------------------------------------------------------
# selector cases: the +-1-code construction of attn_cases.py. Every cache row and new key is a
# random +-1 vector per (sequence, KV head), q = 16 * code[target]; the target scores 16 D / sqrt(D)
# and leads every other key by tens of nats, so ref64 rounds to the target's value row.
SELECTOR_SEED = 3
SELECTOR_POS = {"mid": (389, 127), "full": (None, 128)}  # None: C - T
SELECTOR_MAPS = {
    "own": lambda p, t: p + t,  # the query's own new token
    "key0": lambda p, t: 0,
    "chunk_first": lambda p, t: (p + t) // CHUNK * CHUNK,  # first key of the last chunk the query sees
    "chunk_before": lambda p, t: max((p + t) // CHUNK * CHUNK - 1, 0),  # last key of the chunk before it
    "prev": lambda p, t: max(p - 1, 0),  # the last key of the cache before the step
}


def _build_selector(mname, D, T, pname):
    nh, nkv = 4, 2
    pos = tuple(CAP - T if p is None else p for p in SELECTOR_POS[pname])
    g = _gen(SELECTOR_SEED)
    code = (2.0 * torch.randint(0, 2, (B, CAP, nkv, D), generator=g) - 1.0).to(torch.bfloat16)
    val = torch.randn(B, CAP, nkv, D, generator=g).to(torch.bfloat16)
    stale_k = (2.0 * torch.randint(0, 2, (B, CAP, nkv, D), generator=g) - 1.0).to(torch.bfloat16)
    stale_v = torch.randn(B, CAP, nkv, D, generator=g).to(torch.bfloat16)
    kvh = torch.arange(nh) // (nh // nkv)
    qkv = torch.zeros(B * T, (nh + 2 * nkv) * D, dtype=torch.bfloat16)
    q, k, v = qkv[:, :nh * D], qkv[:, nh * D:(nh + nkv) * D], qkv[:, (nh + nkv) * D:]
    kc, vc = stale_k.reshape(B, CAP, nkv * D).clone(), stale_v.reshape(B, CAP, nkv * D).clone()
    want = torch.zeros(B * T, nh * D, dtype=torch.bfloat16)
    for b, p in enumerate(pos):
        kc[b, :p] = code[b, :p].reshape(p, nkv * D)  # rows p .. stay stale: other codes, other values
        vc[b, :p] = val[b, :p].reshape(p, nkv * D)
        for t in range(T):
            tgt = SELECTOR_MAPS[mname](p, t)
            assert 0 <= tgt <= p + t
            k[b * T + t] = code[b, p + t].reshape(-1)
            v[b * T + t] = val[b, p + t].reshape(-1)
            q[b * T + t] = (16.0 * code[b, tgt][kvh]).reshape(-1)
            want[b * T + t] = val[b, tgt][kvh].reshape(-1)
    case = Case(f"decsel_{mname}_d{D}_t{T}_{pname}", "selector", q, k, v, kc, vc, pos, T, nh, nkv, D, want=want)
    check_selector(case)
    return case


def check_selector(case):
    """The case's precondition: the float64 oracle rounds to the selected value row, bit for bit."""
    got = ref_step(case).to(torch.bfloat16).reshape(B * case.T, case.nh * case.D)
    assert torch.equal(got, case.want), f"{case.name}: ref64 does not round to the selected row — change SELECTOR_SEED"


# ---------------------------------------------------------------------------------------------
# poison cases: attn_cases._beacon's scheme. Poisoned: every stale cache row of the victim
# sequence (rows pos+T ..), its new tokens t' > t0 (rows t <= t0 are checked), and the whole cache
# and step of the other sequence (whose rows are not checked). Over t0 = 0 .. T-1 and both victims
# every row is checked.
POISON_POS = {"edge": (127, 128), "ragged": (389, 63)}


def poison_t0(T):
    return sorted({0, T // 2, T - 1})


def _build_poison(D, T, pname, victim, t0):
    nh, nkv = 4, 2
    pos = POISON_POS[pname]
    g = _gen(600 + D + 3 * T + 17 * victim + t0 + len(pname))
    q, k, v = _packed(T, nh, nkv, D, g)
    kc = torch.randn(B, CAP, nkv * D, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, CAP, nkv * D, generator=g).to(torch.bfloat16)
    seq_c = torch.arange(B * CAP) // CAP
    row_c = torch.arange(B * CAP) % CAP
    seq_n = torch.arange(B * T) // T
    tok_n = torch.arange(B * T) % T
    AC._beacon(q, kc.view(B * CAP, -1), vc.view(B * CAP, -1), nh, nkv, D,
               (seq_c != victim) | (row_c >= pos[victim] + T))
    AC._beacon(q, k, v, nh, nkv, D, (seq_n != victim) | (tok_n > t0))
    rows = torch.zeros(B, T, dtype=torch.bool)
    rows[victim, :t0 + 1] = True
    return Case(f"decpoison_d{D}_t{T}_{pname}_v{victim}_upto{t0}", "poison", q, k, v, kc, vc, pos, T, nh, nkv, D,
                rows=rows)


# ---------------------------------------------------------------------------------------------
_BUILDERS = {}
for _D in (64, 128):
    for _nh, _nkv in HEADS:
        for _T in STEPS:
            for _p in pos_sets(_T):
                _BUILDERS[_rname(_D, _nh, _nkv, _T, _p)] = functools.partial(_build_random, _D, _nh, _nkv, _T, _p)
RANDOM_CASES = tuple(_BUILDERS)
for _m in SELECTOR_MAPS:
    for _D in (64, 128):
        for _T in STEPS:
            for _p in SELECTOR_POS:
                _BUILDERS[f"decsel_{_m}_d{_D}_t{_T}_{_p}"] = functools.partial(_build_selector, _m, _D, _T, _p)
SELECTOR_CASES = tuple(n for n in _BUILDERS if n.startswith("decsel_"))
for _D in (64, 128):
    for _T in STEPS:
        for _p in POISON_POS:
            for _v in range(B):
                for _t0 in poison_t0(_T):
                    _BUILDERS[f"decpoison_d{_D}_t{_T}_{_p}_v{_v}_upto{_t0}"] = functools.partial(
                        _build_poison, _D, _T, _p, _v, _t0)
POISON_CASES = tuple(n for n in _BUILDERS if n.startswith("decpoison_"))


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of that name, built once per process; its tensors are shared and stay unchanged."""
    return _BUILDERS[name]()


# ---------------------------------------------------------------------------------------------
# layout, ticket and append cases
OUT_SENTINEL = -77.0
GUARD_ROWS, GUARD_COLS = 3, 32
CACHE_SENTINEL = -55.0
APPEND_POS = [(0, 389), (127, 128), (CAP - 2, CAP)]  # the last: two of four rows fit, then none


@functools.lru_cache(maxsize=None)
def guard_case(D):
    """rep*T = 8: half a column group is padding; five and one active chunks."""
    return dataclasses.replace(_build_random(D, 4, 2, 4, "full", seed=900 + D), name=f"decguard_d{D}")


@functools.lru_cache(maxsize=None)
def twice_cases(D, T):
    """Two steps of one shape for two launches on one workspace: five and four active chunks,
    then two and one — over the first launch's tickets and stale partials."""
    a = dataclasses.replace(_build_random(D, 4, 1, T, "full", seed=9000 + D + T), name=f"dectwice_d{D}_t{T}_0",
                            pos=(CAP - T, 389))
    b = dataclasses.replace(_build_random(D, 4, 1, T, "full", seed=9500 + D + T), name=f"dectwice_d{D}_t{T}_1",
                            pos=(200, 5))
    return a, b


# ---------------------------------------------------------------------------------------------
# Mutants: what a subtly wrong kernel would return, written with ref64's hooks over the WHOLE
# appended caches (S = C, kv_batch picks the sequence, ``visible`` is the mask).

def _visible(p, T, last=None):
    """[T][C] bool: key <= p + t (``last``: another per-row last key)."""
    last = p + torch.arange(T) if last is None else last
    return torch.arange(CAP)[None, :] <= last[:, None]


def ref_hooks(case, visible=None, kv_head=None, kv_batch=None):
    """ref64 over the whole caches; ``visible(b, p, T)`` -> [T][C] bool, ``kv_batch(b)`` -> sequence."""
    kc, vc = appended(case)
    T, nh, nkv, D = case.dims
    kf, vf = kc.reshape(B * CAP, -1), vc.reshape(B * CAP, -1)
    out = []
    for b, p in enumerate(case.pos):
        vis = _visible(p, T) if visible is None else visible(b, p, T)
        src = b if kv_batch is None else kv_batch(b)
        out.append(K.ref64(case.q[b * T:(b + 1) * T], kf, vf, 1, CAP, nh, nkv, D, True, Sq=T, q_off=p, visible=vis,
                           kv_head=kv_head, kv_batch=lambda _b, src=src: src))
    return torch.cat(out)


def _mut_new_tokens_uncausal(case):
    """Every query sees all T new tokens."""
    return dict(visible=lambda b, p, T: _visible(p, T, torch.full((T,), p + T - 1)))


def _mut_strict(case):
    """key < pos + t in place of key <= pos + t."""
    return dict(visible=lambda b, p, T: _visible(p, T, p + torch.arange(T) - 1))


def _mut_pos0(case):
    """pos[0] used for every sequence."""
    return dict(visible=lambda b, p, T: _visible(case.pos[0], T))


def _mut_ragged_dropped(case):
    """The keys of the ragged last chunk are never read."""
    return dict(visible=lambda b, p, T: _visible(p, T) & (torch.arange(CAP)[None, :] < (p + T) // CHUNK * CHUNK))


def _mut_stale_visible(case):
    """Stale keys are visible up to the end of the last active chunk."""
    return dict(visible=lambda b, p, T: _visible(p, T) | ((torch.arange(CAP)[None, :] >= p + T)
                                                           & (torch.arange(CAP)[None, :] < -(-(p + T) // CHUNK) * CHUNK)))


def _mut_chunk1_lost(case):
    """Chunk 1 is lost when three or more chunks are active (a partial merged over)."""
    def vis(b, p, T):
        key = torch.arange(CAP)[None, :]
        lost = (key >= CHUNK) & (key < 2 * CHUNK) if -(-(p + T) // CHUNK) >= 3 else torch.zeros(1, CAP, dtype=torch.bool)
        return _visible(p, T) & ~lost
    return dict(visible=vis)


def _mut_h_mod(case):
    """KV head h % nkv in place of h // (nh / nkv)."""
    return dict(kv_head=lambda h: h % case.nkv)


MUTANTS = {"new_tokens_uncausal": _mut_new_tokens_uncausal, "strict_causal": _mut_strict, "pos0_for_all": _mut_pos0,
           "ragged_last_chunk_dropped": _mut_ragged_dropped, "stale_visible_to_chunk_end": _mut_stale_visible,
           "chunk1_lost": _mut_chunk1_lost, "kv_head_modulo": _mut_h_mod}


def mutant_out(mutant, case):
    """The mutant's float64 output [B][T][nh][D] for ``case``, or None where it changes nothing."""
    kw = MUTANTS[mutant](case)
    if "kv_head" in kw and all(kw["kv_head"](h) == h // (case.nh // case.nkv) for h in range(case.nh)):
        return None
    if "visible" in kw and all(torch.equal(kw["visible"](b, p, case.T), _visible(p, case.T))
                               for b, p in enumerate(case.pos)):
        return None
    return ref_hooks(case, **kw)
