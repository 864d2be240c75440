"""Inputs shared by the CPU and GPU tests of flash attention (test_attn_ref_cpu.py,
test_attn_kernels_gpu.py), built on the CPU from fixed seeds, once per process.

The kernel (csrc/kernels/attention_impl.h) walks 64 keys per wave and stage, 64-256 keys per
stage (KS = 1, 2, 4 key groups), 16-64 queries per block, through a ring of ST = 2-8 K/V buffers;
masks are applied only on diagonal and ragged tiles. The sizes below are chosen against those:
S = 600 (D = 64) is ten 64-key tiles, so the 8-stage ring of variants 6 and 7 wraps, and is
ragged for 64, 128 and 256 keys per stage; S = 400 (D = 128) wraps ST = 4 and 5. Heads are few:
what matters is S relative to the tiles.

Three kinds of case:
  random    N(0,1) bf16, checked per row against attn_checks.ref64 to ROW_TOL;
  selector  every query selects exactly one key (+-1 codes, 16x gain): the output equals that
            key's value row bit for bit, so a wrong key, head or batch is an exact mismatch;
  poison    keys that must not be seen score 45-64 nats above the rest and carry v = 2^14, so
            one leaked key replaces the row.
"""
import dataclasses
import functools
from typing import Optional

import torch

import attn_checks as K

ALL_VARIANTS = tuple(range(15))  # 0: the launcher's choice; 1-13: attention.hip; 14: key-split with tickets


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    name: str
    kind: str  # "random" | "selector" | "poison"
    q: torch.Tensor  # [B*Sq][>= nh*D] bf16 (a column view of a packed buffer where the case says so)
    k: torch.Tensor  # [B*S][>= nkv*D]
    v: torch.Tensor
    B: int
    S: int
    nh: int
    nkv: int
    D: int
    causal: bool
    Sq: int
    q_off: int
    chunk: bool = False  # launched with Sq / q_off (otherwise Sq == S, q_off == 0 and neither is passed)
    variants: tuple = ALL_VARIANTS
    want: Optional[torch.Tensor] = None  # selector: the exact output [B*Sq][nh*D] bf16
    rows: Optional[torch.Tensor] = None  # poison: [Sq] bool, the query rows that are checked

    @property
    def shape(self):
        return (self.B, self.S, self.nh, self.nkv, self.D, self.causal, self.Sq, self.q_off)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _packed(B, S, nh, nkv, D, seed):
    """q, k, v as column views of one packed [B*S][(nh + 2 nkv) D] buffer."""
    qkv = torch.randn(B * S, (nh + 2 * nkv) * D, generator=_gen(seed)).to(torch.bfloat16)
    return qkv[:, :nh * D], qkv[:, nh * D:(nh + nkv) * D], qkv[:, (nh + nkv) * D:]


def _chunked(B, S, Sq, nh, nkv, D, seed):
    """q [B*Sq][nh*D] of its own, k and v as column views of one packed buffer."""
    g = _gen(seed)
    kv = torch.randn(B * S, 2 * nkv * D, generator=g).to(torch.bfloat16)
    q = torch.randn(B * Sq, nh * D, generator=g).to(torch.bfloat16)
    return q, kv[:, :nkv * D], kv[:, nkv * D:]


# ---------------------------------------------------------------------------------------------
# random cases: name -> (B, S, nh, nkv, D, causal)
RANDOM_SHAPES = {
    "causal_d64_s600": (1, 600, 2, 1, 64, True),  # 10 tiles: wraps the 8-stage ring; ragged for 64 / 128 / 256
    "causal_d128_s400": (1, 400, 2, 1, 128, True),  # 7 tiles: wraps ST = 4 and 5
    "causal_d64_b2_s200": (2, 200, 4, 2, 64, True),  # the batch boundary falls inside a query block
    "causal_d128_b2_s200": (2, 200, 4, 2, 128, True),
    "full_d64_s130": (1, 130, 4, 4, 64, False),
    "full_d128_s330": (1, 330, 2, 1, 128, False),
}
# query chunks (S, Sq, q_off): the chunk ends at S; q_off odd with keys past the chunk; a chunk at
# the start; fewer than 16 queries
CHUNKS = [(600, 50, 550), (600, 100, 333), (384, 128, 0), (200, 7, 100)]
CHUNK_VARIANTS = (0, 14)


def _chunk_name(S, Sq, q_off, D, causal):
    return f"chunk_{'causal' if causal else 'full'}_d{D}_s{S}_q{Sq}_at{q_off}"


def _build_random(name):
    B, S, nh, nkv, D, causal = RANDOM_SHAPES[name]
    q, k, v = _packed(B, S, nh, nkv, D, seed=7 + list(RANDOM_SHAPES).index(name))
    return Case(name, "random", q, k, v, B, S, nh, nkv, D, causal, S, 0)


def _build_chunk(S, Sq, q_off, D, causal, seed=None):
    B, nh, nkv = 2, 4, 2
    seed = 100 + S + Sq + q_off + D + causal if seed is None else seed
    q, k, v = _chunked(B, S, Sq, nh, nkv, D, seed)
    return Case(_chunk_name(S, Sq, q_off, D, causal), "random", q, k, v, B, S, nh, nkv, D, causal, Sq, q_off,
                chunk=True, variants=CHUNK_VARIANTS)


# ---------------------------------------------------------------------------------------------
# selector cases: code[j] is a random +-1 vector per key, k = code, q[i] = 16 * code[t(i)], v random.
# Every value is exact in bf16 and every score an exact integer in fp32. The target's score is
# 16 D / sqrt(D) (128 at D = 64, 181 at D = 128); with seed 3 the largest cross-correlation is 36
# (D = 64, S = 600) and 46 (D = 128, S = 400), so the target leads every other key by at least 56
# nats and the float64 result rounds to v[t(i)] — which the builder asserts.
SELECTOR_S = {64: 600, 128: 400}
SELECTOR_SEED = 3
SELECTOR_MAPS = {
    # causal: t(i) <= i
    "diag": (True, lambda i, S: i),  # the last visible key
    "key0": (True, lambda i, S: 0 * i),
    "tile_first": (True, lambda i, S: 64 * (i // 64)),  # first key of the diagonal tile
    "tile_before": (True, lambda i, S: (64 * (i // 64) - 1).clamp_min(0)),  # last key of the tile before
    "back256": (True, lambda i, S: (i - 256).clamp_min(0)),  # across a 256-key stage
    # non-causal
    "last_key": (False, lambda i, S: 0 * i + S - 1),  # the last ragged key
    "scatter37": (False, lambda i, S: (i * 37) % S),
}


def _build_selector(mname, D):
    causal, tmap = SELECTOR_MAPS[mname]
    B, S, nh, nkv = 2, SELECTOR_S[D], 4, 2  # another code and v per (batch, KV head)
    g = _gen(SELECTOR_SEED)
    code = (2.0 * torch.randint(0, 2, (B, S, nkv, D), generator=g) - 1.0).to(torch.bfloat16)
    v = torch.randn(B, S, nkv, D, generator=g).to(torch.bfloat16)
    t = tmap(torch.arange(S), S)
    assert t.shape == (S,) and (t >= 0).all() and (t < S).all() and (not causal or (t <= torch.arange(S)).all())
    kvh = torch.arange(nh) // (nh // nkv)
    q = (16.0 * code[:, t][:, :, kvh]).to(torch.bfloat16)  # [B][S][nh][D]
    want = v[:, t][:, :, kvh].reshape(B * S, nh * D).contiguous()
    case = Case(f"select_{mname}_d{D}", "selector", q.reshape(B * S, nh * D), code.reshape(B * S, nkv * D),
                v.reshape(B * S, nkv * D), B, S, nh, nkv, D, causal, S, 0, want=want)
    check_selector(case)
    return case


def check_selector(case):
    """The case's precondition: the float64 reference rounds to the selected value row, bit for bit."""
    got = K.ref64(case.q, case.k, case.v, *case.shape).to(torch.bfloat16).reshape(case.B * case.Sq, case.nh * case.D)
    assert torch.equal(got, case.want), f"{case.name}: ref64 does not round to v[t(i)] — change SELECTOR_SEED"


# ---------------------------------------------------------------------------------------------
# poison cases: column 0 of every head is a beacon (q = 8, clean keys 0, poisoned keys 64 with
# v = 2^14 everywhere): a poisoned key that leaks scores 512 / sqrt(D) = 64 (45 at D = 128) nats
# above its clean value and replaces the row.
POISON_V = 2.0 ** 14
POISON_SHAPE = {64: (1, 600, 2, 1), 128: (1, 400, 2, 1)}  # D -> (B, S, nh, nkv), the ring-wrapping shapes


def poison_boundaries(D):
    S = POISON_SHAPE[D][1]
    return [p for p in (0, 15, 16, 31, 63, 64, 127, 128, 255, 256, 257, S - 2) if p < S]


def _beacon(q, k, v, nh, nkv, D, poisoned):
    """In place: the beacon column of every head; rows ``poisoned`` ([rows of k] bool) of k and v."""
    q[:, 0:nh * D:D] = 8.0
    k[:, 0:nkv * D:D] = 0.0
    k[poisoned, 0:nkv * D:D] = 64.0
    v[poisoned, :nkv * D] = POISON_V


def _build_poison_causal(D, p):
    B, S, nh, nkv = POISON_SHAPE[D]
    q, k, v = _packed(B, S, nh, nkv, D, seed=500 + D + p)
    _beacon(q, k, v, nh, nkv, D, torch.arange(S) > p)
    return Case(f"poison_causal_d{D}_p{p}", "poison", q, k, v, B, S, nh, nkv, D, True, S, 0,
                rows=torch.arange(S) <= p)


def _build_poison_chunk(D):
    B, S, Sq, q_off, nh, nkv = 2, 600, 100, 333, 4, 2
    q, k, v = _chunked(B, S, Sq, nh, nkv, D, seed=700 + D)
    _beacon(q, k, v, nh, nkv, D, (torch.arange(B * S) % S) >= q_off + Sq)  # keys past the chunk's last query
    return Case(f"poison_chunk_d{D}", "poison", q, k, v, B, S, nh, nkv, D, True, Sq, q_off, chunk=True,
                rows=torch.ones(Sq, dtype=torch.bool))


def _build_poison_ragged(D):
    """Non-causal S = 130: k and v are the first 130 rows of a 256-row buffer whose other rows are
    poisoned — the kernel clamps the DMA rows of the last tile to S - 1 and masks key >= S."""
    B, S, nh, nkv, rows = 1, 130, 4, 4, 256
    q, k, v = _packed(B, rows, nh, nkv, D, seed=800 + D)
    _beacon(q, k, v, nh, nkv, D, torch.arange(rows) >= S)
    return Case(f"poison_ragged_d{D}", "poison", q[:S], k[:S], v[:S], B, S, nh, nkv, D, False, S, 0,
                rows=torch.ones(S, dtype=torch.bool))


# ---------------------------------------------------------------------------------------------
_BUILDERS = {}
for _n in RANDOM_SHAPES:
    _BUILDERS[_n] = functools.partial(_build_random, _n)
for _c in CHUNKS:
    for _D in (64, 128):
        for _causal in (True, False):
            _BUILDERS[_chunk_name(*_c, _D, _causal)] = functools.partial(_build_chunk, *_c, _D, _causal)
RANDOM_CASES = tuple(_BUILDERS)  # random and query-chunk cases: per-row check, the source of ROW_TOL
for _m in SELECTOR_MAPS:
    for _D in (64, 128):
        _BUILDERS[f"select_{_m}_d{_D}"] = functools.partial(_build_selector, _m, _D)
SELECTOR_CASES = tuple(n for n in _BUILDERS if n.startswith("select_"))
for _D in (64, 128):
    for _p in poison_boundaries(_D):
        _BUILDERS[f"poison_causal_d{_D}_p{_p}"] = functools.partial(_build_poison_causal, _D, _p)
    _BUILDERS[f"poison_chunk_d{_D}"] = functools.partial(_build_poison_chunk, _D)
    _BUILDERS[f"poison_ragged_d{_D}"] = functools.partial(_build_poison_ragged, _D)
POISON_CASES = tuple(n for n in _BUILDERS if n.startswith("poison_"))


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of that name, built once per process; its tensors are shared and stay unchanged."""
    return _BUILDERS[name]()


def case_variants(names):
    """(name, variant) pairs for parametrised tests, without building any case."""
    out = []
    for n in names:
        vs = CHUNK_VARIANTS if n.startswith("chunk_") else ALL_VARIANTS
        out += [(n, v) for v in vs]
    return out


# ---------------------------------------------------------------------------------------------
# layout and ticket cases
OUT_SENTINEL = -77.0  # no output of the guarded case equals it
GUARD_ROWS, GUARD_COLS = 3, 32  # guard rows above and below the output view, guard columns left and right


@functools.lru_cache(maxsize=None)
def guard_case(D):
    """Sq = 50 with B = 2: every query block holds padded rows, and batch 1's rows follow batch 0's
    padded ones directly."""
    return dataclasses.replace(_build_chunk(200, 50, 100, D, True, seed=900 + D), name=f"guard_d{D}")


TWICE_KINDS = ("whole", "chunk")  # causal S = 600, and the query chunk (600, 100, 333)
WRAP_SHAPE = (1, 200, 2, 1)  # (B, S, nh, nkv): seven query tiles of up to two key chunks


@functools.lru_cache(maxsize=None)
def twice_cases(kind, D):
    """Two different inputs of one shape, for two launches of variant 14 back to back."""
    out = []
    for n, seed in enumerate((9000 + D, 9500 + D)):
        if kind == "chunk":
            c = _build_chunk(600, 100, 333, D, True, seed=seed)
        elif kind == "whole":
            c = Case("", "random", *_packed(1, 600, 2, 1, D, seed), 1, 600, 2, 1, D, True, 600, 0)
        else:
            c = Case("", "random", *_packed(*WRAP_SHAPE, D, seed), *WRAP_SHAPE, D, True, WRAP_SHAPE[1], 0)
        out.append(dataclasses.replace(c, name=f"twice_{kind}_d{D}_{n}", variants=(14,)))
    return tuple(out)
