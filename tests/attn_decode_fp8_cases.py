"""Inputs, oracle and mutants shared by the CPU and GPU tests of the fp8 KV cache
(test_attn_decode_fp8_cpu.py, test_attn_decode_fp8_gpu.py), built on the CPU from fixed seeds, once
per process, on the geometry of attn_decode_cases.py (B = 2, C = 640, chunk = 128: five chunks).

Format under test: K and V bytes uint8 [B][C][nkv*D] (OCP e4m3), scales fp32 [B][nkv][C], one per
(position, KV head): the smallest power of two with amax / scale <= 448 over the head's D values of
the bf16 row (an all-zero row: 1), q = rne(x / scale). ``quantize_rows`` below is this module's own
implementation of that rule; nothing here goes through ``ops``.

Random N(0,1) rows nearly all get the scale 2^-7, so a kernel that took a neighbouring key's scale,
or the K scale for V, would pass on them. Every (position, head) row — cache rows and the step's new
rows alike — is therefore multiplied by a power of two drawn per row: K rows by 2^-3 .. 2^2, V rows
by 2^-6 .. 2^6, independently.

Oracle: a dequantised cache row is exactly a bf16 row, so every fp8 case has an EQUIVALENT bf16 case
(``Case8.eq``: an attn_decode_cases.Case whose caches are the dequantised ones and whose new rows
are the quantise-dequantised new rows). ``attn_checks.ref64`` over that case — through
attn_decode_cases.reference / check — sees exactly what the kernel multiplies: quantisation error
is not part of the tolerance.

Three kinds, as there: random (per (row, head) against ref64), selector (the output is the selected
key's dequantised value row bit for bit) and poison (stale rows hold byte 0x7F, the e4m3 NaN, and
NaN / +inf scales; the other sequence and the step's later tokens hold beacon rows that replace the
output if they leak).
"""
import dataclasses
import functools
import math

import torch

import attn_cases as AC
import attn_checks as K
import attn_decode_cases as C

CAP, CHUNK, B = C.CAP, C.CHUNK, C.B

# Largest relative L2 error of one (row, head) of the fp8 attn_decode against ref64 over the
# dequantised cache, as test_attn_decode_fp8_gpu.py prints it on an MI355X; the tolerance is three
# times the figure rounded up to a power of two (the rule of attn_decode_cases.ROW_TOL), capped at
# attn_checks' 2^-6. Measured: 4.855e-3 in f8dec_d64_h4x1_t16_full (sequence 1) over the 54 random
# cases with chunk = 128, every second one with the launcher's chunk and the two-launch cases, so
# the tolerance is 2^-6 (3 x 4.855e-3 = 0.01457 < 0.015625). The figure is above the bf16 cases'
# 2.933e-3 because the V rows here span 2^-6 .. 2^6: a row's output is carried by the few keys with
# large V rows, and the bf16 rounding of their p averages over fewer terms. The kernel's arithmetic
# on a dequantised row is the bf16 kernel's.
MEASURED_ROW_ERR = 4.855e-3
MEASURED_IN = "f8dec_d64_h4x1_t16_full"
ROW_TOL = 2.0 ** math.ceil(math.log2(3 * MEASURED_ROW_ERR))
assert ROW_TOL <= 2.0 ** -6

K_EXP = (-3, 2)  # per-row powers of two, inclusive
V_EXP = (-6, 6)
NAN_BYTE = 0x7F


# ---------------------------------------------------------------------------------------------
# the format, test-local

def quantize_rows(x):
    """bf16 (or float) rows [N][D] -> (uint8 [N][D] e4m3 bytes, fp32 [N] power-of-two scales)."""
    xf = x.float()
    amax = xf.abs().amax(dim=1)
    m, ex = torch.frexp(amax)  # amax = m * 2^ex, m in [0.5, 1); 448 = 0.875 * 2^9
    e = torch.where(m <= 0.875, ex - 9, ex - 8)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    scale = torch.ldexp(torch.ones_like(amax), e)
    q = (xf / scale[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def quantize_cache(x, nkv):
    """bf16 [B][C][nkv*D] -> (uint8 of that shape, fp32 [B][nkv][C])."""
    b, c, e = x.shape
    q, s = quantize_rows(x.reshape(b * c * nkv, e // nkv))
    return q.view(b, c, e), s.view(b, c, nkv).transpose(1, 2).contiguous()


def dequantize_cache(q, scale):
    """uint8 [B][C][E], fp32 [B][nkv][C] -> bf16 [B][C][E] (exact)."""
    b, c, e = q.shape
    nkv = scale.shape[1]
    x = q.view(torch.float8_e4m3fn).float().view(b, c, nkv, e // nkv) * scale.transpose(1, 2)[..., None]
    return x.to(torch.bfloat16).view(b, c, e)


def qdq_rows(x, nkv):
    """[N][nkv*D] bf16 rows through the format and back."""
    n, e = x.shape
    q, s = quantize_rows(x.reshape(n * nkv, e // nkv))
    return (q.view(torch.float8_e4m3fn).float() * s[:, None]).to(torch.bfloat16).view(n, e)


def norm_zero(q):
    """e4m3 bytes with -0 (0x80) as +0: appends are compared up to the sign of a zero."""
    return torch.where(q == 0x80, torch.zeros_like(q), q)


def append_expected(k_new, v_new, kc, vc, ks, vs, pos, T, amax_whole_row=False, scale_at=None):
    """The caches and scales after the append, by plain indexing (rows at or past C write
    nothing). The two keywords are the append mutants of test_attn_decode_fp8_cpu.py: the amax
    over the whole row instead of per head; ``scale_at(p)``: where the scale of position p lands
    in the flat [nkv*C] run of one sequence's heads (honest: h*C + p, and not at all for p >= C)."""
    kc, vc, ks, vs = kc.clone(), vc.clone(), ks.clone(), vs.clone()
    nkv = ks.shape[1]
    E = kc.shape[2]
    for new, cache, sc in ((k_new, kc, ks), (v_new, vc, vs)):
        for b, p in enumerate(pos):
            for t in range(T):
                row = new[b * T + t, :E].reshape(nkv, E // nkv)
                if amax_whole_row:
                    _q, s1 = quantize_rows(row.reshape(1, E))
                    q = (row.float() / s1).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
                    s = s1.expand(nkv)
                else:
                    q, s = quantize_rows(row)
                if p + t < CAP:
                    cache[b, p + t] = q.reshape(E)
                    sc[b, :, p + t] = s
                elif scale_at is not None:
                    flat = sc[b].view(-1)
                    for h in range(nkv):
                        i = scale_at(h, p + t)
                        if 0 <= i < flat.numel():
                            flat[i] = s[h]
    return kc, vc, ks, vs


# ---------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True, eq=False)
class Case8:
    name: str
    kind: str
    eq: C.Case  # the equivalent bf16 case: dequantised caches, quantise-dequantised new rows
    k_new: torch.Tensor  # the step's bf16 rows as the kernel receives them (views of one packed buffer)
    v_new: torch.Tensor
    k_cache: torch.Tensor  # uint8 [B][C][nkv*D] before the step
    v_cache: torch.Tensor
    k_scale: torch.Tensor  # fp32 [B][nkv][C]
    v_scale: torch.Tensor

    q = property(lambda self: self.k_new._base[:, :self.eq.nh * self.eq.D])
    pos = property(lambda self: self.eq.pos)
    T = property(lambda self: self.eq.T)
    nh = property(lambda self: self.eq.nh)
    nkv = property(lambda self: self.eq.nkv)
    D = property(lambda self: self.eq.D)
    want = property(lambda self: self.eq.want)
    rows = property(lambda self: self.eq.rows)


def _pow2(shape, lo_hi, g):
    return torch.ldexp(torch.ones(shape), torch.randint(lo_hi[0], lo_hi[1] + 1, shape, generator=g))


def _scale_rows(x, nkv, f):
    """x [..., nkv*D] bf16 times f [..., nkv] per (row, head): exact."""
    sh = x.shape
    return (x.float().view(*sh[:-1], nkv, -1) * f[..., None]).to(torch.bfloat16).view(sh)


def _finish(base, name, kc, vc, k, v, stale_nan=False):
    """Quantise the bf16 caches, pack the step, build the equivalent bf16 case."""
    T, nh, nkv, D = base.dims
    qkv = torch.cat([base.q, k, v], dim=1).contiguous()
    q, k, v = qkv[:, :nh * D], qkv[:, nh * D:(nh + nkv) * D], qkv[:, (nh + nkv) * D:]
    kq, ks = quantize_cache(kc, nkv)
    vq, vs = quantize_cache(vc, nkv)
    if stale_nan:  # rows no query may see: the NaN byte, scales NaN (K) / +inf (V) alternating with NaN
        for b, p in enumerate(base.pos):
            kq[b, p + T:] = NAN_BYTE
            vq[b, p + T:] = NAN_BYTE
            ks[b, :, p + T:] = math.nan
            vs[b, :, p + T:] = math.inf
            vs[b, :, p + T + 1::2] = math.nan
    dk, dv = dequantize_cache(kq, ks), dequantize_cache(vq, vs)
    eq = dataclasses.replace(base, name=name, q=q, k_new=qdq_rows(k, nkv), v_new=qdq_rows(v, nkv), k_cache=dk,
                             v_cache=dv)
    return Case8(name, base.kind, eq, k, v, kq, vq, ks, vs)


def _build_random(D, nh, nkv, T, pname, seed=None, name=None, pos=None):
    base = C._build_random(D, nh, nkv, T, pname, seed=seed)
    if pos is not None:
        base = dataclasses.replace(base, pos=pos)
    g = torch.Generator().manual_seed(7000 + D + 7 * nh + 13 * nkv + 31 * T + len(pname) + (seed or 0))
    kc = _scale_rows(base.k_cache, nkv, _pow2((B, CAP, nkv), K_EXP, g))
    vc = _scale_rows(base.v_cache, nkv, _pow2((B, CAP, nkv), V_EXP, g))
    k = _scale_rows(base.k_new, nkv, _pow2((B * T, nkv), K_EXP, g))
    v = _scale_rows(base.v_new, nkv, _pow2((B * T, nkv), V_EXP, g))
    return _finish(base, name or "f8" + base.name, kc, vc, k, v)


def _build_selector(mname, D, T, pname):
    """attn_decode_cases' +-1-code construction. V rows get the per-row powers of two. A K row
    that some query selects keeps its scale (codes +-1: 2^-8); every other K row — stale ones too
    — is multiplied by 2^-3 .. 2^0, which only weakens a key that must lose, so the selected key
    still leads by tens of nats, while a kernel that takes a neighbour's K scale weakens the
    selected key itself."""
    base = C._build_selector(mname, D, T, pname)
    nh, nkv = base.nh, base.nkv
    g = torch.Generator().manual_seed(7700 + D + T + len(mname) + len(pname))
    fk_c, fk_n = _pow2((B, CAP, nkv), (-3, 0), g), _pow2((B * T, nkv), (-3, 0), g)
    for b, p in enumerate(base.pos):
        for t in range(T):
            tgt = C.SELECTOR_MAPS[mname](p, t)
            if tgt < p:
                fk_c[b, tgt] = 1.0
            else:
                fk_n[b * T + tgt - p] = 1.0
    fv_c, fv_n = _pow2((B, CAP, nkv), V_EXP, g), _pow2((B * T, nkv), V_EXP, g)
    kc, k = _scale_rows(base.k_cache, nkv, fk_c), _scale_rows(base.k_new, nkv, fk_n)
    vc, v = _scale_rows(base.v_cache, nkv, fv_c), _scale_rows(base.v_new, nkv, fv_n)
    case = _finish(base, "f8" + base.name, kc, vc, k, v)
    # the selected rows, dequantised
    akc, avc = C.appended(case.eq)
    kvh = torch.arange(nh) // (nh // nkv)
    want = torch.zeros_like(base.want)
    for b, p in enumerate(base.pos):
        for t in range(T):
            tgt = C.SELECTOR_MAPS[mname](p, t)
            want[b * T + t] = avc[b, tgt].view(nkv, D)[kvh].reshape(-1)
    case = dataclasses.replace(case, eq=dataclasses.replace(case.eq, want=want))
    C.check_selector(case.eq)  # ref64 rounds to the selected dequantised row, bit for bit
    return case


# poison: attn_decode_cases' beacon scheme on top of NaN-filled stale rows. "edge": (127, 128), the
# victim 0 at T = 1 has ONE active chunk (the direct store), every other several (the merge);
# "one": both sequences inside chunk 0.
POISON_POS = {"edge": (127, 128), "ragged": (389, 63), "one": (40, 77)}


def _build_poison(D, T, pname, victim, t0):
    base = C._build_poison(D, T, "edge", victim, t0)  # (only for the shapes and the seed's q)
    nh, nkv = base.nh, base.nkv
    pos = POISON_POS[pname]
    g = torch.Generator().manual_seed(7900 + D + 3 * T + 17 * victim + t0 + len(pname))
    q, k, v = C._packed(T, nh, nkv, D, g)
    kc = torch.randn(B, CAP, nkv * D, generator=g).to(torch.bfloat16)
    vc = torch.randn(B, CAP, nkv * D, generator=g).to(torch.bfloat16)
    kc = _scale_rows(kc, nkv, _pow2((B, CAP, nkv), K_EXP, g))
    vc = _scale_rows(vc, nkv, _pow2((B, CAP, nkv), V_EXP, g))
    k = _scale_rows(k.contiguous(), nkv, _pow2((B * T, nkv), K_EXP, g))
    v = _scale_rows(v.contiguous(), nkv, _pow2((B * T, nkv), V_EXP, g))
    q = q.contiguous()
    seq_c, seq_n, tok_n = torch.arange(B * CAP) // CAP, torch.arange(B * T) // T, torch.arange(B * T) % T
    AC._beacon(q, kc.view(B * CAP, -1), vc.view(B * CAP, -1), nh, nkv, D, seq_c != victim)
    AC._beacon(q, k, v, nh, nkv, D, (seq_n != victim) | (tok_n > t0))
    rows = torch.zeros(B, T, dtype=torch.bool)
    rows[victim, :t0 + 1] = True
    name = f"f8decpoison_d{D}_t{T}_{pname}_v{victim}_upto{t0}"
    base = dataclasses.replace(base, name=name, q=q, pos=pos, rows=rows)
    return _finish(base, name, kc, vc, k, v, stale_nan=True)


_BUILDERS = {}
for _D in (64, 128):
    for _nh, _nkv in C.HEADS:
        for _T in C.STEPS:
            for _p in C.pos_sets(_T):
                _BUILDERS["f8" + C._rname(_D, _nh, _nkv, _T, _p)] = functools.partial(_build_random, _D, _nh, _nkv, _T, _p)
RANDOM_CASES = tuple(_BUILDERS)
for _m in C.SELECTOR_MAPS:
    for _D in (64, 128):
        for _T in C.STEPS:
            for _p in C.SELECTOR_POS:
                _BUILDERS[f"f8decsel_{_m}_d{_D}_t{_T}_{_p}"] = functools.partial(_build_selector, _m, _D, _T, _p)
SELECTOR_CASES = tuple(n for n in _BUILDERS if n.startswith("f8decsel_"))
for _D in (64, 128):
    for _T in C.STEPS:
        for _p in POISON_POS:
            for _v in range(B):
                for _t0 in C.poison_t0(_T):
                    _BUILDERS[f"f8decpoison_d{_D}_t{_T}_{_p}_v{_v}_upto{_t0}"] = functools.partial(
                        _build_poison, _D, _T, _p, _v, _t0)
POISON_CASES = tuple(n for n in _BUILDERS if n.startswith("f8decpoison_"))


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of that name, built once per process; its tensors are shared and stay unchanged."""
    return _BUILDERS[name]()


def check(out, c, tol, what):
    return C.check(out, c.eq, tol, what)


def active_chunks(c, b):
    return -(-min(c.pos[b] + c.T, CAP) // CHUNK)


@functools.lru_cache(maxsize=None)
def guard_case(D):
    return _build_random(D, 4, 2, 4, "full", seed=900 + D, name=f"f8decguard_d{D}")


@functools.lru_cache(maxsize=None)
def twice_cases(D, T):
    """Two steps of one shape for two launches on one workspace: five and four active chunks, then
    two and one."""
    return (_build_random(D, 4, 1, T, "full", seed=9000 + D + T, name=f"f8dectwice_d{D}_t{T}_0", pos=(CAP - T, 389)),
            _build_random(D, 4, 1, T, "full", seed=9500 + D + T, name=f"f8dectwice_d{D}_t{T}_1", pos=(200, 5)))


# append cases: the last runs past C (two of four rows fit, then none)
APPEND_POS = C.APPEND_POS
SCALE_SENTINEL = -3.0
BYTE_SENTINEL = 0x55


def append_inputs(nkv, D, T, seed):
    """The step's rows (packed, scaled per (row, head), one head's row all zero, one element -0)
    and sentinel-filled caches and scales."""
    g = torch.Generator().manual_seed(seed)
    E = nkv * D
    new = torch.randn(B * T, 3 * E, generator=g).to(torch.bfloat16)
    new[:, E:2 * E] = _scale_rows(new[:, E:2 * E].contiguous(), nkv, _pow2((B * T, nkv), K_EXP, g))
    new[:, 2 * E:] = _scale_rows(new[:, 2 * E:].contiguous(), nkv, _pow2((B * T, nkv), V_EXP, g))
    new[0, E:E + D] = 0.0  # an all-zero head row: scale 1
    new[-1, 2 * E + 3] = -0.0
    kc = torch.full((B, CAP, E), BYTE_SENTINEL, dtype=torch.uint8)
    ks = torch.full((B, nkv, CAP), SCALE_SENTINEL)
    return new, kc, kc.clone(), ks, ks.clone()


def check_append(got, want, what):
    """(k bytes, v bytes, k scales, v scales), whole tensors: bytes up to the sign of a zero,
    scales bit for bit. The scale comparison is what catches a write into the next head's run."""
    for name, g_, w_ in zip(("k bytes", "v bytes"), got[:2], want[:2]):
        g_, w_ = norm_zero(g_.cpu()), norm_zero(w_)
        assert torch.equal(g_, w_), f"{what}: {name} differ at {(g_ != w_).nonzero()[:4].tolist()}"
    for name, g_, w_ in zip(("k scales", "v scales"), got[2:], want[2:]):
        g_ = g_.cpu()
        assert torch.equal(g_.view(torch.int32), w_.view(torch.int32)), \
            f"{what}: {name} differ at [b, head, position] {(g_.view(torch.int32) != w_.view(torch.int32)).nonzero()[:4].tolist()}"


# ---------------------------------------------------------------------------------------------
# Mutants of the attention: what a kernel with a subtly wrong scale would return — ref64 over
# caches dequantised with the wrong scale. (The append mutants are append_expected's keywords.)

def _appended8(c):
    """(k bytes, v bytes, k scales, v scales) after the honest append."""
    return append_expected(c.k_new, c.v_new, c.k_cache, c.v_cache, c.k_scale, c.v_scale, c.pos, c.T)


def _shift(s):
    """scale of key + 1 (the last key: its own)."""
    return torch.cat([s[:, :, 1:], s[:, :, -1:]], dim=2)


def mutant_out(mutant, c):
    """bf16 [B*T][nh*D]: the mutant's output for case ``c``."""
    kq, vq, ks, vs = _appended8(c)
    T, nh, nkv, D = c.eq.dims
    if mutant == "v_scale_ignored":
        vs = torch.ones_like(vs)
    elif mutant == "k_scale_for_v":
        vs = ks
    elif mutant == "scale_of_next_key":
        ks, vs = _shift(ks), _shift(vs)
    elif mutant != "stale_scale_read":
        raise KeyError(mutant)
    dk, dv = dequantize_cache(kq, ks).float(), dequantize_cache(vq, vs).float()
    out = []
    for b, p in enumerate(c.pos):
        n = min(p + T, CAP)
        o = K.ref64(c.q[b * T:(b + 1) * T], dk[b, :n], dv[b, :n], 1, n, nh, nkv, D, True, Sq=T, q_off=p)
        if mutant == "stale_scale_read" and n < CAP and n % 64:
            # the first stale key of the last wave tile enters as p * scale with p = 0: 0 * NaN
            o = o + 0.0 * vs[b, :, n].double().repeat_interleave(nh // nkv)[None, None, :, None]
        out.append(o)
    return torch.cat(out).to(torch.bfloat16).reshape(B * T, nh * D)


MUTANTS = ("v_scale_ignored", "k_scale_for_v", "scale_of_next_key", "stale_scale_read")
