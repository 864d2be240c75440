"""The chunk attention over the KV cache (csrc/kernels/attn_chunk.hip) on the cases of
attn_chunk_cases.py: ``kv_append`` then ``attention_chunk`` — against the float64 oracle per (row,
head), selector cases bit for bit, NaN-poisoned stale rows, every configuration the launcher can
choose, bit-identity with ``ops.attention`` on the same keys, the e4m3 caches through
``kv_dequantize_rows``, and ``kv_advance``. test_attn_chunk_cpu.py shows that these checks reject
mutants. The worst row error of the random cases is printed: the source of MEASURED_ROW_ERR.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_checks as K  # noqa: E402
import attn_chunk_cases as CC  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -55.0
_worst = {"err": 0.0, "in": None}


def _note(err, name):
    if err > _worst["err"]:
        _worst.update(err=err, **{"in": name})
    print(f"largest row error so far: {_worst['err']:.4g} in {_worst['in']}")


def _step(c, variant=0, out=None):
    """The case on the device: the packed qkv buffer moves whole (q, k and v stay column views)."""
    qkv = c.q._base.to(DEV)
    nq, nk = c.nh * c.D, c.nkv * c.D
    q, k, v = qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:]
    kc, vc = c.k_cache.to(DEV), c.v_cache.to(DEV)
    pos = torch.tensor(c.pos, dtype=torch.int32, device=DEV)
    ops.kv_append(k, v, kc, vc, pos, c.T)
    o = ops.attention_chunk(q, kc, vc, pos, c.T, c.nh, c.nkv, c.D, out=out, variant=variant)
    return o, q, kc, vc


@pytest.mark.parametrize("name", CC.RANDOM_CASES)
def test_random(name):
    c = CC.case(name)
    o, _q, kc, vc = _step(c)
    _note(CC.check(o, c, CC.ROW_TOL, name), name)
    want_k, want_v = CC.appended(c)
    assert torch.equal(kc.cpu(), want_k) and torch.equal(vc.cpu(), want_v)


@pytest.mark.parametrize("variant", CC.VARIANTS)
@pytest.mark.parametrize("name", CC.EDGE_CASES)
def test_every_variant(name, variant):
    """Each (NW, ST, KS) configuration on both sides of the 128-key edge; the launcher's own choice
    is one of them."""
    c = CC.case(name)
    assert ops.attention_chunk_variant(CC.B, c.T, c.nh) in CC.VARIANTS and tuple(ops.CHUNK_VARIANTS) == CC.VARIANTS
    o, _q, _kc, _vc = _step(c, variant=variant)
    _note(CC.check(o, c, CC.ROW_TOL, f"{name} variant {variant}"), name)


@pytest.mark.parametrize("name", CC.SELECTOR_CASES)
def test_selector(name):
    """The output is the selected key's value row, bit for bit."""
    c = CC.case(name)
    o, _q, _kc, _vc = _step(c)
    K.check_exact(o, c.want, name, c.T)


@pytest.mark.parametrize("name", CC.POISON_CASES)
def test_poison(name):
    c = CC.case(name)
    o, _q, _kc, _vc = _step(c)
    CC.check(o, c, CC.ROW_TOL, name)


@pytest.mark.parametrize("name", CC.LATER_KEY_CASES)
def test_poison_later_keys(name):
    """NaN in the stale rows AND in the K rows of the chunk's later tokens: rows 0 .. t0 are right."""
    c = CC.case(name)
    o, _q, _kc, _vc = _step(c)
    CC.check_upto(o, c, CC.ROW_TOL, name)


@pytest.mark.parametrize("variant", CC.VARIANTS)
@pytest.mark.parametrize("name", ["chunklater_d64_t40_edge_v0_upto20", "chunklater_d128_t64_ragged_v1_upto0"])
def test_poison_later_keys_every_variant(name, variant):
    c = CC.case(name)
    o, _q, _kc, _vc = _step(c, variant=variant)
    CC.check_upto(o, c, CC.ROW_TOL, f"{name} variant {variant}")


@pytest.mark.parametrize("D", [64, 128])
def test_later_value_rows_must_be_finite(D):
    """The contract ``ops.attention_chunk`` states, pinned: the V row of a later key inside a loaded
    tile enters the second MFMA as 0 x v, so a NaN there reaches the earlier row that shares the
    tile; the other sequence is untouched."""
    c = CC.value_row_case(D)
    o, _q, _kc, _vc = _step(c)
    assert o[20].isnan().any() and torch.isfinite(o[c.T:]).all()


@pytest.mark.parametrize("variant", CC.VARIANTS)
@pytest.mark.parametrize("name", ["chunkpoison_d64_t17_edge_v0_upto8", "chunkpoison_d128_t40_ragged_v1_upto39"])
def test_poison_every_variant(name, variant):
    c = CC.case(name)
    o, _q, _kc, _vc = _step(c, variant=variant)
    CC.check(o, c, CC.ROW_TOL, f"{name} variant {variant}")


@pytest.mark.parametrize("name", ["chunk_d64_h4x1_t64_full", "chunk_d128_h4x2_t17_empty"])
def test_deterministic(name):
    c = CC.case(name)
    first, _q, _kc, _vc = _step(c)
    for _ in range(2):
        again, _q, _kc, _vc = _step(c)
        assert torch.equal(first, again)


@pytest.mark.parametrize("variant", CC.VARIANTS)
@pytest.mark.parametrize("name", ["chunk_d64_h4x2_t40_edge", "chunk_d128_h4x1_t17_edge", "chunk_d128_h2x2_t64_full"])
def test_bit_identical_to_attention(name, variant, monkeypatch):
    """The kernel is attn_item behind another entry: per sequence it equals ``ops.attention`` with
    Sq = T, q_off = p, S = p + T over the sequence's cache rows, for the same configuration."""
    c = CC.case(name)
    o, q, kc, vc = _step(c, variant=variant)
    monkeypatch.setattr(ops, "ATTN_VARIANT", variant)
    for b, p in enumerate(c.pos):
        S = p + c.T
        ref = ops.attention(q[b * c.T:(b + 1) * c.T], kc[b, :S], vc[b, :S], 1, S, c.nh, c.nkv, c.D, Sq=c.T, q_off=p)
        assert torch.equal(o[b * c.T:(b + 1) * c.T], ref), f"{name} variant {variant}: sequence {b} differs"


@pytest.mark.parametrize("D", [64, 128])
def test_overflow_rows_fit_or_are_finite(D):
    """A chunk that runs past C: the rows below C are right, the others finite, nothing faults."""
    c = CC.overflow_case(D)
    o, _q, _kc, _vc = _step(c)
    CC.check(o, c, CC.ROW_TOL, c.name, ref=CC.overflow_reference(c))


@pytest.mark.parametrize("D", [64, 128])
def test_strided_out_with_guards(D):
    """``out`` is a view into a wider and taller sentinel-filled buffer: nothing outside is written."""
    c = CC.case(f"chunk_d{D}_h4x2_t40_edge")
    rows, cols, gr, gc = CC.B * c.T, c.nh * D, 3, 32
    buf = torch.full((rows + 2 * gr, cols + 2 * gc), SENTINEL, dtype=torch.bfloat16, device=DEV)
    view = buf[gr:gr + rows, gc:gc + cols]
    o, _q, _kc, _vc = _step(c, out=view)
    assert o.data_ptr() == view.data_ptr() and o.stride() == view.stride()
    CC.check(view, c, CC.ROW_TOL, c.name)
    guard = buf.cpu()
    guard[gr:gr + rows, gc:gc + cols] = SENTINEL
    assert (guard == SENTINEL).all()


# ---------------------------------------------------------------------------------------------
# fp8 caches

@pytest.mark.parametrize("name", CC.RANDOM_CASES8 + CC.POISON_CASES8)
def test_fp8(name):
    """kv_dequantize_rows is ops.kv_dequantize bit for bit on the rows below pos[b]+T and leaves
    the sentinel in every other row; the chunk attention over it is held to the same oracle."""
    c8 = CC.case8(name)
    qkv = c8.k_new._base.to(DEV)
    nq, nk = c8.nh * c8.D, c8.nkv * c8.D
    q, k, v = qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:]
    kq, vq, ks, vs = (t.to(DEV) for t in (c8.k_cache, c8.v_cache, c8.k_scale, c8.v_scale))
    pos = torch.tensor(c8.pos, dtype=torch.int32, device=DEV)
    ops.kv_append(k, v, kq, vq, pos, c8.T, ks, vs)
    ws = tuple(torch.full(kq.shape, SENTINEL, dtype=torch.bfloat16, device=DEV) for _ in range(2))
    o = ops.attention_chunk(q, kq, vq, pos, c8.T, c8.nh, c8.nkv, c8.D, k_scale=ks, v_scale=vs, workspace=ws)
    for buf, q_, s_ in ((ws[0], kq, ks), (ws[1], vq, vs)):
        whole = ops.kv_dequantize(q_, s_).cpu()
        want = torch.full(whole.shape, SENTINEL, dtype=torch.bfloat16)
        for b, p in enumerate(c8.pos):
            want[b, :p + c8.T] = whole[b, :p + c8.T]
        assert torch.equal(buf.cpu().view(torch.int16), want.view(torch.int16)), f"{name}: dequantised rows"
        assert torch.equal(want.view(torch.int16),
                           CC.dequantized_rows_expected(c8, q_.cpu(), s_.cpu(), SENTINEL).view(torch.int16))
    _note(CC.check(o, c8.eq, CC.ROW_TOL, name), name)


# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pos,limit,T", CC.ADVANCE_CASES)
def test_kv_advance(pos, limit, T):
    p = torch.tensor(pos, dtype=torch.int32, device=DEV)
    lim = torch.tensor(limit, dtype=torch.int32, device=DEV)
    ops.kv_advance(p, lim, T)
    assert p.tolist() == CC.advance_expected(pos, limit, T) and lim.tolist() == list(limit)


def test_pos_is_read_on_the_device():
    """One captured launch follows pos: replayed after pos changed, it gives the new positions' rows."""
    a, b = CC.case("chunk_d64_h4x2_t40_edge"), CC.case("chunk_d64_h4x2_t40_empty")
    outs = []
    for c in (a, b):
        o, _q, _kc, _vc = _step(c)
        outs.append(o)
    qkv = a.q._base.to(DEV)
    nq, nk = a.nh * a.D, a.nkv * a.D
    q = qkv[:, :nq]
    kc, vc = CC.appended(a)
    kc, vc = kc.to(DEV), vc.to(DEV)
    pos = torch.tensor(a.pos, dtype=torch.int32, device=DEV)
    o = torch.empty_like(outs[0])
    ops.attention_chunk(q, kc, vc, pos, a.T, a.nh, a.nkv, a.D, out=o)  # (warm-up outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.attention_chunk(q, kc, vc, pos, a.T, a.nh, a.nkv, a.D, out=o)
    g.replay()
    assert torch.equal(o, outs[0])
    kb, vb = CC.appended(b)
    qkv.copy_(b.q._base)
    kc.copy_(kb)
    vc.copy_(vb)
    pos.copy_(torch.tensor(b.pos, dtype=torch.int32))
    g.replay()
    assert torch.equal(o, outs[1])


def test_unsupported_shapes_raise():
    c = CC.case(CC.RANDOM_CASES[0])
    pos = torch.tensor(c.pos, dtype=torch.int32, device=DEV)
    kc = torch.zeros(CC.B, CC.CAP, c.nkv * c.D, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="T <= 1024"):
        ops.attention_chunk(torch.zeros(CC.B * 1025, c.nh * c.D, dtype=torch.bfloat16, device=DEV), kc, kc, pos, 1025,
                            c.nh, c.nkv, c.D)
    k96 = torch.zeros(CC.B, CC.CAP, 96, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="head_dim 64 or 128"):
        ops.attention_chunk(torch.zeros(CC.B * 4, 96, dtype=torch.bfloat16, device=DEV), k96, k96, pos, 4, 1, 1, 96)
    k8 = torch.zeros(CC.B, CC.CAP, c.nkv * c.D, dtype=torch.uint8, device=DEV)
    ones = torch.ones(CC.B, c.nkv, CC.CAP, device=DEV)
    with pytest.raises(ValueError, match="workspace"):  # fp8 caches without the two bf16 buffers
        ops.attention_chunk(torch.zeros(CC.B * 4, c.nh * c.D, dtype=torch.bfloat16, device=DEV), k8, k8, pos, 4, c.nh,
                            c.nkv, c.D, k_scale=ones, v_scale=ones)
