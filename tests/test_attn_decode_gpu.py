"""The KV-cache kernels (csrc/kernels/attn_decode.hip) on the cases of attn_decode_cases.py:
``kv_append`` then ``attn_decode`` with chunk = 128, so the C = 640 caches span five chunks —
against the independent float64 oracle per (row, head), and against exact expectations: selector
cases whose output is one value row bit for bit, poisoned stale rows, later tokens and the other
sequence, caches compared whole after the append. test_attn_decode_cpu.py shows that these checks
reject mutants.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_checks as K  # noqa: E402
import attn_decode_cases as C  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _workspace(c, chunk=C.CHUNK):
    return ops.attention_decode_workspace(C.B, c.T, C.CAP, c.nh, c.nkv, c.D, DEV, chunk=chunk)


def _step(c, ws=None, out=None, chunk=C.CHUNK):
    """The case on the device: the packed qkv buffer moves whole (q, k and v stay column views)."""
    qkv = c.q._base.to(DEV)
    nq, nk = c.nh * c.D, c.nkv * c.D
    q, k, v = qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:]
    kc, vc = c.k_cache.to(DEV), c.v_cache.to(DEV)
    pos = torch.tensor(c.pos, dtype=torch.int32, device=DEV)
    ops.kv_append(k, v, kc, vc, pos, c.T)
    ws = _workspace(c, chunk) if ws is None else ws
    o = ops.attention_decode(q, kc, vc, pos, c.T, c.nh, c.nkv, c.D, out=out, workspace=ws, chunk=chunk)
    return o, kc, vc, ws


@pytest.mark.parametrize("name", C.RANDOM_CASES)
def test_random(name):
    c = C.case(name)
    o, kc, vc, ws = _step(c)
    C.check(o, c, C.ROW_TOL, name)
    want_k, want_v = C.appended(c)
    assert torch.equal(kc.cpu(), want_k) and torch.equal(vc.cpu(), want_v)
    assert int(ws[1].abs().sum()) == 0, "a ticket was not reset"


@pytest.mark.parametrize("name", C.RANDOM_CASES[::5])
def test_random_with_the_launchers_chunk(name):
    """chunk = 0: the launcher's own KC (one 640-key chunk per KV head here: no merge)."""
    c = C.case(name)
    o, _kc, _vc, _ws = _step(c, chunk=0)
    C.check(o, c, C.ROW_TOL, f"{name} chunk 0")


@pytest.mark.parametrize("name", C.SELECTOR_CASES)
def test_selector(name):
    """The output is the selected key's value row, bit for bit (see test_attn_kernels_gpu.py)."""
    c = C.case(name)
    o, _kc, _vc, _ws = _step(c)
    K.check_exact(o, c.want, name, c.T)


@pytest.mark.parametrize("name", C.POISON_CASES)
def test_poison(name):
    c = C.case(name)
    o, _kc, _vc, _ws = _step(c)
    C.check(o, c, C.ROW_TOL, name)


@pytest.mark.parametrize("pos", C.APPEND_POS)
@pytest.mark.parametrize("T", [1, 4, 16])
@pytest.mark.parametrize("E", [64, 256])
def test_append_is_exact(E, T, pos):
    """Whole caches bit for bit after an append into sentinel-filled ones: the new rows where they
    belong, rows at or past C dropped, nothing else written."""
    g = torch.Generator().manual_seed(5 + T + E)
    new = torch.randn(C.B * T, 3 * E, generator=g).to(torch.bfloat16)
    kc = torch.full((C.B, C.CAP, E), C.CACHE_SENTINEL, dtype=torch.bfloat16, device=DEV)
    vc = kc.clone()
    nd = new.to(DEV)
    ops.kv_append(nd[:, E:2 * E], nd[:, 2 * E:], kc, vc, torch.tensor(pos, dtype=torch.int32, device=DEV), T)
    want_k = torch.full((C.B, C.CAP, E), C.CACHE_SENTINEL, dtype=torch.bfloat16)
    want_v = want_k.clone()
    for b, p in enumerate(pos):
        for t in range(T):
            if p + t < C.CAP:
                want_k[b, p + t], want_v[b, p + t] = new[b * T + t, E:2 * E], new[b * T + t, 2 * E:]
    assert torch.equal(kc.cpu(), want_k) and torch.equal(vc.cpu(), want_v)


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 16])
def test_twice_on_one_workspace(D, T):
    """Two launches on one workspace, different inputs, the second with fewer active chunks: the
    tickets are reset and the first launch's stale partials are not merged."""
    a, b = C.twice_cases(D, T)
    ws = _workspace(a)
    oa, _kc, _vc, _ws = _step(a, ws=ws)
    ob, _kc, _vc, _ws = _step(b, ws=ws)
    C.check(oa, a, C.ROW_TOL, a.name)
    C.check(ob, b, C.ROW_TOL, b.name)
    assert not torch.equal(oa, ob) and int(ws[1].abs().sum()) == 0


@pytest.mark.parametrize("name", ["dec_d64_h4x1_t16_full", "dec_d128_h4x2_t4_empty"])
def test_deterministic(name):
    """The merge reads every chunk in chunk order: the same launch twice is bit-identical."""
    c = C.case(name)
    ws = _workspace(c)
    first, _kc, _vc, _ws = _step(c, ws=ws)
    for _ in range(3):
        again, _kc, _vc, _ws = _step(c, ws=ws)
        assert torch.equal(first, again)


@pytest.mark.parametrize("D", [64, 128])
def test_strided_out_with_guards(D):
    """``out`` is a view into a wider and taller sentinel-filled buffer: the rows are right and
    nothing outside the view is written — not by the padded columns of a column group either."""
    c = C.guard_case(D)
    rows, cols = C.B * c.T, c.nh * D
    buf = torch.full((rows + 2 * C.GUARD_ROWS, cols + 2 * C.GUARD_COLS), C.OUT_SENTINEL, dtype=torch.bfloat16,
                     device=DEV)
    view = buf[C.GUARD_ROWS:C.GUARD_ROWS + rows, C.GUARD_COLS:C.GUARD_COLS + cols]
    o, _kc, _vc, _ws = _step(c, out=view)
    assert o.data_ptr() == view.data_ptr() and o.stride() == view.stride()
    C.check(view, c, C.ROW_TOL, c.name)
    guard = buf.cpu()
    assert (guard[C.GUARD_ROWS:C.GUARD_ROWS + rows, C.GUARD_COLS:C.GUARD_COLS + cols] != C.OUT_SENTINEL).all()
    guard[C.GUARD_ROWS:C.GUARD_ROWS + rows, C.GUARD_COLS:C.GUARD_COLS + cols] = C.OUT_SENTINEL
    assert (guard == C.OUT_SENTINEL).all(), \
        f"written outside the output view at (row, column) {(guard != C.OUT_SENTINEL).nonzero()[:4].tolist()}"


def test_prologue_gathers_tokens_and_tables():
    T, H, D = 4, 768, 128
    pos = torch.tensor([0, C.CAP - 2], dtype=torch.int32)  # the second runs past C: clamped to the last row
    g = torch.Generator().manual_seed(2)
    tokens = torch.randint(0, 50000, (C.B, C.CAP), generator=g, dtype=torch.int32)
    wpe = torch.randn(C.CAP, H, generator=g).to(torch.bfloat16)
    cos, sin = ops.rope_tables(C.CAP, D, 10000.0)
    p = [min(int(pos[b]) + t, C.CAP - 1) for b in range(C.B) for t in range(T)]
    tok = torch.zeros(C.B * T, dtype=torch.int32, device=DEV)
    out = torch.zeros(C.B * T, H, dtype=torch.bfloat16, device=DEV)
    ops.decode_prologue(pos.to(DEV), T, C.CAP, tokens.to(DEV), tok, [wpe.to(DEV)], [out])
    assert tok.cpu().tolist() == [int(tokens[i // T, q]) for i, q in enumerate(p)]
    assert torch.equal(out.cpu(), wpe[p])
    co, so = torch.zeros(C.B * T, D // 2, device=DEV), torch.zeros(C.B * T, D // 2, device=DEV)
    ops.decode_prologue(pos.to(DEV), T, C.CAP, tables=[cos.to(DEV), sin.to(DEV)], outs=[co, so])
    assert torch.equal(co.cpu(), cos[p]) and torch.equal(so.cpu(), sin[p])


def test_unsupported_shapes_raise():
    c = C.case(C.RANDOM_CASES[0])
    pos = torch.tensor(c.pos, dtype=torch.int32, device=DEV)
    kc = torch.zeros(C.B, C.CAP, c.D, dtype=torch.bfloat16, device=DEV)
    ws = (torch.zeros(1 << 20, device=DEV), torch.zeros(64, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="T <= 16"):
        ops.attention_decode(torch.zeros(C.B * 17, c.D, dtype=torch.bfloat16, device=DEV), kc, kc, pos, 17, 1, 1, c.D,
                             workspace=ws)
    with pytest.raises(RuntimeError, match="<= 64"):
        ops.attention_decode(torch.zeros(C.B * 16, 8 * c.D, dtype=torch.bfloat16, device=DEV), kc, kc, pos, 16, 8, 1,
                             c.D, workspace=ws)
    with pytest.raises(RuntimeError, match="partials"):
        ops.attention_decode(torch.zeros(C.B, c.D, dtype=torch.bfloat16, device=DEV), kc, kc, pos, 1, 1, 1, c.D,
                             workspace=(ws[0][:8], ws[1]), chunk=C.CHUNK)
