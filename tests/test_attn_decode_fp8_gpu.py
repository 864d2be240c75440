"""The fp8 KV-cache kernels (csrc/kernels/attn_decode_fp8.hip) on the cases of
attn_decode_fp8_cases.py: the quantising ``kv_append`` then ``attn_decode`` on e4m3 bytes with
chunk = 128, so the C = 640 caches span five chunks — against the float64 oracle over the
dequantised cache per (row, head), and against exact expectations: selector cases whose output is
one dequantised value row bit for bit, NaN-poisoned stale rows and scales, byte caches and scale
tensors compared whole after the append. test_attn_decode_fp8_cpu.py shows that these checks reject
mutants.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_checks as K  # noqa: E402
import attn_decode_cases as C  # noqa: E402
import attn_decode_fp8_cases as F  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _workspace(c, chunk=F.CHUNK):
    return ops.attention_decode_workspace(F.B, c.T, F.CAP, c.nh, c.nkv, c.D, DEV, chunk=chunk)


def _step(c, ws=None, out=None, chunk=F.CHUNK):
    """The case on the device: the packed qkv buffer moves whole (q, k and v stay column views)."""
    qkv = c.k_new._base.to(DEV)
    nq, nk = c.nh * c.D, c.nkv * c.D
    q, k, v = qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:]
    st = [t.to(DEV) for t in (c.k_cache, c.v_cache, c.k_scale, c.v_scale)]
    pos = torch.tensor(c.pos, dtype=torch.int32, device=DEV)
    ops.kv_append(k, v, st[0], st[1], pos, c.T, k_scale=st[2], v_scale=st[3])
    ws = _workspace(c, chunk) if ws is None else ws
    o = ops.attention_decode(q, st[0], st[1], pos, c.T, c.nh, c.nkv, c.D, out=out, workspace=ws, chunk=chunk,
                             k_scale=st[2], v_scale=st[3])
    return o, st, ws


@pytest.mark.parametrize("name", F.RANDOM_CASES)
def test_random(name):
    c = F.case(name)
    o, st, ws = _step(c)
    F.check(o, c, F.ROW_TOL, name)
    F.check_append(st, F._appended8(c), name)
    assert int(ws[1].abs().sum()) == 0, "a ticket was not reset"


@pytest.mark.parametrize("name", F.RANDOM_CASES[::2] + F.POISON_CASES[::3])
def test_with_the_launchers_chunk(name):
    """chunk = 0: the launcher's own KC (one 640-key chunk per KV head here: no merge). With
    chunk = 128 a chunk is at most one stage; here it is up to five (D = 128) or two and a half
    (D = 64, a ragged last stage), which is what exercises the ring of stage buffers."""
    c = F.case(name)
    o, _st, _ws = _step(c, chunk=0)
    F.check(o, c, F.ROW_TOL, f"{name} chunk 0")


@pytest.mark.parametrize("name", F.SELECTOR_CASES)
def test_selector(name):
    """The output is the selected key's dequantised value row, bit for bit."""
    c = F.case(name)
    o, _st, _ws = _step(c)
    K.check_exact(o, c.want, name, c.T)


@pytest.mark.parametrize("name", F.POISON_CASES)
def test_poison(name):
    c = F.case(name)
    o, _st, _ws = _step(c)
    F.check(o, c, F.ROW_TOL, name)


@pytest.mark.parametrize("pos", F.APPEND_POS)
@pytest.mark.parametrize("T", [1, 4, 16])
@pytest.mark.parametrize("nkv,D", [(1, 64), (2, 128), (3, 64)])
def test_append_is_exact(nkv, D, T, pos):
    """Whole byte caches and whole scale tensors after an append into sentinel-filled ones, against
    the test-local quantiser: bytes up to the sign of a zero, scales bit for bit; rows at or past C
    write neither bytes nor a scale (index C of a head's scales is index 0 of the next head's)."""
    E = nkv * D
    new, kc, vc, ks, vs = F.append_inputs(nkv, D, T, seed=5 + T + E)
    want = F.append_expected(new[:, E:2 * E], new[:, 2 * E:], kc, vc, ks, vs, pos, T)
    nd = new.to(DEV)
    got = [t.to(DEV) for t in (kc, vc, ks, vs)]
    ops.kv_append(nd[:, E:2 * E], nd[:, 2 * E:], got[0], got[1], torch.tensor(pos, dtype=torch.int32, device=DEV), T,
                  k_scale=got[2], v_scale=got[3])
    F.check_append(got, want, f"append nkv {nkv} D {D} T {T} at {pos}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("T", [1, 16])
def test_twice_on_one_workspace(D, T):
    """Two launches on one workspace, different inputs, the second with fewer active chunks: the
    tickets are reset and the first launch's stale partials are not merged."""
    a, b = F.twice_cases(D, T)
    ws = _workspace(a)
    oa, _st, _ws = _step(a, ws=ws)
    ob, _st, _ws = _step(b, ws=ws)
    F.check(oa, a, F.ROW_TOL, a.name)
    F.check(ob, b, F.ROW_TOL, b.name)
    assert not torch.equal(oa, ob) and int(ws[1].abs().sum()) == 0


@pytest.mark.parametrize("name", ["f8dec_d64_h4x1_t16_full", "f8dec_d128_h4x2_t4_empty"])
def test_deterministic(name):
    """The merge reads every chunk in chunk order: the same launch twice is bit-identical."""
    c = F.case(name)
    ws = _workspace(c)
    first, _st, _ws = _step(c, ws=ws)
    for _ in range(3):
        again, _st, _ws = _step(c, ws=ws)
        assert torch.equal(first, again)


@pytest.mark.parametrize("D", [64, 128])
def test_strided_out_with_guards(D):
    """``out`` is a view into a wider and taller sentinel-filled buffer: the rows are right and
    nothing outside the view is written — not by the padded columns of a column group either."""
    c = F.guard_case(D)
    rows, cols = F.B * c.T, c.nh * D
    buf = torch.full((rows + 2 * C.GUARD_ROWS, cols + 2 * C.GUARD_COLS), C.OUT_SENTINEL, dtype=torch.bfloat16,
                     device=DEV)
    view = buf[C.GUARD_ROWS:C.GUARD_ROWS + rows, C.GUARD_COLS:C.GUARD_COLS + cols]
    o, _st, _ws = _step(c, out=view)
    assert o.data_ptr() == view.data_ptr() and o.stride() == view.stride()
    F.check(view, c, F.ROW_TOL, c.name)
    guard = buf.cpu()
    assert (guard[C.GUARD_ROWS:C.GUARD_ROWS + rows, C.GUARD_COLS:C.GUARD_COLS + cols] != C.OUT_SENTINEL).all()
    guard[C.GUARD_ROWS:C.GUARD_ROWS + rows, C.GUARD_COLS:C.GUARD_COLS + cols] = C.OUT_SENTINEL
    assert (guard == C.OUT_SENTINEL).all(), \
        f"written outside the output view at (row, column) {(guard != C.OUT_SENTINEL).nonzero()[:4].tolist()}"


def test_error_paths():
    c = F.case(F.RANDOM_CASES[0])
    pos = torch.tensor(c.pos, dtype=torch.int32, device=DEV)
    kc = torch.zeros(F.B, F.CAP, c.D, dtype=torch.uint8, device=DEV)
    ks = torch.ones(F.B, 1, F.CAP, device=DEV)
    ws = (torch.zeros(1 << 20, device=DEV), torch.zeros(64, dtype=torch.int32, device=DEV))
    q1 = torch.zeros(F.B, c.D, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(RuntimeError, match="need k_scale and v_scale"):
        ops.attention_decode(q1, kc, kc, pos, 1, 1, 1, c.D, workspace=ws)
    with pytest.raises(RuntimeError, match="need k_scale and v_scale"):
        ops.kv_append(q1, q1, kc, kc.clone(), pos, 1)
    bad = torch.ones(F.B, F.CAP, 1, device=DEV)
    with pytest.raises(RuntimeError, match=r"\[B\]\[n_kv_head\]\[C\]"):
        ops.attention_decode(q1, kc, kc, pos, 1, 1, 1, c.D, workspace=ws, k_scale=bad, v_scale=bad)
    with pytest.raises(RuntimeError, match=r"\[B\]\[n_kv_head\]\[C\]"):
        ops.kv_append(q1, q1, kc, kc.clone(), pos, 1, k_scale=ks[:, :, :-1].contiguous(), v_scale=ks[:, :, :-1].contiguous())
    with pytest.raises(RuntimeError, match="T <= 16"):
        ops.attention_decode(torch.zeros(F.B * 17, c.D, dtype=torch.bfloat16, device=DEV), kc, kc, pos, 17, 1, 1, c.D,
                             workspace=ws, k_scale=ks, v_scale=ks)
    with pytest.raises(RuntimeError, match="<= 64"):
        ops.attention_decode(torch.zeros(F.B * 16, 8 * c.D, dtype=torch.bfloat16, device=DEV), kc, kc, pos, 16, 8, 1,
                             c.D, workspace=ws, k_scale=ks, v_scale=ks)


def test_zz_report_worst_row_error():
    """Prints the figure MEASURED_ROW_ERR is taken from (runs last in this module)."""
    rand = {k: v for k, v in K.row_error.items() if k.startswith("f8dec_") or k.startswith("f8dectwice")}
    if rand:
        worst = max(rand, key=rand.get)
        print(f"fp8 attn_decode worst random row error {rand[worst]:.4g} in {worst}")
        assert rand[worst] <= F.ROW_TOL
