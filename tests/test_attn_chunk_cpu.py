"""The chunk-attention checks themselves, on the CPU: the CPU paths of ``ops.attention_chunk``,
``ops.kv_dequantize_rows`` and ``ops.kv_advance`` pass the cases of attn_chunk_cases.py, the model
of an honest kernel stays inside the tolerance, the poison precondition holds, and two mutants of
the kernel entry — q_off = 0, and keys bounded by C instead of pos[b]+T — FAIL the checks that
test_attn_chunk_gpu.py applies to the kernel, at the committed tolerance.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_checks as K  # noqa: E402
import attn_chunk_cases as CC  # noqa: E402
import attn_decode_fp8_cases as F  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

# the CPU path is an fp32 softmax rounded to bf16 (test_attn_decode_cpu.py): half an ulp of bf16 per
# element bounds the row's relative L2 error by 2^-8; fp32 against float64 adds a few 1e-6
REF_TOL_CPU = 2.0 ** -8 + 2.0 ** -16


def _step(c, out=None):
    kc, vc = c.k_cache.clone(), c.v_cache.clone()
    pos = torch.tensor(c.pos, dtype=torch.int32)
    ops.kv_append(c.k_new, c.v_new, kc, vc, pos, c.T)
    return ops.attention_chunk(c.q, kc, vc, pos, c.T, c.nh, c.nkv, c.D, out=out), kc, vc


@pytest.mark.parametrize("name", CC.RANDOM_CASES)
def test_cpu_path_random(name):
    c = CC.case(name)
    o, kc, vc = _step(c)
    assert o.dtype == torch.bfloat16 and tuple(o.shape) == (CC.B * c.T, c.nh * c.D)
    CC.check(o, c, REF_TOL_CPU, f"ops.attention_chunk {name}")
    want_k, want_v = CC.appended(c)
    assert torch.equal(kc, want_k) and torch.equal(vc, want_v)


@pytest.mark.parametrize("name", CC.SELECTOR_CASES[::5])  # (5 is coprime to the 2 position sets, 3 widths, 2 head dims)
def test_cpu_path_selector(name):
    c = CC.case(name)  # (its builder asserts the precondition: ref64 rounds to the selected row)
    o, _kc, _vc = _step(c)
    K.check_exact(o, c.want, name, c.T)


@pytest.mark.parametrize("name", CC.POISON_CASES[::5])  # (coprime to the 3 t0, 2 victims, 2 position sets, 3 widths)
def test_cpu_path_poison(name):
    c = CC.case(name)
    o, _kc, _vc = _step(c)
    CC.check(o, c, REF_TOL_CPU, name)


@pytest.mark.parametrize("name", CC.POISON_CASES[::7])
def test_poison_case_is_what_it_claims(name):
    """Every cache row at or past pos[b]+T is NaN in K and V, no row below it is."""
    c = CC.case(name)
    kc, vc = CC.appended(c)
    for b, p in enumerate(c.pos):
        assert kc[b, p + c.T:].isnan().all() and vc[b, p + c.T:].isnan().all() and p + c.T < CC.CAP
        assert not kc[b, :p + c.T].isnan().any() and not vc[b, :p + c.T].isnan().any()
    assert torch.isfinite(CC.C.reference(c)).all()


@pytest.mark.parametrize("name", CC.LATER_KEY_CASES[::5])
def test_cpu_path_later_keys(name):
    """NaN in the K rows of the chunk's later tokens: the rows up to t0 are right."""
    c = CC.case(name)
    victim = int(c.rows.any(dim=1).nonzero()[0])
    t0 = int(c.rows[victim].sum()) - 1
    assert c.k_new[victim * c.T + t0 + 1:(victim + 1) * c.T].isnan().all() and not c.v_new.isnan().any()
    assert not c.k_new[victim * c.T:victim * c.T + t0 + 1].isnan().any()
    o, _kc, _vc = _step(c)
    CC.check_upto(o, c, REF_TOL_CPU, name)
    assert o[victim * c.T + t0 + 1:(victim + 1) * c.T].isnan().any(), "a later row sees its NaN key"


@pytest.mark.parametrize("D", [64, 128])
def test_later_value_rows_must_be_finite(D):
    """The stated contract, pinned: a NaN V row of a later key of the chunk reaches an earlier row
    (0 x NaN), so V rows below pos[b]+T must be finite."""
    c = CC.value_row_case(D)
    o, _kc, _vc = _step(c)
    assert o[20].isnan().any()
    assert torch.isfinite(o[c.T:]).all()  # the other sequence is untouched


def test_every_row_is_poison_checked():
    seen = {}
    for name in CC.POISON_CASES:
        D, T, pname = name.split("_")[1:4]
        key = (D, T, pname)
        rows = torch.zeros(CC.B, int(T[1:]), dtype=torch.bool)
        v, t0 = int(name.split("_v")[1][0]), int(name.split("upto")[1])
        rows[v, :t0 + 1] = True
        seen[key] = seen.get(key, torch.zeros_like(rows)) | rows
    assert seen and all(v.all() for v in seen.values())


@pytest.mark.parametrize("name", CC.RANDOM_CASES[::2])  # (every position set, width, head pair and head dim)
def test_honest_kernel_model_passes(name):
    """P rounded to bf16, exact accumulation, bf16 output: inside the tolerance."""
    c = CC.case(name)
    kc, vc = CC.appended(c)
    T, nh, nkv, D = c.dims
    rows = [K.ref64(c.q[b * T:(b + 1) * T], kc[b, :p + T], vc[b, :p + T], 1, p + T, nh, nkv, D, True, Sq=T, q_off=p,
                    p_bf16=True) for b, p in enumerate(c.pos)]
    flat = torch.cat(rows).to(torch.bfloat16).reshape(CC.B * T, nh * D)
    worst = CC.check(flat, c, CC.ROW_TOL, f"honest model {name}")
    assert worst > 2.0 ** -11, "the model rounds nothing"


@pytest.mark.parametrize("D", [64, 128])
def test_overflow_rows_fit_or_are_finite(D):
    c = CC.overflow_case(D)
    o, _kc, _vc = _step(c)
    CC.check(o, c, REF_TOL_CPU, c.name, ref=CC.overflow_reference(c))


def _rejected(mutant, names):
    for name in names:
        c = CC.case(name)
        got = mutant(c)
        if got is None:
            continue
        flat = got.to(torch.bfloat16).reshape(CC.B * c.T, c.nh * c.D)
        try:
            if c.kind == "selector":
                K.check_exact(flat, c.want, f"{mutant.__name__} on {name}", c.T)
            else:
                CC.check(flat, c, CC.ROW_TOL, f"{mutant.__name__} on {name}")
        except AssertionError as e:
            return f"{name}: {e}"
    return None


def test_mutant_q_off_zero_is_rejected():
    """By the random check, by the selector check and by the poison check (pos > 0 in all of them)."""
    for names in (CC.EDGE_CASES[:2], CC.SELECTOR_CASES[:1], CC.POISON_CASES[:1]):
        how = _rejected(CC.mutant_q_off_zero, names)
        print(how)
        assert how is not None, f"no check on {names} rejects a kernel that reads q_off = 0"


def test_mutant_keys_bounded_by_capacity_is_rejected():
    """Only the NaN rows show it: its scores are masked, so the random and selector checks pass."""
    how = _rejected(CC.mutant_keys_bounded_by_capacity, CC.POISON_CASES[:1])
    print(how)
    assert how is not None and "not finite" in how
    assert _rejected(CC.mutant_keys_bounded_by_capacity, CC.EDGE_CASES[:1]) is None


# ---------------------------------------------------------------------------------------------
# fp8 caches

def _appended8(c8):
    kq, vq, ks, vs = (t.clone() for t in (c8.k_cache, c8.v_cache, c8.k_scale, c8.v_scale))
    pos = torch.tensor(c8.pos, dtype=torch.int32)
    ops.kv_append(c8.k_new, c8.v_new, kq, vq, pos, c8.T, ks, vs)
    return kq, vq, ks, vs, pos


@pytest.mark.parametrize("name", CC.RANDOM_CASES8[::5] + CC.POISON_CASES8)  # (5: every position set, width, head pair)
def test_cpu_path_fp8(name):
    c8 = CC.case8(name)
    kq, vq, ks, vs, pos = _appended8(c8)
    for q_, s_ in ((kq, ks), (vq, vs)):
        buf = torch.full(q_.shape, -55.0, dtype=torch.bfloat16)
        assert ops.kv_dequantize_rows(q_, s_, pos, c8.T, buf) is buf
        want = CC.dequantized_rows_expected(c8, q_, s_, -55.0)
        assert torch.equal(buf.view(torch.int16), want.view(torch.int16))
    o = ops.attention_chunk(c8.q, kq, vq, pos, c8.T, c8.nh, c8.nkv, c8.D, k_scale=ks, v_scale=vs)
    CC.check(o, c8.eq, REF_TOL_CPU, name)


def test_dequantize_rows_is_kv_dequantize_below_the_length():
    c8 = CC.case8(CC.RANDOM_CASES8[1])
    kq, _vq, ks, _vs, pos = _appended8(c8)
    buf = torch.zeros(kq.shape, dtype=torch.bfloat16)
    ops.kv_dequantize_rows(kq, ks, pos, c8.T, buf)
    whole = ops.kv_dequantize(kq, ks)
    for b, p in enumerate(c8.pos):
        assert torch.equal(buf[b, :p + c8.T], whole[b, :p + c8.T]) and torch.equal(whole[b], F.dequantize_cache(kq, ks)[b])


# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pos,limit,T", CC.ADVANCE_CASES)
def test_kv_advance(pos, limit, T):
    p, lim = torch.tensor(pos, dtype=torch.int32), torch.tensor(limit, dtype=torch.int32)
    ops.kv_advance(p, lim, T)
    assert p.tolist() == CC.advance_expected(pos, limit, T) and lim.tolist() == list(limit)
    # through the caller's buffer: the same result, pos written in place
    p2, tmp = torch.tensor(pos, dtype=torch.int32), torch.zeros(len(pos), dtype=torch.int32)
    ptr = p2.data_ptr()
    ops.kv_advance(p2, lim, T, tmp=tmp)
    assert p2.tolist() == p.tolist() and p2.data_ptr() == ptr and lim.tolist() == list(limit)


def test_argument_checks():
    c = CC.case(CC.RANDOM_CASES[0])
    pos = torch.tensor(c.pos, dtype=torch.int32)
    q = torch.zeros(CC.B * 1025, c.nh * c.D, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="T <= 1024"):
        ops.attention_chunk(q, c.k_cache, c.v_cache, pos, 1025, c.nh, c.nkv, c.D)
    with pytest.raises(RuntimeError, match="multiple of n_kv_head"):
        ops.attention_chunk(c.q, c.k_cache, c.v_cache, pos, c.T, 3, 2, c.D)
    with pytest.raises(RuntimeError, match="variant"):
        ops.attention_chunk(c.q, c.k_cache, c.v_cache, pos, c.T, c.nh, c.nkv, c.D, variant=5)
    with pytest.raises(RuntimeError, match="go with uint8"):
        ops.attention_chunk(c.q, c.k_cache, c.v_cache, pos, c.T, c.nh, c.nkv, c.D,
                            k_scale=torch.ones(CC.B, c.nkv, CC.CAP), v_scale=torch.ones(CC.B, c.nkv, CC.CAP))
    with pytest.raises(RuntimeError, match="int32"):
        ops.kv_advance(pos, pos.long(), 4)
    with pytest.raises(RuntimeError, match="uint8"):
        ops.kv_dequantize_rows(c.k_cache, torch.ones(CC.B, c.nkv, CC.CAP), pos, c.T, c.k_cache.clone())
