"""The fp8 KV-cache checks themselves, on the CPU: the CPU paths of ``ops.kv_append`` and
``ops.attention_decode`` with scales pass every case of attn_decode_fp8_cases.py, the test-local
quantiser agrees with the project's rule, the selector and poison preconditions hold, and mutants —
a wrong, shifted, stale or misplaced scale, an amax over the wrong extent — FAIL the checks that
test_attn_decode_fp8_gpu.py applies to the kernels, at the committed tolerance.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_checks as K  # noqa: E402
import attn_decode_cases as C  # noqa: E402
import attn_decode_fp8_cases as F  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

# as test_attn_decode_cpu.py: an fp32 softmax rounded to bf16 over exactly-dequantised rows
REF_TOL_CPU = 2.0 ** -8 + 2.0 ** -16


def _step(c, out=None):
    kc, vc, ks, vs = c.k_cache.clone(), c.v_cache.clone(), c.k_scale.clone(), c.v_scale.clone()
    pos = torch.tensor(c.pos, dtype=torch.int32)
    ops.kv_append(c.k_new, c.v_new, kc, vc, pos, c.T, k_scale=ks, v_scale=vs)
    o = ops.attention_decode(c.q, kc, vc, pos, c.T, c.nh, c.nkv, c.D, out=out, chunk=F.CHUNK, k_scale=ks, v_scale=vs)
    return o, (kc, vc, ks, vs)


def test_local_quantiser_is_the_projects_rule():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(512, 64, generator=g) * torch.ldexp(torch.ones(512, 1), torch.randint(-20, 20, (512, 1), generator=g)))
    x = x.to(torch.bfloat16)
    x[3] = 0.0
    x[5, 0] = 448.0 * 2.0 ** -3  # amax / scale == 448 exactly
    q, s = F.quantize_rows(x)
    pq, ps = ops.quantize_fp8(x)
    assert torch.equal(s, ps) and torch.equal(F.norm_zero(q), F.norm_zero(pq.view(torch.uint8)))
    assert s[3] == 1.0 and s[5] == 2.0 ** -3
    amax = x.float().abs().amax(1)
    nz = amax > 0
    assert (amax[nz] / s[nz] <= 448).all() and (amax[nz] / (s[nz] / 2) > 448).all()  # the smallest such power of two
    assert torch.equal(torch.ldexp(torch.ones_like(s), torch.log2(s).round().int()), s)


def test_dequantised_rows_are_exact_bf16():
    c = F.case(F.RANDOM_CASES[0])
    x = c.k_cache.view(torch.float8_e4m3fn).float().view(F.B, F.CAP, c.nkv, c.D) * c.k_scale.transpose(1, 2)[..., None]
    assert torch.equal(x.view(F.B, F.CAP, -1), c.eq.k_cache.float())
    assert torch.equal(ops.kv_dequantize(c.k_cache, c.k_scale), c.eq.k_cache)


def test_random_rows_carry_many_scales():
    """The point of the per-row powers of two: neighbouring keys and K / V differ in scale."""
    c = F.case(F.RANDOM_CASES[0])
    assert len(c.k_scale.unique()) >= 6 and len(c.v_scale.unique()) >= 12
    assert (c.k_scale[:, :, 1:] != c.k_scale[:, :, :-1]).float().mean() > 0.5
    assert (c.k_scale != c.v_scale).float().mean() > 0.5


@pytest.mark.parametrize("name", F.RANDOM_CASES)
def test_cpu_path_random(name):
    c = F.case(name)
    o, got = _step(c)
    assert o.dtype == torch.bfloat16 and tuple(o.shape) == (F.B * c.T, c.nh * c.D)
    F.check(o, c, REF_TOL_CPU, f"ops.attention_decode {name}")
    F.check_append(got, F._appended8(c), name)
    assert torch.equal(ops.kv_dequantize(got[0], got[2])[:, :1], C.appended(c.eq)[0][:, :1])


@pytest.mark.parametrize("name", F.SELECTOR_CASES)
def test_cpu_path_selector(name):
    c = F.case(name)
    C.check_selector(c.eq)  # the precondition, as a test
    o, _ = _step(c)
    K.check_exact(o, c.want, name, c.T)


@pytest.mark.parametrize("name", F.POISON_CASES)
def test_cpu_path_poison(name):
    c = F.case(name)
    o, _ = _step(c)
    F.check(o, c, REF_TOL_CPU, name)


def test_poison_cases_are_what_they_claim():
    one = several = 0
    for name in F.POISON_CASES:
        c = F.case(name)
        victim = int(c.rows.any(dim=1).nonzero()[0])
        for b, p in enumerate(c.pos):
            assert (c.k_cache[b, p + c.T:] == F.NAN_BYTE).all() and (c.v_cache[b, p + c.T:] == F.NAN_BYTE).all()
            assert not torch.isfinite(c.k_scale[b, :, p + c.T:]).any() and not torch.isfinite(c.v_scale[b, :, p + c.T:]).any()
            assert torch.isfinite(c.k_scale[b, :, :p]).all()
        # the other sequence's rows carry the beacon: K column 0 is 64, V is 2^14
        ob, op_ = 1 - victim, c.pos[1 - victim]
        assert (c.eq.k_cache[ob, :op_, 0] == 64.0).all() and (c.eq.v_cache[ob, :op_] == 2.0 ** 14).all()
        n = F.active_chunks(c, victim)
        one += n == 1
        several += n > 1
    assert one and several, "the direct store and the merge must both be poison-checked"


def _rejections(mutant, names):
    for name in names:
        c = F.case(name)
        flat = F.mutant_out(mutant, c)
        try:
            if c.kind == "selector":
                K.check_exact(flat, c.want, f"{mutant} on {name}", c.T)
            else:
                F.check(flat, c, F.ROW_TOL, f"{mutant} on {name}")
        except AssertionError as e:
            return {name: str(e)}
    return {}


def test_unmutated_model_passes():
    """mutant_out's form without a mutation is inside the tolerance (here: 'stale_scale_read' on
    cases whose stale scales are finite changes nothing)."""
    for name in F.RANDOM_CASES[::9]:
        F.check(F.mutant_out("stale_scale_read", F.case(name)), F.case(name), F.ROW_TOL, name)


@pytest.mark.parametrize("mutant", F.MUTANTS)
def test_attention_mutant_is_rejected(mutant):
    hits = {}
    for names in (F.RANDOM_CASES[::3], F.SELECTOR_CASES[::5], F.POISON_CASES[::4]):
        hits.update(_rejections(mutant, names))
    for name, how in hits.items():
        print(f"{mutant}: rejected by {name} — {how[:200]}")
    assert hits, f"no check rejects the mutant {mutant}"


@pytest.mark.parametrize("mutant", ["scale_written_at_index_C", "amax_over_the_whole_row"])
def test_append_mutant_is_rejected(mutant):
    """The whole-tensor comparison of the append rejects a scale written at index C of a head's run
    (index 0 of the next head's) and a scale taken over the row instead of per head."""
    nkv, D, T = 2, 64, 4
    hit = False
    for pos in F.APPEND_POS:
        new, kc, vc, ks, vs = F.append_inputs(nkv, D, T, seed=40)
        E = nkv * D
        want = F.append_expected(new[:, E:2 * E], new[:, 2 * E:], kc, vc, ks, vs, pos, T)
        kw = dict(scale_at=lambda h, p: h * F.CAP + p) if mutant == "scale_written_at_index_C" else dict(amax_whole_row=True)
        got = F.append_expected(new[:, E:2 * E], new[:, 2 * E:], kc, vc, ks, vs, pos, T, **kw)
        try:
            F.check_append(got, want, mutant)
        except AssertionError as e:
            print(f"{mutant}: rejected at pos {pos} — {str(e)[:200]}")
            hit = True
    assert hit


@pytest.mark.parametrize("pos", F.APPEND_POS)
@pytest.mark.parametrize("T", [1, 4])
def test_append_is_exact(pos, T):
    nkv, D = 2, 64
    E = nkv * D
    new, kc, vc, ks, vs = F.append_inputs(nkv, D, T, seed=5 + T)
    want = F.append_expected(new[:, E:2 * E], new[:, 2 * E:], kc, vc, ks, vs, pos, T)
    ops.kv_append(new[:, E:2 * E], new[:, 2 * E:], kc, vc, torch.tensor(pos, dtype=torch.int32), T, k_scale=ks,
                  v_scale=vs)
    F.check_append((kc, vc, ks, vs), want, f"append at {pos}")
    assert (want[2] == 1.0).any() or pos[0] >= F.CAP  # the all-zero head row: scale 1


@pytest.mark.parametrize("D", [64, 128])
def test_strided_out_with_guards(D):
    c = F.guard_case(D)
    rows, cols = F.B * c.T, c.nh * D
    buf = torch.full((rows + 2 * C.GUARD_ROWS, cols + 2 * C.GUARD_COLS), C.OUT_SENTINEL, dtype=torch.bfloat16)
    view = buf[C.GUARD_ROWS:C.GUARD_ROWS + rows, C.GUARD_COLS:C.GUARD_COLS + cols]
    o, _ = _step(c, out=view)
    assert o.data_ptr() == view.data_ptr()
    F.check(view, c, REF_TOL_CPU, c.name)
    guard = buf.clone()
    guard[C.GUARD_ROWS:C.GUARD_ROWS + rows, C.GUARD_COLS:C.GUARD_COLS + cols] = C.OUT_SENTINEL
    assert (guard == C.OUT_SENTINEL).all()


def test_error_paths():
    c = F.case(F.RANDOM_CASES[0])
    pos = torch.tensor(c.pos, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="need k_scale and v_scale"):
        ops.attention_decode(c.q, c.k_cache, c.v_cache, pos, c.T, c.nh, c.nkv, c.D)
    with pytest.raises(RuntimeError, match="need k_scale and v_scale"):
        ops.kv_append(c.k_new, c.v_new, c.k_cache.clone(), c.v_cache.clone(), pos, c.T)
    bad = c.k_scale.transpose(1, 2).contiguous()  # [B][C][nkv]
    with pytest.raises(RuntimeError, match=r"\[B\]\[n_kv_head\]\[C\]"):
        ops.attention_decode(c.q, c.k_cache, c.v_cache, pos, c.T, c.nh, c.nkv, c.D, k_scale=bad, v_scale=bad)
    with pytest.raises(RuntimeError, match="go with uint8"):
        ops.attention_decode(c.q, c.eq.k_cache, c.eq.v_cache, pos, c.T, c.nh, c.nkv, c.D, k_scale=c.k_scale,
                             v_scale=c.v_scale)
    q = torch.zeros(F.B * 17, c.nh * c.D, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="T <= 16"):
        ops.attention_decode(q, c.k_cache, c.v_cache, pos, 17, c.nh, c.nkv, c.D, k_scale=c.k_scale, v_scale=c.v_scale)
    q = torch.zeros(F.B * 16, 8 * c.D, dtype=torch.bfloat16)
    kc, ks = c.k_cache[:, :, :c.D].contiguous(), c.k_scale[:, :1].contiguous()
    with pytest.raises(RuntimeError, match="<= 64"):
        ops.attention_decode(q, kc, kc, pos, 16, 8, 1, c.D, k_scale=ks, v_scale=ks)


def test_tolerance_follows_the_rule():
    assert F.ROW_TOL == 2.0 ** math.ceil(math.log2(3 * F.MEASURED_ROW_ERR)) <= 2.0 ** -6
