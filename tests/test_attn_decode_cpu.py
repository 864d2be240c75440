"""The decode-attention checks themselves, on the CPU: the CPU paths of ``ops.kv_append``,
``ops.attention_decode`` and ``ops.decode_prologue`` pass every case of attn_decode_cases.py, the
model of an honest kernel stays inside the tolerance, the selector and poison preconditions hold,
and mutants — ref64 with a subtly wrong mask, length, chunk or head map — FAIL the checks that
test_attn_decode_gpu.py applies to the kernels, at the committed tolerance.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_cases as AC  # noqa: E402
import attn_checks as K  # noqa: E402
import attn_decode_cases as C  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

# the CPU path is an fp32 softmax rounded to bf16: half an ulp of bf16 per element bounds the
# row's relative L2 error by 2^-8; fp32 against float64 over at most 640 keys adds a few 1e-6
REF_TOL_CPU = 2.0 ** -8 + 2.0 ** -16


def _step(c, out=None):
    """append, then attend: the CPU path of ops on copies of the case's caches."""
    kc, vc = c.k_cache.clone(), c.v_cache.clone()
    pos = torch.tensor(c.pos, dtype=torch.int32)
    ops.kv_append(c.k_new, c.v_new, kc, vc, pos, c.T)
    o = ops.attention_decode(c.q, kc, vc, pos, c.T, c.nh, c.nkv, c.D, out=out, chunk=C.CHUNK)
    return o, kc, vc


@pytest.mark.parametrize("name", C.RANDOM_CASES)
def test_cpu_path_random(name):
    c = C.case(name)
    o, kc, vc = _step(c)
    assert o.dtype == torch.bfloat16 and tuple(o.shape) == (C.B * c.T, c.nh * c.D)
    C.check(o, c, REF_TOL_CPU, f"ops.attention_decode {name}")
    want_k, want_v = C.appended(c)
    assert torch.equal(kc, want_k) and torch.equal(vc, want_v)


@pytest.mark.parametrize("name", C.SELECTOR_CASES)
def test_cpu_path_selector(name):
    c = C.case(name)
    C.check_selector(c)  # the precondition, as a test
    o, _kc, _vc = _step(c)
    K.check_exact(o, c.want, name, c.T)
    # the two sequences and the two KV groups want different rows, the heads of a group the same
    w = c.want.reshape(C.B, c.T, c.nh, c.D)
    assert torch.equal(w[:, :, 0], w[:, :, 1]) and not torch.equal(w[:, :, 1], w[:, :, 2])
    assert not torch.equal(w[0], w[1])


@pytest.mark.parametrize("name", C.POISON_CASES)
def test_cpu_path_poison(name):
    c = C.case(name)
    o, _kc, _vc = _step(c)
    C.check(o, c, REF_TOL_CPU, name)


@pytest.mark.parametrize("name", C.POISON_CASES)
def test_poison_case_is_what_it_claims(name):
    """A checked row sees no poisoned key; the stale rows right after the victim's last key, its
    later new tokens and the other sequence are poisoned."""
    c = C.case(name)
    ref = C.reference(c)
    victim = int(c.rows.any(dim=1).nonzero()[0])
    t0 = int(c.rows[victim].sum()) - 1
    assert c.rows[1 - victim].sum() == 0 and ref[victim, :t0 + 1].abs().max() < 16.0 < AC.POISON_V
    kc, vc = C.appended(c)
    poisoned = (vc[:, :, 0] == AC.POISON_V) & (kc[:, :, 0] == 64.0)  # [B][C]
    p = c.pos[victim]
    assert not poisoned[victim, :p + t0 + 1].any()
    assert poisoned[victim, p + t0 + 1:].all() and poisoned[1 - victim].all()
    assert p + t0 + 1 < C.CAP


def test_every_row_is_poison_checked():
    seen = {}
    for name in C.POISON_CASES:
        c = C.case(name)
        key = (c.D, c.T, c.pos)
        seen[key] = seen.get(key, torch.zeros(C.B, c.T, dtype=torch.bool)) | c.rows
    assert seen and all(v.all() for v in seen.values())


@pytest.mark.parametrize("name", C.RANDOM_CASES)
def test_honest_kernel_model_passes(name):
    """P rounded to bf16, exact accumulation, bf16 output: inside the tolerance on every random case."""
    c = C.case(name)
    kc, vc = C.appended(c)
    T, nh, nkv, D = c.dims
    rows = [K.ref64(c.q[b * T:(b + 1) * T], kc[b, :p + T], vc[b, :p + T], 1, p + T, nh, nkv, D, True, Sq=T, q_off=p,
                    p_bf16=True) for b, p in enumerate(c.pos)]
    flat = torch.cat(rows).to(torch.bfloat16).reshape(C.B * T, nh * D)
    worst = C.check(flat, c, C.ROW_TOL, f"honest model {name}")
    assert worst > 2.0 ** -11, "the model rounds nothing"


@pytest.mark.parametrize("name", C.RANDOM_CASES[::7])
def test_hook_form_of_the_oracle_is_the_oracle(name):
    """The form the mutants are written in (whole caches, a visibility matrix, kv_batch) without a
    mutation is the per-sequence oracle."""
    c = C.case(name)
    assert torch.allclose(C.ref_hooks(c), C.reference(c), rtol=1e-12, atol=1e-14)


def _rejections(mutant, names):
    for name in names:
        c = C.case(name)
        got = C.mutant_out(mutant, c)
        if got is None:
            continue
        flat = got.to(torch.bfloat16).reshape(C.B * c.T, c.nh * c.D)
        try:
            if c.kind == "selector":
                K.check_exact(flat, c.want, f"{mutant} on {name}", c.T)
            else:
                C.check(flat, c, C.ROW_TOL, f"{mutant} on {name}")
        except AssertionError as e:
            return {name: str(e)}
    return {}


@pytest.mark.parametrize("mutant", list(C.MUTANTS))
def test_mutant_is_rejected(mutant):
    by_kind = {"random": _rejections(mutant, C.RANDOM_CASES), "selector": _rejections(mutant, C.SELECTOR_CASES),
               "poison": _rejections(mutant, C.POISON_CASES)}
    for kind, hits in by_kind.items():
        for _name, how in hits.items():
            print(f"{mutant}: rejected by the {kind} check — {how}")
    assert any(by_kind.values()), f"no check rejects the mutant {mutant}"


@pytest.mark.parametrize("pos", C.APPEND_POS)
@pytest.mark.parametrize("T", [1, 4])
def test_append_is_exact(pos, T):
    c = C.case(C.RANDOM_CASES[0])
    E = c.nkv * c.D
    g = torch.Generator().manual_seed(5 + T)
    new = torch.randn(C.B * T, 3 * E, generator=g).to(torch.bfloat16)
    kc = torch.full((C.B, C.CAP, E), C.CACHE_SENTINEL, dtype=torch.bfloat16)
    vc = kc.clone()
    ops.kv_append(new[:, E:2 * E], new[:, 2 * E:], kc, vc, torch.tensor(pos, dtype=torch.int32), T)
    want_k, want_v = torch.full_like(kc, C.CACHE_SENTINEL), torch.full_like(vc, C.CACHE_SENTINEL)
    for b, p in enumerate(pos):
        for t in range(T):
            if p + t < C.CAP:
                want_k[b, p + t], want_v[b, p + t] = new[b * T + t, E:2 * E], new[b * T + t, 2 * E:]
    assert torch.equal(kc, want_k) and torch.equal(vc, want_v)


@pytest.mark.parametrize("D", [64, 128])
def test_strided_out_with_guards(D):
    c = C.guard_case(D)
    rows, cols = C.B * c.T, c.nh * D
    buf = torch.full((rows + 2 * C.GUARD_ROWS, cols + 2 * C.GUARD_COLS), C.OUT_SENTINEL, dtype=torch.bfloat16)
    view = buf[C.GUARD_ROWS:C.GUARD_ROWS + rows, C.GUARD_COLS:C.GUARD_COLS + cols]
    o, _kc, _vc = _step(c, out=view)
    assert o.data_ptr() == view.data_ptr()
    C.check(view, c, REF_TOL_CPU, c.name)
    guard = buf.clone()
    guard[C.GUARD_ROWS:C.GUARD_ROWS + rows, C.GUARD_COLS:C.GUARD_COLS + cols] = C.OUT_SENTINEL
    assert (guard == C.OUT_SENTINEL).all()


def test_prologue_gathers_tokens_and_tables():
    T, H, D = 4, 64, 64
    pos = torch.tensor([0, C.CAP - 2], dtype=torch.int32)  # the second runs past C: clamped to the last row
    g = torch.Generator().manual_seed(2)
    tokens = torch.randint(0, 50000, (C.B, C.CAP), generator=g, dtype=torch.int32)
    wpe = torch.randn(C.CAP, H, generator=g).to(torch.bfloat16)
    cos, sin = ops.rope_tables(C.CAP, D, 10000.0)
    tok = torch.zeros(C.B * T, dtype=torch.int32)
    outs = [torch.zeros(C.B * T, H, dtype=torch.bfloat16)]
    ops.decode_prologue(pos, T, C.CAP, tokens, tok, [wpe], outs)
    p = [min(int(pos[b]) + t, C.CAP - 1) for b in range(C.B) for t in range(T)]
    assert tok.tolist() == [int(tokens[i // T, q]) for i, q in enumerate(p)]
    assert torch.equal(outs[0], wpe[p])
    co, so = torch.zeros(C.B * T, D // 2), torch.zeros(C.B * T, D // 2)
    ops.decode_prologue(pos, T, C.CAP, tables=[cos, sin], outs=[co, so])
    assert torch.equal(co, cos[p]) and torch.equal(so, sin[p])


def test_unsupported_shapes_raise():
    c = C.case(C.RANDOM_CASES[0])
    pos = torch.tensor(c.pos, dtype=torch.int32)
    q = torch.zeros(C.B * 17, c.nh * c.D, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="T <= 16"):
        ops.attention_decode(q, c.k_cache, c.v_cache, pos, 17, c.nh, c.nkv, c.D)
    q = torch.zeros(C.B * 16, 8 * c.D, dtype=torch.bfloat16)
    kc = c.k_cache[:, :, :c.D].contiguous()
    with pytest.raises(RuntimeError, match="<= 64"):
        ops.attention_decode(q, kc, kc, pos, 16, 8, 1, c.D)
