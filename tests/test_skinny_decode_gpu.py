"""Decode steps of plans with ``skinny_gemm=True`` on the GPU. ``DLS_SKINNY=all`` sends every dense
GEMM of a step of up to 16 rows to the skinny kernel, so the coverage does not depend on the two
measured constants (ops.SKINNY_MAX_ROWS, ops.SKINNY_LMHEAD): ``mini-gpt2`` and ``mini-llama``
(folded LayerNorm / RMSNorm, RoPE, SwiGLU, bias, GELU, residual), one eager step, then ONE captured
hipGraph under torch's sync debug mode, both ``kv_dtype``s, held to decode_checks' margin against
the fp32 reference, with ``ex._skinny`` saying that every dense GEMM ran skinny. Then the unfolded
path of the full-width Llama (FOLD_MAX_K lowered), the fallbacks (32 rows, ``DLS_SKINNY=0``, the
default switches), ``mini-mixtral`` with ``moe_decode``, a ``prefill_chunk`` plan, and generation."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_fp8_checks as D8  # noqa: E402
import generate_checks as G  # noqa: E402
import moe_decode_checks as M  # noqa: E402
import prefill_checks as P  # noqa: E402
from decode_checks import CAP, B, check_steps, stream  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402
from distributed_llm_scheduler_amd.parallel import executor as exm  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
sync = torch.cuda.synchronize


def _no_sync(fn):
    def call(*a):
        torch.cuda.set_sync_debug_mode("error")
        try:
            return fn(*a)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return call


def _plan(model, T, batch=B, skinny=True, **kw):
    p = runtime.plan(model, world=1, seq=T, batch=batch, kv_cache=CAP, **(dict(skinny_gemm=True) if skinny else {}), **kw)
    assert p.completed == p.total
    return p


def _dense_gemms(p):
    """(task, weight) of every dense GEMM of the plan's DAG: QKV, out-projection, the MLP pair, the LM head."""
    out = set()
    for t in p.tasks:
        k, W = t.op.kind, t.op.weights
        if k == "attention":
            out |= {(t.id, W["w_qkv"]), (t.id, W["w_o"])}
        elif k == "swiglu_mlp":
            out |= {(t.id, W["w_gate_up"]), (t.id, W["w_down"])}
        elif k in ("linear", "lm_head") and "route" not in t.id and "gate" not in t.id:
            out.add((t.id, W["w"]))
    return out


def _all_skinny(ex, p):
    ran = {k for k, v in ex._skinny.items() if v == "skinny"}
    assert ran >= _dense_gemms(p), sorted(_dense_gemms(p) - ran)
    assert set(ex._skinny.values()) == {"skinny"}, ex._skinny


def _check(p, ex, store, tokens, T, steps, kv_dtype, **kw):
    fn = D8.check_steps_fp8 if kv_dtype == "fp8" else check_steps
    fn(p, ex, store, tokens, T, steps, sync=sync, **kw)


MODELS = ("mini-gpt2", "mini-llama")
KV = ("bf16", "fp8")


def _each(fn, *cases):
    """fn(*case) for every case of one test; between cases, as conftest does between tests, the
    hipGraphs and buffers of the executors that died are destroyed (parallel/lifetime.py)."""
    from distributed_llm_scheduler_amd.parallel import lifetime

    for case in cases:
        fn(*case)
        lifetime.release()


def test_steps_one_eager_then_one_graph(monkeypatch):
    """Both models, T in {1, 4}, both kv_dtypes: eight plans in one test."""
    monkeypatch.setenv("DLS_SKINNY", "all")
    _each(_steps, *[(m, T, kv) for m in MODELS for T in (1, 4) for kv in KV])


def _steps(model, T, kv_dtype):
    p = _plan(model, T, kv_dtype=kv_dtype)
    store = runtime.make_store(p)
    tokens = stream(p.cfg.vocab_size, seed=3)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    ex.set_tokens("@tokens", tokens)
    assert not ex._stats_out and not ex._ext_stats  # no statistics hand-off in a plan with the option
    _check(p, ex, store, tokens, T, 1, kv_dtype)  # eager (derives weights: may sync)
    _all_skinny(ex, p)
    assert ex.capture() and ex._graph is not None and not ex._segments
    _check(p, ex, store, tokens, T, 5, kv_dtype, start=T, step=_no_sync(ex.step))
    _all_skinny(ex, p)
    last = ex.output("output_projection").clone()
    ex.kv_reset()  # the same graph from the same state: bit-identical (no unordered sum in the step)
    for _ in range(6):
        ex.step()
    sync()
    assert torch.equal(ex.output("output_projection"), last)


def test_unfolded_norms_as_the_full_width_llama(monkeypatch):
    """FOLD_MAX_K below the hidden size: no norm is folded, as at Llama-3-8B's K = 4096. Every
    norm is a launch in front of its GEMM, a skinny residual GEMM claims no post-norm, and the
    step has no more launches than the plan without the option (whose residual GEMM runs its
    post-norm as a second launch or in its split-K reduce)."""
    monkeypatch.setenv("DLS_SKINNY", "all")
    monkeypatch.setattr(exm, "FOLD_MAX_K", 128)
    monkeypatch.setattr(exm, "HANDOFF_MAX_K", 128)
    _each(_unfolded, (1,), (4,))


def _unfolded(T):
    launches = {}
    for skinny in (True, False):
        p = _plan("mini-llama", T, skinny=skinny)
        assert p.cfg.n_embd > 128
        store = runtime.make_store(p)
        tokens = stream(p.cfg.vocab_size, seed=4)
        ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
        ex.set_tokens("@tokens", tokens)
        check_steps(p, ex, store, tokens, T, 1, sync=sync)
        assert ex._pn_done is None or not skinny  # no skinny producer claimed a norm
        assert ex.capture()
        check_steps(p, ex, store, tokens, T, 4, start=T, sync=sync, step=_no_sync(ex.step))
        launches[skinny] = ex.launches
        if skinny:
            _all_skinny(ex, p)
        else:
            assert ex._skinny == {}
    assert 0 < launches[True] <= launches[False], launches


def test_fallbacks(monkeypatch):
    """B*T = 32 rows fall back to the tiles with the reason; DLS_SKINNY=0 runs the plain plan's
    launches; without DLS_SKINNY the dispatch obeys the two measured constants."""
    monkeypatch.setenv("DLS_SKINNY", "all")
    _each(_32_rows, ())
    monkeypatch.setenv("DLS_SKINNY", "0")
    _each(_switch_off, *[(m,) for m in MODELS])
    monkeypatch.delenv("DLS_SKINNY")
    _each(_default_switches, (1,), (2,))


def _32_rows():
    T = 16
    p = _plan("mini-llama", T)
    store = runtime.make_store(p)
    tokens = stream(p.cfg.vocab_size, seed=5)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=False, autotune=False)
    ex.set_tokens("@tokens", tokens)
    check_steps(p, ex, store, tokens, T, 3, sync=sync)
    assert set(ex._skinny) >= _dense_gemms(p)
    assert all(v.startswith("M = 32 rows") for v in ex._skinny.values()), ex._skinny


def _switch_off(model):
    launches = []
    for skinny in (True, False):
        p = _plan(model, 1, skinny=skinny)
        store = runtime.make_store(p)
        tokens = stream(p.cfg.vocab_size, seed=6)
        ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
        ex.set_tokens("@tokens", tokens)
        check_steps(p, ex, store, tokens, 1, 1, sync=sync)
        assert ex.capture() and ex._skinny == {}
        check_steps(p, ex, store, tokens, 1, 3, start=1, sync=sync)
        launches.append((ex.launches, sorted(ex._stats_out), sorted(ex._post_norm)))
    assert launches[0] == launches[1]


def _default_switches(nb):
    """Without DLS_SKINNY the dispatch obeys ops.SKINNY_MAX_ROWS and ops.SKINNY_LMHEAD."""
    p = _plan("mini-llama", 1, batch=nb)
    store = runtime.make_store(p)
    tokens = stream(p.cfg.vocab_size, seed=7)[:nb]
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=False, autotune=False)
    ex.set_tokens("@tokens", tokens)
    check_steps(p, ex, store, tokens, 1, 3, sync=sync)
    assert set(ex._skinny) >= _dense_gemms(p)
    for (task, w), v in ex._skinny.items():
        if nb > ops.SKINNY_MAX_ROWS:
            assert v.startswith(f"M = {nb} rows"), (task, w, v)
        elif ex._w(w).shape[0] >= ops.LMHEAD_MIN_N and not ops.SKINNY_LMHEAD:
            assert "SKINNY_LMHEAD" in v
        else:
            assert v == "skinny", (task, w, v)


def test_mixtral_dense_gemms_run_skinny(monkeypatch):
    """moe_decode + skinny_gemm at one token row: the expert launches on the grouped skinny kernel,
    the attention GEMMs and the LM head on the dense one; the near-tie measure of top-2 routing."""
    monkeypatch.setenv("DLS_SKINNY", "all")
    _each(_mixtral, *[(kv,) for kv in KV])


def _mixtral(kv_dtype):
    p = _plan("mini-mixtral", 1, batch=1, moe_decode=True, kv_dtype=kv_dtype)
    store = runtime.make_store(p)
    tokens = stream(p.cfg.vocab_size, seed=1)[:1]
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    ex.set_tokens("@tokens", tokens)
    ex.step()
    assert ex.capture() and ex._graph is not None
    ran = {k for k, v in ex._skinny.items() if v == "skinny"}
    want = _dense_gemms(p)  # QKV and out-projection of every layer, the LM head (the router runs fused with the routing)
    assert len(want) == 2 * p.cfg.n_layer + 1 and ran >= want, sorted(want - ran)
    assert set(ex._skinny.values()) == {"skinny"}
    assert sorted(ex._moe_skinny.values()) == [("gate_up", "down")] * p.cfg.n_layer
    ex.kv_reset()
    M.check_steps_top2(p, ex, store, tokens, 1, 32, step=_no_sync(ex.step), sync=sync, kv_dtype=kv_dtype)


def test_prefill_chunk_plan_token_steps_skinny_chunks_on_tiles(monkeypatch):
    """Chunk steps keep the tile kernels (nothing of them is recorded in ex._skinny, and the chunk
    graph exists), token steps run skinny, and a generation repeats bit for bit."""
    monkeypatch.setenv("DLS_SKINNY", "all")
    _each(_prefill_chunk, *[(m,) for m in MODELS])


def _prefill_chunk(model):
    TC, cap, targets = 48, 256, [200, 9]
    p = runtime.plan(model, world=1, seq=1, batch=B, kv_cache=cap, prefill_chunk=TC, generate=True, skinny_gemm=True)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    g = torch.Generator().manual_seed(11)
    prompts = tuple(torch.randint(0, p.cfg.vocab_size, (n + 1,), generator=g).tolist() for n in targets)
    ex.set_sampling(**G.SAMPLING)
    ex.set_prompts("@tokens", prompts)
    assert ex.prefill() == 5 and ex._skinny == {}  # chunk steps only so far: tiles
    chunks, *eager = P.run_generate(ex, G.SAMPLING, prompts=prompts, sync=sync)  # eager: derives the weights
    assert chunks == 5
    _all_skinny(ex, p)
    P.check_generate(p, store, G.SAMPLING, *eager, prompts=prompts)
    assert ex.capture() and ex._chunk_graph is not None
    _, *first = P.run_generate(ex, G.SAMPLING, prompts=prompts, sync=sync, step=_no_sync(ex.step))
    _, *again = P.run_generate(ex, G.SAMPLING, prompts=prompts, sync=sync)
    P.check_generate(p, store, G.SAMPLING, *first, prompts=prompts)
    assert torch.equal(again[2], first[2]), "the streams differ"
    assert all(torch.equal(a, b) for a, b in zip(again[0], first[0])), "the logits differ"
    assert all(torch.equal(a, b) for a, b in zip(again[1], first[1])), "the sampler statistics differ"
    _all_skinny(ex, p)


def test_generates_on_the_captured_graph(monkeypatch):
    """Ragged prompts, greedy then sampled, on ONE graph of skinny launches: every token passes
    the sampling oracle on the executor's own logits, which are held to the reference."""
    monkeypatch.setenv("DLS_SKINNY", "all")
    _each(_generates, *[(m, kv) for m in MODELS for kv in KV])


def _generates(model, kv_dtype):
    p = _plan(model, 1, kv_dtype=kv_dtype, generate=True)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    greedy = G.run(ex, G.GREEDY, step=_no_sync(ex.step), sync=sync, capture_after=1)
    graph = ex._graph
    assert graph is not None
    _all_skinny(ex, p)
    G.check(p, store, G.GREEDY, *greedy, kv_dtype=kv_dtype)
    sampled = G.run(ex, G.SAMPLING, step=_no_sync(ex.step), sync=sync)
    G.check(p, store, G.SAMPLING, *sampled, kv_dtype=kv_dtype)
    assert ex._graph is graph
    ex.set_sampling(**G.SAMPLING)
    ex.set_prompts("@tokens", G.PROMPTS)
    out = ex.generate(G.NEW)
    assert out == [sampled[2][b, len(pr):len(pr) + G.NEW].tolist() for b, pr in enumerate(G.PROMPTS)]
