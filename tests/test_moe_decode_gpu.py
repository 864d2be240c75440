"""MoE decode steps on the GPU: ``mini-mixtral`` (top-2, the near-tie measure of
moe_decode_checks.py) and its all-k variant (every row held), with both ``kv_dtype``s — one eager
step, then ONE captured hipGraph replayed under torch's sync debug mode. Every configuration holds
the same checks and asserts which launches of every layer's expert batch took the skinny kernel
(``ex._moe_skinny``): one sequence x T 1 = 1 token row (ops.MOE_SKINNY_MAX_ROWS), both launches — with
the fused routing, which gathers rows by ``a_rows``, and without it, on permuted rows; two sequences
(2, 8 and 32 rows) and ``DLS_MOE_SKINNY=0``, none: the grouped kernels of full steps. Then the per-expert
path of a plan without batches, a capped plan, and generation on the captured graph after ragged
prompts.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import generate_checks as G  # noqa: E402
import moe_decode_checks as M  # noqa: E402
from decode_checks import CAP, B, stream  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402
from distributed_llm_scheduler_amd.parallel import executor as exm  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# (sequences, tokens per step, steps, skinny switch, fused routing). Two sequences: 24 positions = 48
# rows at T 1 and 4, all 64 = 128 rows at T 16; one sequence: 32 positions (20 of its 32 reference
# rows are clear with stream(vocab, seed=1), computed on the CPU)
CONFIGS = {"B1-T1": (1, 1, 32, True, True), "B1-T1-unfused": (1, 1, 32, True, False), "T1": (2, 1, 24, True, True),
           "T4": (2, 4, 6, True, True), "T16": (2, 16, 4, True, True), "T4-switch-off": (2, 4, 6, False, True)}


def _launches(rows, switch):
    """What ex._moe_skinny holds for every batch of a step of ``rows`` token rows."""
    if not switch or rows > ops.MOE_SKINNY_MAX_ROWS:
        return None
    return ("gate_up", "down")


def _no_sync_step(ex):
    def step():
        torch.cuda.set_sync_debug_mode("error")
        try:
            return ex.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return step


def _model(kind, monkeypatch):
    return M.register_allk("mini-mixtral", monkeypatch.setitem) if kind == "allk" else "mini-mixtral"


def _plan(model, T, batch=B, **kw):
    p = runtime.plan(model, world=1, seq=T, batch=batch, kv_cache=CAP, moe_decode=True, **kw)
    assert p.completed == p.total
    return p


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("kind", ["allk", "top2"])
def test_steps_one_eager_then_one_graph(monkeypatch, kind, kv_dtype, config):
    nb, T, steps, switch, fused = CONFIGS[config]
    monkeypatch.setattr(exm, "MOE_SKINNY", switch)
    monkeypatch.setattr(exm, "MOE_FUSED_ROUTE", fused)
    p = _plan(_model(kind, monkeypatch), T, batch=nb, kv_dtype=kv_dtype)
    store = runtime.make_store(p)
    tokens = stream(p.cfg.vocab_size, seed=1)[:nb]
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    ex.set_tokens("@tokens", tokens)
    assert len(ex._moe_batch) == p.cfg.n_layer
    ex.step()  # (derives weights: may sync)
    assert ex.capture() and ex._graph is not None and not ex._segments
    want = _launches(nb * T, switch)
    assert sorted(ex._moe_skinny.values()) == ([want] * p.cfg.n_layer if want else [])
    if config.startswith("B1"):
        assert want == ("gate_up", "down")  # the one-row step is what runs the executor's skinny gate/up launch
    ex.kv_reset()
    check = M.check_steps_allk if kind == "allk" else M.check_steps_top2
    check(p, ex, store, tokens, T, steps, step=_no_sync_step(ex), sync=torch.cuda.synchronize, kv_dtype=kv_dtype)
    last = ex.output("output_projection").clone()
    # a second run of the same graph from the same state is bitwise equal
    ex.kv_reset()
    for _ in range(steps):
        ex.step()
    torch.cuda.synchronize()
    assert torch.equal(ex.output("output_projection"), last)


@pytest.mark.parametrize("kind", ["allk", "top2"])
def test_single_expert_nodes(monkeypatch, kind):
    """Without the per-layer batch every expert node runs alone (_moe_expert): today's kernels on
    a handful of rows."""
    monkeypatch.setattr(exm, "MOE_BATCH", False)
    monkeypatch.setattr(exm, "MOE_XBATCH", False)
    T = 4
    p = _plan(_model(kind, monkeypatch), T)
    store = runtime.make_store(p)
    tokens = stream(p.cfg.vocab_size, seed=1)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=False, autotune=False)
    ex.set_tokens("@tokens", tokens)
    assert not ex._moe_batch and not ex._xbatch
    check = M.check_steps_allk if kind == "allk" else M.check_steps_top2
    check(p, ex, store, tokens, T, 6, sync=torch.cuda.synchronize)
    assert not ex._moe_skinny


def test_capped_plan_runs_the_per_expert_path(monkeypatch):
    """A cap below parameters + activations + caches: parameters are evicted and re-filled every
    step, the batches are off, and the steps are still right."""
    T = 4
    model = _model("allk", monkeypatch)
    roomy = _plan(model, T)
    pr = roomy.programs[0]
    need = pr.param_arena_bytes + pr.act_arena_bytes + roomy.kv_cache_bytes[0]
    p = _plan(model, T, cap_gb=0.8 * need / 1e9)
    assert p.programs[0].counts().get("evict", 0) > 0
    store = runtime.make_store(p)
    tokens = stream(p.cfg.vocab_size, seed=1)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=False, debug=True, autotune=False)
    ex.set_tokens("@tokens", tokens)
    assert not ex._moe_batch
    M.check_steps_allk(p, ex, store, tokens, T, 4, sync=torch.cuda.synchronize)
    ex.check_guards()


@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_generates_on_the_captured_graph(monkeypatch, kv_dtype, nb):
    """Ragged prompts, greedy then sampled, on ONE graph: every token passes sample_cases.accept on
    the executor's own logits (generate_checks.check), which are held to the reference as well —
    on the all-k variant, where that holds for every row. One sequence generates on the skinny
    kernel, two on the grouped kernels."""
    prompts = G.PROMPTS[:nb]
    p = _plan(_model("allk", monkeypatch), 1, batch=nb, kv_dtype=kv_dtype, generate=True)
    store = runtime.make_store(p)
    sync = torch.cuda.synchronize
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    greedy = G.run(ex, G.GREEDY, prompts=prompts, step=_no_sync_step(ex), sync=sync, capture_after=1)
    graph = ex._graph
    want = _launches(nb, True)
    assert graph is not None and sorted(ex._moe_skinny.values()) == ([want] * p.cfg.n_layer if want else [])
    G.check(p, store, G.GREEDY, *greedy, prompts=prompts, kv_dtype=kv_dtype)
    sampled = G.run(ex, G.SAMPLING, prompts=prompts, step=_no_sync_step(ex), sync=sync)
    G.check(p, store, G.SAMPLING, *sampled, prompts=prompts, kv_dtype=kv_dtype)
    assert ex._graph is graph
    ex.set_sampling(**G.SAMPLING)
    ex.set_prompts("@tokens", prompts)
    out = ex.generate(G.NEW)
    assert out == [sampled[2][b, len(pr):len(pr) + G.NEW].tolist() for b, pr in enumerate(prompts)]


def test_top2_generation_tokens_are_accepted():
    """Top-2 routing: the tokens of the captured graph against its OWN logits of every step."""
    import sample_cases as S

    p = _plan("mini-mixtral", 1, generate=True)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    logits, stats, toks = G.run(ex, G.SAMPLING, step=_no_sync_step(ex), sync=torch.cuda.synchronize, capture_after=1)
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
    s_ = G.SAMPLING
    for b, pr in enumerate(G.PROMPTS):
        assert toks[b, :len(pr)].tolist() == list(pr)
        for s in range(len(pr) - 1, len(logits)):
            S.accept(logits[s][b].double(), f32(s_["temperature"]), s_["top_k"], f32(s_["top_p"]),
                     S.uniform(s_["seed"], 0, b, s + 1), int(toks[b, s + 1]), stats[s][b], S.EPS,
                     f"mini-mixtral sequence {b} step {s}")
