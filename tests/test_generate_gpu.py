"""Generating plans on the GPU: ``mini-gpt2`` and ``mini-llama``, two sequences with ragged prompts
in a cache of 64 positions, with and without an fp8 cache — eagerly, then as ONE captured hipGraph
replayed under torch's sync debug mode: the sampling launch (csrc/kernels/sample.hip) after the LM
head writes the token the next replay embeds, with no device-to-host synchronisation in a step.
The checks are those of generate_checks.py, against the executor's own logits of every step.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import generate_checks as G  # noqa: E402
from generate_checks import CAP, B  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _no_sync_step(ex):
    """ex.step() under torch's sync debug mode: any synchronising call inside the step raises."""
    def step():
        torch.cuda.set_sync_debug_mode("error")
        try:
            return ex.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return step


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("model", ["mini-gpt2", "mini-llama"])
def test_generates_eager_then_as_one_graph(model, kv_dtype):
    p = runtime.plan(model, world=1, seq=1, batch=B, kv_cache=CAP, kv_dtype=kv_dtype, generate=True)
    assert p.completed == p.total
    store = runtime.make_store(p)
    sync = torch.cuda.synchronize
    eager = runtime.make_executor(p, 0, DEV, store, use_graph=False, autotune=False)
    for sampling in (G.GREEDY, G.SAMPLING):
        G.check(p, store, sampling, *G.run(eager, sampling, step=_no_sync_step(eager), sync=sync), kv_dtype=kv_dtype)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    greedy = G.run(ex, G.GREEDY, step=_no_sync_step(ex), sync=sync, capture_after=1)
    graph = ex._graph
    assert graph is not None and ex.launches is not None and ex.launches > 0
    G.check(p, store, G.GREEDY, *greedy, kv_dtype=kv_dtype)
    # new parameters are device writes: the same graph samples, from step 0 on
    sampled = G.run(ex, G.SAMPLING, step=_no_sync_step(ex), sync=sync)
    G.check(p, store, G.SAMPLING, *sampled, kv_dtype=kv_dtype)
    assert ex._graph is graph and not torch.equal(sampled[2], greedy[2])
    # kv_reset (set_prompts) and the same seed: the same stream, bit-identical statistics
    again = G.run(ex, G.SAMPLING, step=_no_sync_step(ex), sync=sync)
    assert torch.equal(again[2], sampled[2]) and all(torch.equal(a, b) for a, b in zip(again[1], sampled[1]))
    other = G.run(ex, dict(G.SAMPLING, seed=8), step=_no_sync_step(ex), sync=sync)
    assert ex._graph is graph and not torch.equal(other[2], sampled[2])
    # generate(): the same steps, one synchronisation at the end
    ex.set_sampling(**G.SAMPLING)
    ex.set_prompts("@tokens", G.PROMPTS)
    out = ex.generate(G.NEW)
    assert out == [sampled[2][b, len(pr):len(pr) + G.NEW].tolist() for b, pr in enumerate(G.PROMPTS)]


def test_guards_capacity_and_eos():
    p = runtime.plan("mini-llama", world=1, seq=1, batch=B, kv_cache=CAP, generate=True)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=False, debug=True, autotune=False)
    run = G.run(ex, G.SAMPLING, sync=torch.cuda.synchronize)
    G.check(p, store, G.SAMPLING, *run)
    ex.check_guards()
    assert ex.memory_bytes()["kv_slab"] >= p.kv_cache_bytes[0] + p.sampler_bytes[0]
    ex.set_prompts("@tokens", G.PROMPTS)
    before = G.state(ex)["tokens"].clone()
    with pytest.raises(RuntimeError, match="do not fit the KV cache capacity"):
        ex.generate(CAP - 6)
    torch.cuda.synchronize()
    assert ex.kv_lengths() == [0] * B and torch.equal(G.state(ex)["tokens"], before)
    first = ex.generate(G.NEW)
    eos = first[0][1]
    ex.set_sampling(**dict(G.SAMPLING, eos=eos))
    ex.set_prompts("@tokens", G.PROMPTS)
    out = ex.generate(G.NEW)
    cut = first[0].index(eos)
    assert out[0] == first[0][:cut + 1] + [eos] * (G.NEW - cut - 1)
    ex.check_guards()
