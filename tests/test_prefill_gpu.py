"""Chunked prompt prefill on the GPU: ``mini-gpt2`` and ``mini-llama``, two sequences in a cache of
256 positions, chunk steps of 48 tokens up to the ragged targets [200, 9] — eagerly, then with the
token step and the chunk step as TWO captured hipGraphs replayed under torch's sync debug mode —
with bf16 and fp8 caches, followed by token steps checked at each sequence's own position
(prefill_checks.py), and generation after a chunked prefill against the sampling oracle.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import generate_checks as G  # noqa: E402
import prefill_checks as P  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, CAP, TC = 2, 256, 48
TARGETS = [200, 9]
MODELS = ["mini-gpt2", "mini-llama"]
sync = torch.cuda.synchronize


def _plan(model, **kw):
    return runtime.plan(model, world=1, seq=1, batch=B, kv_cache=CAP, prefill_chunk=TC, **kw)


def _stream(vocab, seed):
    return torch.randint(0, vocab, (B, CAP), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


def _no_sync(fn):
    """fn() under torch's sync debug mode: any synchronising call inside raises."""
    def call(*a):
        torch.cuda.set_sync_debug_mode("error")
        try:
            return fn(*a)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return call


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("model", MODELS)
def test_eager(model, kv_dtype):
    p = _plan(model, kv_dtype=kv_dtype)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=False, autotune=False)
    tokens = _stream(p.cfg.vocab_size, 3)
    ex.set_tokens("@tokens", tokens)
    P.poison_caches(ex)
    assert ex.prefill(TARGETS) == 5 and ex.kv_lengths() == TARGETS
    P.check_token_steps(p, ex, store, tokens, 4, kv_dtype, sync=sync, what="eager")


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("model", MODELS)
def test_captured(model, kv_dtype):
    p = _plan(model, kv_dtype=kv_dtype)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    tokens = _stream(p.cfg.vocab_size, 4)
    ex.set_tokens("@tokens", tokens)
    P.poison_caches(ex)
    assert ex.prefill([TC, 9]) == 1  # the first chunk step, eager: it derives the weights and may synchronise
    assert ex.capture() and not ex._segments
    graphs = (ex._graph, ex._chunk_graph)
    assert all(g is not None for g in graphs) and ex.launches > 0 and ex.chunk_launches > 0
    sync()
    assert ex.kv_lengths() == [TC, 9]  # the captures' warm-up steps left no trace
    assert ex._kv[""]["pos"].tolist() == [TC, 9]
    prefill, step = _no_sync(ex.prefill), _no_sync(ex.step)
    assert prefill(TARGETS) == 4 and ex.kv_lengths() == TARGETS  # four replays of the chunk graph
    P.check_token_steps(p, ex, store, tokens, 4, kv_dtype, sync=sync, step=step, what="captured")
    # kv_reset and a second run over another stream: the same two graph objects
    ex.kv_reset()
    tokens = _stream(p.cfg.vocab_size, 5)
    ex.set_tokens("@tokens", tokens)
    assert prefill(TARGETS) == 5 and ex.kv_lengths() == TARGETS
    P.check_token_steps(p, ex, store, tokens, 3, kv_dtype, sync=sync, step=step, what="captured, second run")
    assert (ex._graph, ex._chunk_graph) == graphs


@pytest.mark.parametrize("model", MODELS)
def test_generate_after_chunked_prefill(model):
    p = _plan(model, generate=True)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    g = torch.Generator().manual_seed(11)
    prompts = tuple(torch.randint(0, p.cfg.vocab_size, (n + 1,), generator=g).tolist() for n in TARGETS)
    chunks, *greedy = P.run_generate(ex, G.GREEDY, prompts=prompts, sync=sync)  # eager
    assert chunks == 5
    P.check_generate(p, store, G.GREEDY, *greedy, prompts=prompts)
    assert ex.capture() and ex._chunk_graph is not None
    ex.prefill, ex.step = _no_sync(ex.prefill), _no_sync(ex.step)
    chunks, *sampled = P.run_generate(ex, G.SAMPLING, prompts=prompts, sync=sync)
    assert chunks == 5
    P.check_generate(p, store, G.SAMPLING, *sampled, prompts=prompts)
    assert not torch.equal(sampled[2], greedy[2])
    # generate(): prefill() plus NEW token steps, one synchronisation at the end; it returns what
    # it left in the stream (a repeat of the whole run: test_generate_repeats_bit_identically)
    ex.set_prompts("@tokens", prompts)
    out = ex.generate(G.NEW)
    assert ex.prefill_steps == 5 and ex.kv_lengths() == [len(pr) - 1 + G.NEW for pr in prompts]
    stream = G.state(ex)["tokens"].cpu()
    assert out == [stream[b, len(pr):len(pr) + G.NEW].tolist() for b, pr in enumerate(prompts)]
    assert all(stream[b, :len(pr)].tolist() == list(pr) for b, pr in enumerate(prompts))
    # ... and, the run being repeatable, the oracle-accepted stream of the sampled run above
    assert out == [sampled[2][b, len(pr):len(pr) + G.NEW].tolist() for b, pr in enumerate(prompts)]

@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("model", MODELS)
def test_chunk_steps_repeat_bit_identically(model, kv_dtype):
    """The chunk steps add no unordered sum: captured prefills of the same streams leave the same
    cache bytes (and scales) below the targets, bit for bit. Their split-K GEMMs combine at most
    two K slices in the launch (wider splits go through the reduce kernel, which sums in slice
    order), and their folded norms take the row statistics in the consumer's main loop."""
    p = _plan(model, kv_dtype=kv_dtype)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    ex.set_tokens("@tokens", _stream(p.cfg.vocab_size, 8))
    assert ex.prefill([TC, 9]) == 1 and ex.capture()

    def rows():
        ex.kv_reset()
        assert ex.prefill(TARGETS) == 5
        sync()
        out = []
        for cs in ex._kv_cache.values():
            for c in cs[:2]:
                out += [c[b, :n].clone() for b, n in enumerate(TARGETS)]
            for sc in cs[2:]:
                out += [sc[b, :, :n].clone() for b, n in enumerate(TARGETS)]
        return out

    first = rows()
    for _ in range(4):
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(rows(), first))


@pytest.mark.parametrize("model", MODELS)
def test_generate_repeats_bit_identically(model):
    """A repeat with the same seed gives bit-identical streams and sampler statistics.

    Both step shapes of a plan with prefill_chunk are free of unordered sums for that: the chunk
    step's split-K GEMMs combine at most two K slices in the launch, and neither shape takes row
    statistics that producers add with float atomics (the consumer GEMM accumulates them in its main
    loop: the same launches). Measured on an MI355X (profiles/prefill_chunk/determinism.txt): with
    the hand-off still on in the token step, 5 of 40 repeats of this run differed on mini-gpt2,
    first in the fourth token step; without it every group output of every token step and the
    sampler statistics were identical in 80 of 80 repeats on both models."""
    p = _plan(model, generate=True)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    g = torch.Generator().manual_seed(11)
    prompts = tuple(torch.randint(0, p.cfg.vocab_size, (n + 1,), generator=g).tolist() for n in TARGETS)
    P.run_generate(ex, G.SAMPLING, prompts=prompts, sync=sync)  # eager: derives the weights
    assert ex.capture()
    _, *first = P.run_generate(ex, G.SAMPLING, prompts=prompts, sync=sync)
    _, *again = P.run_generate(ex, G.SAMPLING, prompts=prompts, sync=sync)
    assert torch.equal(again[2], first[2]), "the streams differ"
    assert all(torch.equal(a, b) for a, b in zip(again[1], first[1])), "the sampler statistics differ"


@pytest.mark.parametrize("model", MODELS)
def test_token_step_launches_as_without_the_option(model):
    """The captured token step of a plan with prefill_chunk has the kernel launches of the plan
    without it (its folded norms take their row statistics in the consumer GEMM: no launch more or less)."""
    counts = []
    for tc in (None, TC):
        p = runtime.plan(model, world=1, seq=1, batch=B, kv_cache=CAP, prefill_chunk=tc, generate=True)
        ex = runtime.make_executor(p, 0, DEV, runtime.make_store(p), use_graph=True, autotune=False)
        ex.step()
        assert ex.capture()
        counts.append(ex.launches)
    assert counts[0] == counts[1] > 0


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_debug_mode_guards_and_memory(kv_dtype):
    p = _plan("mini-llama", kv_dtype=kv_dtype, generate=True)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=False, debug=True, autotune=False)
    tokens = _stream(p.cfg.vocab_size, 6)
    ex.set_tokens("@tokens", tokens)
    assert ex.prefill(TARGETS) == 5
    ex.step()
    ex.check_guards()
    m = ex.memory_bytes()
    assert m["prefill"] == p.prefill_bytes[0] > 0
    assert m["kv_slab"] >= p.kv_cache_bytes[0] + p.sampler_bytes[0]
    assert p.stats["prefill_gb_per_rank"] == [p.prefill_bytes[0] / 1e9]
