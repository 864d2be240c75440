"""Decode steps with KV caches on the GPU: incremental steps equal the fp32 reference forward —
eagerly, then as ONE captured hipGraph replayed over a growing sequence with no device-to-host
synchronisation inside a step — restarts, and the capacity check. The models are the mini presets:
their head_dim is 64, one the kernels have (the tiny presets' 16 runs on the CPU backend only,
test_decode_cpu.py).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from decode_checks import CAP, B, check_steps, stream  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402
from distributed_llm_scheduler_amd.parallel.executor import synthetic_tokens  # noqa: E402

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


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("model", ["mini-gpt2", "mini-llama"])
def test_incremental_equals_full_eager_then_one_graph(model, T):
    p = runtime.plan(model, world=1, seq=T, batch=B, kv_cache=CAP)
    assert p.completed == p.total
    store = runtime.make_store(p)
    tokens = synthetic_tokens("@tokens", B * CAP, p.cfg.vocab_size).view(B, CAP)
    eager = runtime.make_executor(p, 0, DEV, store, use_graph=False, autotune=False)
    check_steps(p, eager, store, tokens, T, steps=1, sync=torch.cuda.synchronize)  # (derives weights: may sync)
    check_steps(p, eager, store, tokens, T, steps=5, start=T, sync=torch.cuda.synchronize, step=_no_sync_step(eager))
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    check_steps(p, ex, store, tokens, T, steps=1, sync=torch.cuda.synchronize)
    assert ex.capture() and ex._graph is not None and not ex._segments
    assert ex.launches is not None and ex.launches > 0
    assert ex.kv_lengths() == [T] * B  # the capture's own warm-up steps left no trace
    graph = ex._graph
    check_steps(p, ex, store, tokens, T, steps=5, start=T, sync=torch.cuda.synchronize, step=_no_sync_step(ex))
    assert ex._graph is graph and ex.kv_lengths() == [6 * T] * B


def test_restart_and_capacity():
    T = 4
    p = runtime.plan("mini-llama", world=1, seq=T, batch=B, kv_cache=CAP)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=False, debug=True, autotune=False)
    check_steps(p, ex, store, synthetic_tokens("@tokens", B * CAP, p.cfg.vocab_size).view(B, CAP), T, steps=3,
                sync=torch.cuda.synchronize)
    ex.kv_reset()
    other = stream(p.cfg.vocab_size, seed=77)
    ex.set_tokens("@tokens", other)
    check_steps(p, ex, store, other, T, steps=2, sync=torch.cuda.synchronize)
    ex.kv_reset([CAP - T - 1, 0])
    ex.step()
    torch.cuda.synchronize()
    before = ex.output("output_projection").clone()
    with pytest.raises(RuntimeError, match="past the KV cache capacity"):
        ex.step()
    torch.cuda.synchronize()
    assert torch.equal(ex.output("output_projection"), before) and ex.kv_lengths() == [CAP - 1, T]
    ex.check_guards()
    assert set(ex.memory_bytes()) >= {"kv_cache", "kv_slab"}
    assert ex.memory_bytes()["kv_cache"] == p.kv_cache_bytes[0]
