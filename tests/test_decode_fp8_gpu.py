"""Decode steps with an fp8 KV cache on the GPU: incremental steps stay inside the bound of
decode_fp8_checks.py — eagerly, then as ONE captured hipGraph replayed over a growing sequence with
no device-to-host synchronisation inside a step — restarts, the capacity check, the guards and the
executor's cache bytes against the plan's. The models are the mini presets (head_dim 64).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from decode_checks import CAP, B, stream  # noqa: E402
from decode_fp8_checks import check_steps_fp8  # noqa: E402
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
def test_incremental_eager_then_one_graph(model, T):
    p = runtime.plan(model, world=1, seq=T, batch=B, kv_cache=CAP, kv_dtype="fp8")
    assert p.completed == p.total
    store = runtime.make_store(p)
    tokens = synthetic_tokens("@tokens", B * CAP, p.cfg.vocab_size).view(B, CAP)
    sync = torch.cuda.synchronize
    eager = runtime.make_executor(p, 0, DEV, store, use_graph=False, autotune=False)
    check_steps_fp8(p, eager, store, tokens, T, steps=1, sync=sync)  # (derives weights: may sync)
    check_steps_fp8(p, eager, store, tokens, T, steps=5, start=T, sync=sync, step=_no_sync_step(eager),
                    what=f"{model} T={T} eager")
    assert all(len(cs) == 4 and cs[0].dtype == torch.uint8 for cs in eager._kv_cache.values())
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    check_steps_fp8(p, ex, store, tokens, T, steps=1, sync=sync)
    assert ex.capture() and ex._graph is not None and not ex._segments
    assert ex.launches is not None and ex.launches > 0
    assert ex.kv_lengths() == [T] * B  # the capture's own warm-up steps left no trace
    graph = ex._graph
    check_steps_fp8(p, ex, store, tokens, T, steps=5, start=T, sync=sync, step=_no_sync_step(ex),
                    what=f"{model} T={T} graph")
    assert ex._graph is graph and ex.kv_lengths() == [6 * T] * B


def test_restart_capacity_guards_and_bytes():
    T = 4
    p = runtime.plan("mini-llama", world=1, seq=T, batch=B, kv_cache=CAP, kv_dtype="fp8")
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=False, debug=True, autotune=False)
    sync = torch.cuda.synchronize
    check_steps_fp8(p, ex, store, synthetic_tokens("@tokens", B * CAP, p.cfg.vocab_size).view(B, CAP), T, steps=3,
                    sync=sync)
    ex.kv_reset()
    other = stream(p.cfg.vocab_size, seed=77)
    ex.set_tokens("@tokens", other)
    check_steps_fp8(p, ex, store, other, T, steps=2, sync=sync, what="mini-llama restart")
    ex.kv_reset([CAP - T - 1, 0])
    ex.step()
    sync()
    before = ex.output("output_projection").clone()
    with pytest.raises(RuntimeError, match="past the KV cache capacity"):
        ex.step()
    sync()
    assert torch.equal(ex.output("output_projection"), before) and ex.kv_lengths() == [CAP - 1, T]
    ex.check_guards()
    assert ex.memory_bytes()["kv_cache"] == p.kv_cache_bytes[0]
    cfg = p.cfg
    assert p.kv_cache_bytes[0] == cfg.n_layer * 2 * B * CAP * cfg.kv_heads * (cfg.head_dim + 4)
    ex.kv_randomize(16, seed=1)
    ex.step()
    sync()
    assert torch.isfinite(ex.output("output_projection").float()).all() and ex.kv_lengths() == [16 + T] * B
    ex.check_guards()
