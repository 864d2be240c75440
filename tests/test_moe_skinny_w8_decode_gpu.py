"""Decode steps of an fp8-experts ``mini-mixtral`` plan with ``moe_decode=True, moe_skinny_w8=True``
on the GPU, all-k variant (every row held) and top-2 (the near-tie measure of moe_decode_checks.py),
both ``kv_dtype``s: one eager step, then ONE captured hipGraph replayed under torch's sync debug
mode, against ``reference.forward`` on the same store. A step of at most
``ops.MOE_SKINNY_W8_MAX_ROWS`` token rows (one sequence x T 1; two x T 4) takes
``ops.gemm_grouped_skinny_w8`` for both launches of every layer (``ex._moe_skinny``); two sequences
x T 4 under a bound of 1, two x T 16 and ``MOE_SKINNY`` off run the grouped W8 tiles. Then the CLI."""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import moe_decode_checks as M  # noqa: E402
from decode_checks import CAP, stream  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402
from distributed_llm_scheduler_amd.parallel import executor as exm  # noqa: E402
from distributed_llm_scheduler_amd.parallel import lifetime  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# (sequences, tokens per step, steps, skinny switch, row bound or None for the measured one): 32
# positions of one sequence, 24 or all 64 of two
CONFIGS = {"B1-T1": (1, 1, 32, True, None), "B2-T4": (2, 4, 6, True, None), "B2-T4-bound-1": (2, 4, 6, True, 1),
           "B2-T16": (2, 16, 4, True, None), "B1-T1-switch-off": (1, 1, 32, False, None)}


def _no_sync_step(ex):
    def step():
        torch.cuda.set_sync_debug_mode("error")
        try:
            return ex.step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return step


@pytest.mark.parametrize("kind", ["allk", "top2"])
def test_steps_one_eager_then_one_graph(monkeypatch, kind):
    for kv_dtype in ("bf16", "fp8"):
        for config in CONFIGS:
            with monkeypatch.context() as m:
                _steps(m, kind, kv_dtype, config)
            lifetime.release()  # (as between tests: the executor's graph and buffers)


def _steps(monkeypatch, kind, kv_dtype, config):
    nb, T, steps, switch, bound = CONFIGS[config]
    monkeypatch.setattr(exm, "MOE_SKINNY", switch)
    if bound is not None:
        monkeypatch.setattr(ops, "MOE_SKINNY_W8_MAX_ROWS", bound)
    model = M.register_allk("mini-mixtral", monkeypatch.setitem) if kind == "allk" else "mini-mixtral"
    p = runtime.plan(model, world=1, seq=T, batch=nb, kv_cache=CAP, moe_decode=True, moe_skinny_w8=True,
                     weight_dtype="fp8-experts", kv_dtype=kv_dtype)
    assert p.completed == p.total
    store = runtime.make_store(p)
    tokens = stream(p.cfg.vocab_size, seed=1)[:nb]
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    ex.set_tokens("@tokens", tokens)
    assert len(ex._moe_batch) == p.cfg.n_layer
    ex.step()  # (derives weights: may sync)
    assert ex.capture() and ex._graph is not None and not ex._segments
    skinny = switch and nb * T <= ops.MOE_SKINNY_W8_MAX_ROWS
    assert skinny == (config in ("B1-T1", "B2-T4"))
    assert sorted(ex._moe_skinny.values()) == ([("gate_up", "down")] * p.cfg.n_layer if skinny else [])
    ex.kv_reset()
    check = M.check_steps_allk if kind == "allk" else M.check_steps_top2
    check(p, ex, store, tokens, T, steps, step=_no_sync_step(ex), sync=torch.cuda.synchronize, kv_dtype=kv_dtype)
    last = ex.output("output_projection").clone()
    ex.kv_reset()  # a second run of the same graph from the same state is bitwise equal
    for _ in range(steps):
        ex.step()
    torch.cuda.synchronize()
    assert torch.equal(ex.output("output_projection"), last)


def test_cli_run():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "distributed_llm_scheduler_amd.cli", "run", "--model", "mini-mixtral",
                          "--seq", "1", "--batch", "1", "--kv-cache", "64", "--moe-decode", "--moe-skinny-w8",
                          "--weight-dtype", "fp8-experts", "--past", "8", "--steps", "2"],
                         cwd=root, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
