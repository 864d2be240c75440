"""Decode steps on ranks that hold no KV cache: whether a plan has a cache is a property of the
plan, so kv_randomize / kv_reset / set_tokens / kv_lengths work on every rank alike (a pipeline
of four ranks over two layers leaves two of them without an attention task), a step past the
capacity raises on all ranks together, and the CLI's --trace and --loopback paths keep to the cache.
"""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from decode_checks import CAP, B, MARGIN, ref_logits, stream  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402

WORLD, T = 4, 4


def test_some_pipeline_ranks_hold_no_cache():
    """The premise of the test below, and of any SPMD caller: accepted plans leave ranks without a cache."""
    p = runtime.plan("tiny-llama", world=WORLD, seq=T, batch=B, placement="pipeline", kv_cache=CAP)
    assert sum(1 for n in p.kv_cache_bytes if n == 0) >= 1 and sum(p.kv_cache_bytes) > 0
    q = runtime.plan("tiny-llama", world=2, seq=T, batch=B, kv_cache=CAP)  # the default scheduler: all on one GPU
    assert sorted(q.kv_cache_bytes)[0] == 0 < sorted(q.kv_cache_bytes)[1]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = runtime.plan("tiny-llama", world=world, seq=T, batch=B, placement="pipeline", kv_cache=CAP)
        store = runtime.make_store(p)
        ex = runtime.make_executor(p, rank, "cpu", store, pg=dist.group.WORLD, debug=True)
        res = {"rank": rank, "planned": p.kv_cache_bytes[rank], "caches": len(ex._kv_cache), "errs": []}
        ex.kv_randomize(8, seed=3)  # every rank, as the CLI and any SPMD caller do
        res["randomized"] = ex.kv_lengths()
        ex.kv_reset()
        res["reset"] = ex.kv_lengths()
        tokens = stream(p.cfg.vocab_size, seed=5)
        ex.set_tokens("@tokens", tokens)  # ignored where the rank does not embed
        for n in range(3):
            ex.step()
            if p.placement["output_projection"] == rank:
                logits = ex.output("output_projection").float()
                for b in range(B):
                    ref = ref_logits(p, store, tokens[b, :(n + 1) * T])[n * T:]
                    res["errs"].append(((logits[b] - ref).abs().max().item(), ref.abs().max().item()))
        res["lengths"] = ex.kv_lengths()
        ex.kv_reset([CAP - T + 1, 0])
        try:  # past the capacity: every rank raises before it launches or posts anything, none waits
            ex.step()
            res["raised"] = None
        except RuntimeError as e:
            res["raised"] = str(e)
        res["after"] = ex.kv_lengths()
        ex.check_guards()
        q.put(res)
    finally:
        dist.destroy_process_group()


def test_four_pipeline_ranks_two_without_a_cache_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(timeout=240)
    assert all(pr.exitcode == 0 for pr in procs), [pr.exitcode for pr in procs]
    results = sorted((q.get(timeout=5) for _ in range(WORLD)), key=lambda r: r["rank"])
    bare = [r["rank"] for r in results if r["planned"] == 0]
    assert bare and len(bare) < WORLD, results
    errs = [e for r in results for e in r["errs"]]
    assert len(errs) == 3 * B and all(err < MARGIN * scale for err, scale in errs), errs
    for r in results:
        assert (r["caches"] == 0) == (r["planned"] == 0), r
        assert r["randomized"] == [8, 8] and r["reset"] == [0, 0] and r["lengths"] == [3 * T] * B, r
        assert r["raised"] is not None and "past the KV cache capacity" in r["raised"], r
        assert r["after"] == [CAP - T + 1, 0], r


def test_no_cache_in_the_plan_still_says_so():
    p = runtime.plan("tiny-llama", world=1, seq=T, batch=B)
    ex = runtime.make_executor(p, 0, "cpu", runtime.make_store(p))
    for call in (ex.kv_lengths, ex.kv_reset, lambda: ex.kv_randomize(4), lambda: ex.set_tokens("@tokens", None)):
        with pytest.raises(RuntimeError, match="no KV cache"):
            call()


def _cli(*args):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "distributed_llm_scheduler_amd.cli", "run", "--model", "tiny-llama",
                          "--device", "cpu", *args], cwd=root, capture_output=True, text=True, timeout=120)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    return out, [json.loads(ln) for ln in lines]


def test_cli_trace_step_after_a_run_that_fills_the_cache(tmp_path):
    """--past 61 + 3 steps fill 64 positions exactly; the profiled step of --trace starts from --past again."""
    trace = str(tmp_path / "trace.json")
    out, docs = _cli("--seq", "1", "--kv-cache", "64", "--past", "61", "--steps", "3", "--trace", trace)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len(docs) == 1 and docs[0]["valid"] is True and docs[0]["past"] == 61
    assert json.load(open(trace))
    out, docs = _cli("--seq", "1", "--kv-cache", "64", "--past", "62", "--steps", "3")
    assert out.returncode != 0 and not docs and "exceeds --kv-cache 64" in out.stderr


def test_cli_loopback_applies_past_and_the_capacity_check():
    """The loopback harness never resets, so its warm-up steps count: 16 + (1 + 2) x 4 <= 64 runs, 56 + 12 does not."""
    common = ("--loopback", "2", "--transport", "device", "--placement", "pipeline", "--replicas", "2", "--seq", "4",
              "--kv-cache", "64", "--warmup", "1", "--steps", "2")
    out, docs = _cli(*common, "--past", "16")
    assert out.returncode == 0, out.stderr[-2000:]
    assert len(docs) == 1 and docs[0]["valid"] is True and docs[0]["p2p_errors"] == [0, 0]
    assert docs[0]["kv_cache"] == 64 and docs[0]["past"] == 16 and docs[0]["kv_cache_gb"] > 0
    out, docs = _cli(*common, "--past", "56")
    assert out.returncode != 0 and not docs and "exceeds --kv-cache 64" in out.stderr
