"""The plan option ``skinny_gemm=True`` without a GPU: what it accepts and refuses, that it enters
``Plan.args`` and saved plans only when set and changes no program, ``resume``, decode steps of the
tiny presets on the CPU executor (which never dispatches to the skinny kernel: the option must not
change a CPU step), both CLI commands, and a replica plan on two gloo ranks."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import moe_decode_checks as M  # noqa: E402
from decode_checks import CAP, MARGIN, B, check_steps, ref_logits, stream  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402
from distributed_llm_scheduler_amd.models import registry  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402

KW = dict(world=1, batch=B, kv_cache=CAP, skinny_gemm=True)


def _prog(p):
    return [[(i.op, i.task, tuple(i.group)) for i in pr.instrs] for pr in p.programs]


def test_accepted():
    for model, kw in (("tiny-gpt2", dict(seq=1)), ("tiny-llama", dict(seq=4)), ("tiny-llama", dict(seq=16, kv_dtype="fp8")),
                      ("tiny-gpt2", dict(seq=1, generate=True)), ("tiny-llama", dict(seq=1, prefill_chunk=8)),
                      ("tiny-llama", dict(seq=1, prefill_chunk=8, generate=True, kv_dtype="fp8")),
                      ("tiny-mixtral", dict(seq=1, moe_decode=True)), ("tiny-llama", dict(seq=4, placement="pipeline"))):
        p = runtime.plan(model, **KW, **kw)
        assert p.completed == p.total and p.args["skinny_gemm"] is True
        plain = runtime.plan(model, **{k: v for k, v in KW.items() if k != "skinny_gemm"}, **kw)
        # the executor's choice of kernel, nothing the DAG, the placement or the programs see
        assert _prog(p) == _prog(plain) and p.order == plain.order and p.placement == plain.placement
        assert p.stats["kernels_per_rank"] == plain.stats["kernels_per_rank"]


def test_capped_plan_accepted():
    roomy = runtime.plan("tiny-llama", seq=1, **KW)
    pr = roomy.programs[0]
    need = pr.param_arena_bytes + pr.act_arena_bytes + roomy.kv_cache_bytes[0]
    p = runtime.plan("tiny-llama", seq=1, cap_gb=0.8 * need / 1e9, **KW)
    assert p.completed == p.total and p.programs[0].counts().get("evict", 0) > 0


def test_refused():
    with pytest.raises(ValueError, match="skinny_gemm=True needs a KV cache"):
        runtime.plan("tiny-llama", world=1, batch=B, seq=4, skinny_gemm=True)
    for wd, extra in (("fp8", {}), ("mxfp4", dict(act_dtype="fp8"))):
        with pytest.raises(ValueError, match="skinny_gemm=True takes weight_dtype='bf16' only"):
            runtime.plan("tiny-llama", seq=1, weight_dtype=wd, **extra, **KW)
    with pytest.raises(ValueError, match="moe_decode"):  # an MoE model still needs its own option
        runtime.plan("tiny-mixtral", seq=1, **KW)
    registry.check_skinny_gemm(False, None, "fp8")  # unset: nothing to check
    with pytest.raises(ValueError):
        registry.check_skinny_gemm(True, None)
    with pytest.raises(ValueError):
        registry.check_skinny_gemm(True, 64, "fp8-experts")


def test_option_unset_changes_nothing(tmp_path):
    p = runtime.plan("tiny-llama", world=1, batch=B, seq=1, kv_cache=CAP)
    assert "skinny_gemm" not in p.args
    path = str(tmp_path / "plain.json")
    runtime.save_plan(p, path)
    assert "skinny_gemm" not in json.load(open(path))["args"]
    ex = runtime.make_executor(p, 0, "cpu", runtime.make_store(p))
    assert ex.skinny_gemm is False and not ex._skinny_on and ex._skinny == {}


def test_saved_plan_resume_and_mismatch(tmp_path):
    a, b = str(tmp_path / "skinny.json"), str(tmp_path / "plain.json")
    p = runtime.plan("tiny-llama", seq=1, **KW)
    runtime.save_plan(p, a)
    assert json.load(open(a))["args"]["skinny_gemm"] is True
    again = runtime.plan("tiny-llama", seq=1, resume=a, **KW)
    assert again.order == p.order and again.args == p.args
    with pytest.raises(ValueError, match="different arguments.*skinny_gemm"):
        runtime.plan("tiny-llama", world=1, batch=B, seq=1, kv_cache=CAP, resume=a)
    plain = runtime.plan("tiny-llama", world=1, batch=B, seq=1, kv_cache=CAP)
    runtime.save_plan(plain, b)
    with pytest.raises(ValueError, match="different arguments.*skinny_gemm"):
        runtime.plan("tiny-llama", seq=1, resume=b, **KW)


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("model", ["tiny-gpt2", "tiny-llama"])
def test_cpu_steps_are_those_without_the_option(monkeypatch, model, T):
    """The CPU executor never dispatches to the skinny kernel, whatever DLS_SKINNY says: the steps
    match the reference and equal the plain plan's bit for bit."""
    monkeypatch.setenv("DLS_SKINNY", "all")
    p = runtime.plan(model, seq=T, **KW)
    plain = runtime.plan(model, world=1, batch=B, seq=T, kv_cache=CAP)
    store = runtime.make_store(p)
    tokens = stream(p.cfg.vocab_size, seed=5)
    ex = runtime.make_executor(p, 0, "cpu", store)
    ref = runtime.make_executor(plain, 0, "cpu", store)
    assert ex.skinny_gemm and not ex._skinny_on
    for e in (ex, ref):
        e.set_tokens("@tokens", tokens)
    check_steps(p, ex, store, tokens, T, steps=3)
    for _ in range(3):
        ref.step()
    assert torch.equal(ex.output("output_projection"), ref.output("output_projection")) and ex._skinny == {}


def test_cli_run_and_generate():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, "-m", "distributed_llm_scheduler_amd.cli"]
    out = subprocess.run(base + ["run", "--model", "tiny-llama", "--seq", "1", "--kv-cache", "64", "--skinny-gemm",
                                 "--past", "8", "--steps", "2", "--device", "cpu"],
                         cwd=root, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    doc = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert doc["valid"] is True and doc["kv_cache"] == 64
    out = subprocess.run(base + ["generate", "--model", "tiny-gpt2", "--kv-cache", "32", "--skinny-gemm",
                                 "--prompt-len", "3", "--new", "4", "--batch", "2", "--device", "cpu"],
                         cwd=root, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    doc = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert len(doc["tokens"]) == 2 and all(len(t) == 4 for t in doc["tokens"])
    out = subprocess.run(base + ["run", "--model", "tiny-llama", "--seq", "4", "--skinny-gemm", "--device", "cpu"],
                         cwd=root, capture_output=True, text=True, timeout=240)
    assert out.returncode != 0 and "skinny_gemm" in out.stderr


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
        T = 1
        p = runtime.plan("tiny-llama", world=world, seq=T, batch=B, kv_cache=CAP, skinny_gemm=True, placement="replica",
                         replicas=world)
        store = runtime.make_store(p)
        ex = runtime.make_executor(p, rank, "cpu", store, pg=dist.group.WORLD)
        tokens = stream(p.cfg.vocab_size, seed=11 + rank)
        ex.set_tokens(f"r{rank}/@tokens", tokens)
        res = {"rank": rank, "home": p.placement[f"r{rank}/output_projection"], "errs": [], "option": ex.skinny_gemm}
        for n in range(3):
            ex.step()
            logits = ex.output(f"r{rank}/output_projection").float()
            for b in range(B):
                ref = ref_logits(p, store, tokens[b, :(n + 1) * T])[n * T:]
                res["errs"].append(((logits[b] - ref).abs().max().item(), ref.abs().max().item()))
        q.put(res)
    finally:
        dist.destroy_process_group()


def test_replica_plan_on_two_gloo_ranks():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(timeout=240)
    assert all(pr.exitcode == 0 for pr in procs), [pr.exitcode for pr in procs]
    results = sorted((q.get(timeout=5) for _ in range(world)), key=lambda r: r["rank"])
    for r in results:
        assert r["home"] == r["rank"] and r["option"] and len(r["errs"]) == 3 * B
        assert all(err < MARGIN * scale for err, scale in r["errs"]), r
