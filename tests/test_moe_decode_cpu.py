"""MoE decode (runtime.plan moe_decode=True) without a GPU: what the option accepts and refuses,
what it leaves alone, ``resume``, decode steps and generation of the tiny Mixtral presets on the CPU
executor (strict on the all-k variant, the near-tie measure of moe_decode_checks.py on top-2), the
CLI, and a replica plan on two gloo ranks.
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

import generate_checks as G  # noqa: E402
import moe_decode_checks as M  # noqa: E402
from decode_checks import CAP, B, check_steps, stream  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402

KW = dict(world=1, batch=B, kv_cache=CAP, moe_decode=True)


def test_accepted_and_refused():
    for kw in (dict(seq=1), dict(seq=16), dict(seq=1, generate=True), dict(seq=4, kv_dtype="fp8"),
               dict(seq=1, generate=True, kv_dtype="fp8"), dict(seq=4, placement="pipeline")):
        p = runtime.plan("tiny-mixtral", **KW, **kw)
        assert p.completed == p.total and p.args["moe_decode"] is True and p.kv_cache_bytes[0] > 0
    # without the option the refusal stands, and names the option
    with pytest.raises(ValueError, match=r"MoE.*moe_decode=True"):
        runtime.plan("tiny-mixtral", world=1, batch=B, seq=4, kv_cache=CAP)
    refused = [
        (dict(model="tiny-mixtral", seq=4, kv_cache=None), "needs a KV cache"),
        (dict(model="tiny-llama", seq=4), "needs an MoE model"),
        (dict(model="tiny-mixtral", seq=1, prefill_chunk=8), "prefill_chunk"),
        (dict(model="tiny-mixtral", seq=4, weight_dtype="fp8-experts"), "weight_dtype='bf16' only"),
        (dict(model="tiny-mixtral", seq=4, weight_dtype="mxfp4-experts", act_dtype="fp8"), "weight_dtype='bf16' only"),
        # every other restriction of the cache holds
        (dict(model="tiny-mixtral", seq=4, tp=2), "tensor or sequence"),
        (dict(model="tiny-mixtral", seq=4, sp=2), "tensor or sequence"),
        (dict(model="tiny-mixtral", seq=4, merge_mb=2, replicas=2), "merge_mb"),
        (dict(model="tiny-mixtral", seq=4, placement="expert"), "placement"),
        (dict(model="tiny-mixtral", seq=17), "1 .. 16"),
        (dict(model="tiny-mixtral", seq=4, kv_cache=129), "exceeds tiny-mixtral's 128 positions"),
        (dict(model="tiny-mixtral", seq=4, generate=True), "seq=1"),
    ]
    for kw, match in refused:
        args = dict(KW)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            runtime.plan(**args)


def test_rep_times_t_limit(monkeypatch):
    from distributed_llm_scheduler_amd.models import config

    monkeypatch.setitem(config.PRESETS, "tiny-moe-gqa8", config.PRESETS["tiny-mixtral"].with_(
        name="tiny-moe-gqa8", n_head=16, n_kv_head=2, n_embd=256))
    with pytest.raises(ValueError, match="exceeds the decode attention"):
        runtime.plan("tiny-moe-gqa8", seq=9, **KW)
    assert runtime.plan("tiny-moe-gqa8", seq=8, **KW).completed


def test_option_unset_changes_nothing(tmp_path):
    dense = runtime.plan("tiny-llama", world=1, batch=B, seq=4, kv_cache=CAP)
    moe = runtime.plan("tiny-mixtral", world=1, batch=B, seq=4)
    assert "moe_decode" not in dense.args and "moe_decode" not in moe.args
    path = str(tmp_path / "moe.json")
    runtime.save_plan(moe, path)
    assert "moe_decode" not in json.load(open(path))["args"]
    # the decode plan's DAG is the model's own: same tasks, same program but for what the cache adds
    dec = runtime.plan("tiny-mixtral", seq=4, **KW)
    assert [(t.id, t.op.kind) for t in dec.tasks] == [(t.id, t.op.kind) for t in moe.tasks]
    assert [(i.op, i.task) for i in dec.programs[0].instrs] == [(i.op, i.task) for i in moe.programs[0].instrs]
    assert dec.stats["kernels_per_rank"] == moe.stats["kernels_per_rank"]


def test_saved_plan_resume_and_mismatch(tmp_path):
    a, b = str(tmp_path / "dec.json"), str(tmp_path / "dense.json")
    p = runtime.plan("tiny-mixtral", seq=4, **KW)
    runtime.save_plan(p, a)
    assert json.load(open(a))["args"]["moe_decode"] is True
    again = runtime.plan("tiny-mixtral", seq=4, resume=a, **KW)
    assert again.order == p.order and again.kv_cache_bytes == p.kv_cache_bytes and again.args == p.args
    with pytest.raises(ValueError, match="different arguments.*kv_cache"):
        runtime.plan("tiny-mixtral", world=1, batch=B, seq=4, resume=a)
    plain = runtime.plan("tiny-mixtral", world=1, batch=B, seq=4)
    runtime.save_plan(plain, b)
    with pytest.raises(ValueError, match="different arguments.*moe_decode"):
        runtime.plan("tiny-mixtral", seq=4, resume=b, **KW)


@pytest.mark.parametrize("T", [1, 4, 16])
def test_all_k_steps_match_the_reference(monkeypatch, T):
    """Every expert takes every token, so routing cannot flip: every row of every step is held."""
    model = M.register_allk("tiny-mixtral", monkeypatch.setitem)
    p = runtime.plan(model, seq=T, **KW)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
    tokens = stream(p.cfg.vocab_size, seed=1)
    ex.set_tokens("@tokens", tokens)
    check_steps(p, ex, store, tokens, T, steps=min(6, CAP // T))


@pytest.mark.parametrize("T", [1, 4, 16])
def test_top2_steps_near_tie_measure(T):
    p = runtime.plan("mini-mixtral", seq=T, **KW)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store)
    tokens = stream(p.cfg.vocab_size, seed=1)
    ex.set_tokens("@tokens", tokens)
    checked, clear, _ = M.check_steps_top2(p, ex, store, tokens, T, steps=24 // T if T < 16 else 4)
    # the shares the fp32 reference gives for this stream (moe_decode_checks.py)
    assert (checked, clear) == ((48, 29) if T < 16 else (128, 84))


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_all_k_generates_after_ragged_prompts(monkeypatch, kv_dtype):
    model = M.register_allk("tiny-mixtral", monkeypatch.setitem)
    p = runtime.plan(model, seq=1, generate=True, kv_dtype=kv_dtype, **KW)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
    greedy = G.run(ex, G.GREEDY)
    G.check(p, store, G.GREEDY, *greedy, kv_dtype=kv_dtype)
    sampled = G.run(ex, G.SAMPLING)
    G.check(p, store, G.SAMPLING, *sampled, kv_dtype=kv_dtype)


def test_cli_run_and_generate():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    base = [sys.executable, "-m", "distributed_llm_scheduler_amd.cli"]
    out = subprocess.run(base + ["run", "--model", "tiny-mixtral", "--seq", "1", "--kv-cache", "64", "--moe-decode",
                                 "--past", "8", "--steps", "2", "--device", "cpu"],
                         cwd=root, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    doc = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert doc["valid"] is True and doc["kv_cache"] == 64
    out = subprocess.run(base + ["generate", "--model", "tiny-mixtral", "--kv-cache", "32", "--moe-decode",
                                 "--prompt-len", "3", "--new", "4", "--batch", "2", "--device", "cpu"],
                         cwd=root, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    doc = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert len(doc["tokens"]) == 2 and all(len(t) == 4 for t in doc["tokens"])
    out = subprocess.run(base + ["run", "--model", "tiny-mixtral", "--seq", "1", "--kv-cache", "64", "--device", "cpu"],
                         cwd=root, capture_output=True, text=True, timeout=240)
    assert out.returncode != 0 and "moe_decode" in out.stderr


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
        from distributed_llm_scheduler_amd.models import config

        T = 4
        model = M.register_allk("tiny-mixtral", lambda d, k, v: d.__setitem__(k, v))
        assert model in config.PRESETS
        p = runtime.plan(model, world=world, seq=T, batch=B, kv_cache=CAP, moe_decode=True, placement="replica",
                         replicas=world)
        store = runtime.make_store(p)
        ex = runtime.make_executor(p, rank, "cpu", store, pg=dist.group.WORLD)
        tokens = stream(p.cfg.vocab_size, seed=11 + rank)
        ex.set_tokens(f"r{rank}/@tokens", tokens)
        res = {"rank": rank, "home": p.placement[f"r{rank}/output_projection"], "errs": []}
        from decode_checks import ref_logits

        for n in range(3):
            ex.step()
            logits = ex.output(f"r{rank}/output_projection").float()
            for b in range(B):
                ref = ref_logits(p, store, tokens[b, :(n + 1) * T])[n * T:]
                res["errs"].append(((logits[b] - ref).abs().max().item(), ref.abs().max().item()))
        res["lengths"] = ex.kv_lengths()
        res["bytes"] = (ex.memory_bytes()["kv_cache"], p.kv_cache_bytes[rank])
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
        assert r["home"] == r["rank"] and len(r["errs"]) == 3 * B
        assert all(err < G.MARGIN * scale for err, scale in r["errs"]), r
        assert r["bytes"][0] == r["bytes"][1] > 0
