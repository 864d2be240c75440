"""Decode steps with KV caches (runtime.plan kv_cache=C) on the CPU backend: incremental steps
equal the plain fp32 reference forward over each sequence's tokens so far, restarts, capacity,
pipeline ranks over gloo, fp8 weights, the plan's memory accounting and refusals, and the CLI.
"""
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

from decode_checks import CAP, B, check_steps, ref_logits, stream  # noqa: E402
from distributed_llm_scheduler_amd.models import registry  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402
from distributed_llm_scheduler_amd.parallel.executor import synthetic_tokens  # noqa: E402

MODELS = ["tiny-gpt2", "tiny-llama", "mini-gpt2", "mini-llama"]


@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("model", MODELS)
def test_incremental_equals_full(model, T):
    """Six steps from empty caches: after each, the T logits rows of each sequence match the
    reference forward over its first pos+T tokens, rows pos .. pos+T-1."""
    p = runtime.plan(model, world=1, seq=T, batch=B, kv_cache=CAP)
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
    tokens = synthetic_tokens("@tokens", B * CAP, p.cfg.vocab_size).view(B, CAP)  # the default stream
    check_steps(p, ex, store, tokens, T, steps=6)
    assert ex.kv_lengths() == [6 * T] * B


@pytest.mark.parametrize("model", ["tiny-gpt2", "tiny-llama"])
def test_restart_over_another_stream(model):
    """kv_reset() and a second run over other tokens: stale cache bytes are harmless."""
    T = 4
    p = runtime.plan(model, world=1, seq=T, batch=B, kv_cache=CAP)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store)
    check_steps(p, ex, store, synthetic_tokens("@tokens", B * CAP, p.cfg.vocab_size).view(B, CAP), T, steps=5)
    ex.kv_reset()
    assert ex.kv_lengths() == [0, 0]
    other = stream(p.cfg.vocab_size, seed=77)
    ex.set_tokens("@tokens", other)
    check_steps(p, ex, store, other, T, steps=3)
    ex.kv_reset([9, 2])  # ragged lengths: the rows kept are the second run's
    assert ex.kv_lengths() == [9, 2]
    ex.step()
    logits = ex.output("output_projection").float()
    for b, n in enumerate((9, 2)):
        ref = ref_logits(p, store, other[b, :n + T])[n:]
        assert (logits[b] - ref).abs().max() < 0.03 * ref.abs().max()


def test_step_past_capacity_raises_before_any_launch():
    T = 4
    p = runtime.plan("tiny-llama", world=1, seq=T, batch=B, kv_cache=CAP)
    ex = runtime.make_executor(p, 0, "cpu", runtime.make_store(p), debug=True)
    ex.kv_reset([CAP - T - 1, 0])
    ex.step()
    before = ex.output("output_projection").clone()
    k0 = {t: (k.clone(), v.clone()) for t, (k, v) in ex._kv_cache.items()}
    with pytest.raises(RuntimeError, match="past the KV cache capacity"):
        ex.step()
    assert ex.kv_lengths() == [CAP - 1, T]
    assert torch.equal(ex.output("output_projection"), before)
    assert all(torch.equal(k, ex._kv_cache[t][0]) and torch.equal(v, ex._kv_cache[t][1]) for t, (k, v) in k0.items())
    ex.check_guards()
    ex.kv_reset([CAP - T, 0])  # exactly to capacity is a step
    ex.step()
    ex.check_guards()


def test_fp8_weights_with_cache():
    T = 4
    p = runtime.plan("tiny-llama", world=1, seq=T, batch=B, kv_cache=CAP, weight_dtype="fp8")
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store)
    check_steps(p, ex, store, synthetic_tokens("@tokens", B * CAP, p.cfg.vocab_size).view(B, CAP), T, steps=4)


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
        T = 4
        p = runtime.plan("tiny-llama", world=world, seq=T, batch=B, placement="pipeline", kv_cache=CAP)
        store = runtime.make_store(p)
        ex = runtime.make_executor(p, rank, "cpu", store, pg=dist.group.WORLD)
        tokens = synthetic_tokens("@tokens", B * CAP, p.cfg.vocab_size).view(B, CAP)
        mine = sorted(t.id for t in p.tasks if t.op.kind == "attention" and p.placement[t.id] == rank)
        res = {"rank": rank, "caches": sorted(ex._kv_cache), "mine": mine, "errs": [],
               "bytes": ex.memory_bytes()["kv_cache"], "planned": p.kv_cache_bytes[rank]}
        for n in range(4):
            ex.step()
            if p.placement["output_projection"] == rank:
                logits = ex.output("output_projection").float()
                for b in range(B):
                    ref = ref_logits(p, store, tokens[b, :(n + 1) * T])[n * T:]
                    res["errs"].append(((logits[b] - ref).abs().max().item(), ref.abs().max().item()))
        res["lengths"] = ex.kv_lengths()
        q.put(res)
    finally:
        dist.destroy_process_group()


def test_two_ranks_pipeline_gloo():
    """Each rank holds only its own layers' caches; the last stage's logits match the reference."""
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
    errs = [e for r in results for e in r["errs"]]
    assert len(errs) == 4 * B and all(err < 0.03 * scale for err, scale in errs), errs
    for r in results:
        assert r["caches"] == r["mine"] and r["mine"], r
        assert r["bytes"] == r["planned"] > 0 and r["lengths"] == [16, 16]
    assert not set(results[0]["mine"]) & set(results[1]["mine"])


# ------------------------------------------------------------------------------ plan accounting

def test_plan_accounts_for_the_caches():
    T, C = 4, CAP
    p = runtime.plan("tiny-llama", world=1, seq=T, batch=B, kv_cache=C)
    base = runtime.plan("tiny-llama", world=1, seq=T, batch=B)
    cfg = p.cfg
    per_task = 2 * B * C * cfg.kv_heads * cfg.head_dim * 2
    assert p.kv_cache_bytes == [cfg.n_layer * per_task] and base.kv_cache_bytes == []
    assert p.args["kv_cache"] == C and "kv_cache" not in base.args
    mem0 = {t.id: t.memory_required for t in base.tasks}
    for t in p.tasks:
        if t.op.kind == "attention":
            assert t.op.attrs["kv_cache"] == C and registry.kv_cache_bytes(t.op) == per_task
            assert t.memory_required == pytest.approx(mem0[t.id] + per_task / 1e9, rel=1e-12)
        else:
            assert t.memory_required == mem0[t.id] and "kv_cache" not in t.op.attrs
    # the score terms count T queries x C keys
    fl0 = {t.id: t.flops for t in base.tasks}
    a = next(t for t in p.tasks if t.op.kind == "attention")
    assert a.flops - fl0[a.id] == pytest.approx((4.0 * C - 2.0 * T) * B * cfg.n_head * T * cfg.head_dim)
    assert p.stats["kv_cache_gb_per_rank"] == [cfg.n_layer * per_task / 1e9]


def test_cap_below_params_activations_and_caches_raises():
    """Caches persist next to the arenas: a GPU that cannot hold parameter arena + activation
    arena + caches raises, naming the GPU and the three figures; no plan is returned whose sum
    exceeds the cap."""
    kw = dict(world=1, seq=4, batch=8, kv_cache=128)
    p = runtime.plan("tiny-llama", **kw)
    pr = p.programs[0]
    need = pr.param_arena_bytes + pr.act_arena_bytes + p.kv_cache_bytes[0]
    ok = runtime.plan("tiny-llama", cap_gb=(need + 64) / 1e9, **kw)
    assert ok.completed == ok.total and ok.programs[0].counts().get("evict", 0) == 0
    for sched in ("EFT", "MRU_spec"):
        with pytest.raises(ValueError, match=r"GPU 0: parameter arena 0\.000\d+ GB \+ activation arena 0\.000\d+ GB \+ "
                                             r"KV caches 0\.000262 GB exceed its cap of 0\.000261 GB"):
            runtime.plan("tiny-llama", cap_gb=(p.kv_cache_bytes[0] - 1000) / 1e9, scheduler=sched, **kw)
    msg = runtime._kv_over_cap(p, [(need - 1) / 1e9])
    assert msg is not None and msg.startswith("GPU 0: parameter arena") and runtime._kv_over_cap(p, [need / 1e9]) is None


@pytest.mark.parametrize("model,sched", [("tiny-gpt2", "EFT"), ("tiny-llama", "EFT"), ("tiny-llama", "MRU_spec")])
def test_capped_plan_with_refills_and_caches(model, sched):
    """A cap below the unconstrained sum: the plan sets the caches aside, evicts and re-fills
    parameters every step, fits the cap with its caches, and its decode steps are right."""
    from distributed_llm_scheduler_amd.parallel.program import steady_fill_bytes

    T = 4
    roomy = runtime.plan(model, world=1, scheduler=sched, seq=T, batch=B, kv_cache=CAP)
    pr = roomy.programs[0]
    need = pr.param_arena_bytes + pr.act_arena_bytes + roomy.kv_cache_bytes[0]
    cap = 0.8 * need
    p = runtime.plan(model, world=1, scheduler=sched, seq=T, batch=B, kv_cache=CAP, cap_gb=cap / 1e9)
    pr = p.programs[0]
    assert p.completed == p.total and pr.counts().get("evict", 0) > 0
    assert pr.param_arena_bytes + pr.act_arena_bytes + p.kv_cache_bytes[0] <= cap
    assert p.kv_cache_bytes == roomy.kv_cache_bytes
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
    check_steps(p, ex, store, synthetic_tokens("@tokens", B * CAP, p.cfg.vocab_size).view(B, CAP), T, steps=4)
    assert ex.last.bytes_filled == steady_fill_bytes(pr, p.param_bytes) > 0


@pytest.mark.parametrize("kw,match", [
    (dict(model="tiny-mixtral"), "MoE"),
    (dict(tp=2), "tensor or sequence"),
    (dict(sp=2), "tensor or sequence"),
    (dict(merge_mb=2, replicas=2), "merge_mb"),
    (dict(kv_cache=129), "exceeds tiny-llama's 128 positions"),
    (dict(seq=17), "1 .. 16"),
    (dict(model="tiny-gqa8", seq=9), "exceeds the decode attention"),
    (dict(placement="tensor"), "placement"),
])
def test_refusals(kw, match, monkeypatch):
    from distributed_llm_scheduler_amd.models import config

    # 16 query heads on 2 KV heads: 8 query heads per KV head, 8 * 9 = 72 query rows
    monkeypatch.setitem(config.PRESETS, "tiny-gqa8", config.PRESETS["tiny-llama"].with_(
        name="tiny-gqa8", n_head=16, n_kv_head=2, n_embd=256))
    args = dict(model="tiny-llama", world=1, seq=4, batch=1, kv_cache=CAP)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        runtime.plan(**args)
    if args["model"] == "tiny-gqa8":  # eight tokens per step are 64 rows: accepted
        assert runtime.plan(**dict(args, seq=8)).kv_cache_bytes[0] > 0


def test_attn_block_with_a_cache_is_refused(monkeypatch):
    monkeypatch.setenv("DLS_ATTN_BLOCK", "1")
    with pytest.raises(ValueError, match="DLS_ATTN_BLOCK"):
        runtime.plan("tiny-gpt2", world=1, seq=4, kv_cache=CAP)
    assert runtime.plan("tiny-gpt2", world=1, seq=4).completed  # without a cache it is nobody's business


def test_saved_plan_resumes_only_with_the_same_cache(tmp_path):
    path = str(tmp_path / "plan.json")
    p = runtime.plan("tiny-llama", world=1, seq=4, batch=B, kv_cache=CAP)
    runtime.save_plan(p, path)
    assert json.load(open(path))["args"]["kv_cache"] == CAP
    again = runtime.plan("tiny-llama", world=1, seq=4, batch=B, kv_cache=CAP, resume=path)
    assert again.order == p.order and again.kv_cache_bytes == p.kv_cache_bytes
    with pytest.raises(ValueError, match="kv_cache"):
        runtime.plan("tiny-llama", world=1, seq=4, batch=B, kv_cache=32, resume=path)
    with pytest.raises(ValueError, match="kv_cache"):
        runtime.plan("tiny-llama", world=1, seq=4, batch=B, resume=path)
    plain = str(tmp_path / "plain.json")
    runtime.save_plan(runtime.plan("tiny-llama", world=1, seq=4, batch=B), plain)
    assert "kv_cache" not in json.load(open(plain))["args"]
    with pytest.raises(ValueError, match="kv_cache"):
        runtime.plan("tiny-llama", world=1, seq=4, batch=B, kv_cache=CAP, resume=plain)


def test_cli_run_with_a_cache():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "distributed_llm_scheduler_amd.cli", "run", "--model", "tiny-llama",
                          "--seq", "1", "--kv-cache", "64", "--past", "16", "--steps", "3", "--device", "cpu"],
                         cwd=root, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    doc = json.loads(lines[0])
    assert doc["valid"] is True and doc["kv_cache"] == 64 and doc["past"] == 16
    assert doc["kv_cache_gb"] == pytest.approx(2 * 1 * 64 * 2 * 16 * 2 * 2 / 1e9)
