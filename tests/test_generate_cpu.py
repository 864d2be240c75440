"""Generating plans without a GPU: what ``runtime.plan(generate=True)`` refuses and leaves alone,
``resume``, and the tiny presets generating on the CPU executor (the checks of generate_checks.py),
on one rank and as two replica requests on two gloo ranks.
"""
import json
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import generate_checks as G  # noqa: E402
from generate_checks import CAP, B  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402


def test_plan_refusals():
    with pytest.raises(ValueError, match="needs a KV cache"):
        runtime.plan("tiny-gpt2", world=1, seq=1, batch=B, generate=True)
    with pytest.raises(ValueError, match="seq=1.*not generated yet"):
        runtime.plan("tiny-gpt2", world=1, seq=4, batch=B, kv_cache=CAP, generate=True)
    with pytest.raises(ValueError, match=r"GPU 1 .* GPU 0"):
        runtime.plan("tiny-llama", world=2, seq=1, batch=B, kv_cache=CAP, placement="pipeline", generate=True)
    # one GPU, and replicas on their own GPUs, keep embedding and LM head together
    assert runtime.plan("tiny-llama", world=1, seq=1, batch=B, kv_cache=CAP, placement="pipeline",
                        generate=True).completed
    p = runtime.plan("tiny-llama", world=2, seq=1, batch=B, kv_cache=CAP, placement="replica", replicas=2,
                     generate=True)
    assert [t.op.attrs["sample"] for t in p.tasks if t.op.kind == "lm_head"] == [0, 1]


def test_default_plan_is_unchanged(tmp_path):
    base = runtime.plan("tiny-gpt2", world=1, seq=1, batch=B, kv_cache=CAP)
    assert "generate" not in base.args and base.sampler_bytes == [] and "sampler_gb_per_rank" not in base.stats
    assert all("sample" not in t.op.attrs for t in base.tasks if t.op is not None)
    gen = runtime.plan("tiny-gpt2", world=1, seq=1, batch=B, kv_cache=CAP, generate=True)
    assert gen.args["generate"] is True and gen.sampler_bytes[0] > 0
    assert [(t.id, t.op.kind) for t in gen.tasks] == [(t.id, t.op.kind) for t in base.tasks]
    assert gen.stats["kernels_per_rank"] == base.stats["kernels_per_rank"]
    a, b = str(tmp_path / "base.json"), str(tmp_path / "gen.json")
    runtime.save_plan(base, a)
    runtime.save_plan(gen, b)
    da, db = json.load(open(a)), json.load(open(b))
    assert "generate" not in da["args"] and db["args"]["generate"] is True
    assert {k: v for k, v in db["args"].items() if k != "generate"} == da["args"]
    assert da["events"] == db["events"]
    # resume: either way round is a mismatch, the matching way resumes
    with pytest.raises(ValueError, match="different arguments.*generate"):
        runtime.plan("tiny-gpt2", world=1, seq=1, batch=B, kv_cache=CAP, generate=True, resume=a)
    with pytest.raises(ValueError, match="different arguments.*generate"):
        runtime.plan("tiny-gpt2", world=1, seq=1, batch=B, kv_cache=CAP, resume=b)
    assert runtime.plan("tiny-gpt2", world=1, seq=1, batch=B, kv_cache=CAP, generate=True, resume=b).completed
    assert runtime.plan("tiny-gpt2", world=1, seq=1, batch=B, kv_cache=CAP, resume=a).args == base.args


def test_sampler_state_counts_towards_the_cap():
    p = runtime.plan("tiny-gpt2", world=1, seq=1, batch=B, kv_cache=CAP, generate=True)
    pr = p.programs[0]
    exact = (pr.param_arena_bytes + pr.act_arena_bytes + p.kv_cache_bytes[0] + p.sampler_bytes[0]) / 1e9
    assert runtime.plan("tiny-gpt2", world=1, seq=1, batch=B, kv_cache=CAP, generate=True, cap_gb=exact).completed
    without = exact - p.sampler_bytes[0] / 1e9
    assert runtime.plan("tiny-gpt2", world=1, seq=1, batch=B, kv_cache=CAP, cap_gb=without).completed
    with pytest.raises(ValueError, match="sampler state"):
        runtime.plan("tiny-gpt2", world=1, seq=1, batch=B, kv_cache=CAP, generate=True, cap_gb=without)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("model", ["tiny-gpt2", "tiny-llama"])
def test_tiny_presets_generate(model, kv_dtype):
    p = runtime.plan(model, world=1, seq=1, batch=B, kv_cache=CAP, kv_dtype=kv_dtype, generate=True)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
    greedy = G.run(ex, G.GREEDY)
    G.check(p, store, G.GREEDY, *greedy, kv_dtype=kv_dtype)
    sampled = G.run(ex, G.SAMPLING)
    G.check(p, store, G.SAMPLING, *sampled, kv_dtype=kv_dtype)
    assert not torch.equal(greedy[2], sampled[2])
    again = G.run(ex, G.SAMPLING)  # set_prompts resets: the same seed gives the same stream
    assert torch.equal(again[2], sampled[2])
    other = G.run(ex, dict(G.SAMPLING, seed=8))
    assert not torch.equal(other[2], sampled[2])
    ex.check_guards()


def test_generate_returns_the_new_tokens_and_checks_the_capacity():
    p = runtime.plan("tiny-llama", world=1, seq=1, batch=B, kv_cache=CAP, generate=True)
    ex = runtime.make_executor(p, 0, "cpu", runtime.make_store(p))
    with pytest.raises(ValueError, match="set_prompts first"):
        ex.generate(4)
    ex.set_sampling(**G.SAMPLING)
    ex.set_prompts("@tokens", G.PROMPTS)
    out = ex.generate(G.NEW)
    stream = G.state(ex)["tokens"]
    assert out == [stream[b, len(pr):len(pr) + G.NEW].tolist() for b, pr in enumerate(G.PROMPTS)]
    assert ex.kv_lengths() == [G.STEPS] * B
    ex.set_prompts("@tokens", G.PROMPTS)
    before = stream.clone()
    with pytest.raises(RuntimeError, match="do not fit the KV cache capacity"):
        ex.generate(CAP - 6)  # 7 prompt tokens + 58 new ones: one past C
    assert ex.kv_lengths() == [0] * B and torch.equal(G.state(ex)["tokens"], before)
    assert len(ex.generate(CAP - 7)[1]) == CAP - 7
    with pytest.raises(ValueError, match="set_prompts"):
        ex.set_prompts("@tokens", [[1], [2], [3]])
    with pytest.raises(ValueError, match="top_p"):
        ex.set_sampling(top_p=0.0)
    plain = runtime.plan("tiny-llama", world=1, seq=1, batch=B, kv_cache=CAP)
    ex2 = runtime.make_executor(plain, 0, "cpu", runtime.make_store(plain))
    for call in (ex2.set_sampling, lambda: ex2.set_prompts("@tokens", G.PROMPTS), lambda: ex2.generate(1)):
        with pytest.raises(RuntimeError, match="does not sample"):
            call()


def test_eos_ends_a_sequence_and_kv_reset_clears_it():
    p = runtime.plan("tiny-llama", world=1, seq=1, batch=B, kv_cache=CAP, generate=True)
    ex = runtime.make_executor(p, 0, "cpu", runtime.make_store(p))
    ex.set_prompts("@tokens", G.PROMPTS)
    first = ex.generate(G.NEW)
    eos = first[0][1]  # sequence 0's second new token ends it
    ex.set_sampling(eos=eos)
    ex.set_prompts("@tokens", G.PROMPTS)
    out = ex.generate(G.NEW)
    cut = first[0].index(eos)
    assert out[0] == first[0][:cut + 1] + [eos] * (G.NEW - cut - 1)
    assert G.state(ex)["done"].tolist()[0] == 1
    ex.kv_reset()
    assert G.state(ex)["done"].tolist() == [0, 0]


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
        p = runtime.plan("tiny-llama", world=world, seq=1, batch=B, kv_cache=CAP, placement="replica",
                         replicas=world, generate=True)
        store = runtime.make_store(p)
        ex = runtime.make_executor(p, rank, "cpu", store, pg=dist.group.WORLD)
        ex.set_sampling(**G.SAMPLING)  # every rank alike
        for r in range(world):
            ex.set_prompts(f"r{r}/@tokens", G.PROMPTS)
        out = ex.generate(G.NEW)
        pre = f"r{rank}/"
        res = {"rank": rank, "keys": sorted(out), "out": out[pre], "lengths": ex.kv_lengths(), "err": None}
        try:  # its own request's trajectory against the oracle, at the request's own ordinal
            logits, stats, stream = G.run(ex, G.SAMPLING, name=f"r{rank}/@tokens", tid=pre + "output_projection",
                                          prefix=pre)
            G.check(p, store, G.SAMPLING, logits, stats, stream, request=rank)
            assert [stream[b, len(pr):len(pr) + G.NEW].tolist() for b, pr in enumerate(G.PROMPTS)] == out[pre]
        except AssertionError as e:
            res["err"] = str(e)
        q.put(res)
    finally:
        dist.destroy_process_group()


def test_two_replica_requests_on_two_gloo_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(timeout=240)
    assert all(pr.exitcode == 0 for pr in procs), [pr.exitcode for pr in procs]
    results = sorted((q.get(timeout=5) for _ in range(2)), key=lambda r: r["rank"])
    for r in results:
        assert r["err"] is None, r
        assert r["keys"] == [f"r{r['rank']}/"] and r["lengths"] == {"r0/": [G.STEPS] * B, "r1/": [G.STEPS] * B}, r
    # the same prompts, weights and seed: the requests differ by their ordinal in the draw only
    assert results[0]["out"] != results[1]["out"]
