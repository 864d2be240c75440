"""Chunked prompt prefill (runtime.plan prefill_chunk=Tc) without a GPU: what the plan refuses,
leaves alone and accounts for, and the tiny presets on the CPU executor — ragged prefills from
NaN-filled caches followed by token steps, a second prefill, generation after a chunked prefill
(the checks of prefill_checks.py), fp8 caches, two requests and fp8 weights.
"""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_checks as DC  # noqa: E402
import generate_checks as G  # noqa: E402
import prefill_checks as P  # noqa: E402
from decode_checks import CAP, B  # noqa: E402
from distributed_llm_scheduler_amd.models import registry  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402

TC = 5
MODELS = ["tiny-gpt2", "tiny-llama"]


def _plan(model, **kw):
    args = dict(world=1, seq=1, batch=B, kv_cache=CAP, prefill_chunk=TC)
    args.update(kw)
    return runtime.plan(model, **args)


def _executor(p, store=None, **kw):
    store = store or runtime.make_store(p)
    return runtime.make_executor(p, 0, "cpu", store, **kw), store


# ---------------------------------------------------------------------------------------------
# plan and registry

def test_refusals():
    with pytest.raises(ValueError, match="prefill_chunk needs a KV cache"):
        runtime.plan("tiny-gpt2", world=1, seq=1, batch=B, prefill_chunk=TC)
    with pytest.raises(ValueError, match="prefill_chunk needs seq=1, got 4"):
        runtime.plan("tiny-gpt2", world=1, seq=4, batch=B, kv_cache=CAP, prefill_chunk=TC)
    for bad in (1, CAP + 1, 2.0, True, "8"):
        with pytest.raises(ValueError, match=rf"prefill_chunk must be an int in 2 .. min\(kv_cache, 1024\) = {CAP}"):
            _plan("tiny-gpt2", prefill_chunk=bad)
    with pytest.raises(ValueError, match=r"= 1024, got 1025"):
        registry.check_prefill_chunk(1025, 1, 4096)
    registry.check_prefill_chunk(None, 7, None)
    registry.check_prefill_chunk(1024, 1, 4096)
    with pytest.raises(ValueError, match=r"prefill_chunk: the program of GPU \d has \d+ sends / receives"):
        _plan("tiny-llama", world=2, placement="pipeline")
    # replicas on their own GPUs exchange nothing
    assert _plan("tiny-llama", world=2, placement="replica", replicas=2).prefill_bytes[1] > 0


@pytest.mark.parametrize("model,sched", [("tiny-gpt2", "EFT"), ("tiny-llama", "MRU_spec")])
def test_a_plan_that_refills_parameters_is_refused(model, sched):
    """The capped plans of test_decode_cpu.py, which evict and re-fill parameters every step."""
    roomy = runtime.plan(model, world=1, scheduler=sched, seq=1, batch=B, kv_cache=CAP)
    pr = roomy.programs[0]
    cap = 0.8 * (pr.param_arena_bytes + pr.act_arena_bytes + roomy.kv_cache_bytes[0]) / 1e9
    capped = runtime.plan(model, world=1, scheduler=sched, seq=1, batch=B, kv_cache=CAP, cap_gb=cap)
    assert capped.stats["refill_gb_per_step_per_rank"][0] > 0
    with pytest.raises(ValueError, match="re-fills parameters in the steady state"):
        runtime.plan(model, world=1, scheduler=sched, seq=1, batch=B, kv_cache=CAP, cap_gb=cap, prefill_chunk=2)


@pytest.mark.parametrize("kw", [{}, {"generate": True}, {"kv_dtype": "fp8"}])
def test_the_plan_without_the_option_is_unchanged(tmp_path, kw):
    base = _plan("tiny-gpt2", prefill_chunk=None, **kw)
    assert "prefill_chunk" not in base.args and base.prefill_bytes == [] and "prefill_gb_per_rank" not in base.stats
    pf = _plan("tiny-gpt2", **kw)
    assert pf.args["prefill_chunk"] == TC and pf.prefill_bytes[0] > 0
    assert pf.stats["prefill_gb_per_rank"] == [pf.prefill_bytes[0] / 1e9]
    assert [t.to_dict() for t in pf.tasks] == [t.to_dict() for t in base.tasks]
    assert pf.placement == base.placement and pf.order == base.order
    assert [(i.op, i.task, i.group, i.param) for i in pf.programs[0].instrs] == \
           [(i.op, i.task, i.group, i.param) for i in base.programs[0].instrs]
    assert pf.programs[0].act_offset == base.programs[0].act_offset
    for k in ("kernels_per_rank", "act_arena_gb_per_rank", "param_peak_gb_per_rank", "kv_cache_gb_per_rank"):
        assert pf.stats[k] == base.stats[k]
    a, b = str(tmp_path / "base.json"), str(tmp_path / "pf.json")
    runtime.save_plan(base, a)
    runtime.save_plan(pf, b)
    da, db = json.load(open(a)), json.load(open(b))
    assert "prefill_chunk" not in da["args"] and db["args"]["prefill_chunk"] == TC
    assert {k: v for k, v in db["args"].items() if k != "prefill_chunk"} == da["args"] and da["events"] == db["events"]
    with pytest.raises(ValueError, match="different arguments.*prefill_chunk"):
        _plan("tiny-gpt2", resume=a, **kw)
    with pytest.raises(ValueError, match="different arguments.*prefill_chunk"):
        _plan("tiny-gpt2", prefill_chunk=None, resume=b, **kw)
    with pytest.raises(ValueError, match="different arguments.*prefill_chunk"):
        _plan("tiny-gpt2", prefill_chunk=TC + 1, resume=b, **kw)
    assert _plan("tiny-gpt2", resume=b, **kw).prefill_bytes == pf.prefill_bytes
    assert _plan("tiny-gpt2", prefill_chunk=None, resume=a, **kw).args == base.args


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_chunk_buffers_count_towards_the_cap_and_match_the_executor(kv_dtype):
    p = _plan("tiny-llama", kv_dtype=kv_dtype, generate=True)
    pr = p.programs[0]
    exact = pr.param_arena_bytes + pr.act_arena_bytes + p.kv_cache_bytes[0] + p.sampler_bytes[0] + p.prefill_bytes[0]
    assert _plan("tiny-llama", kv_dtype=kv_dtype, generate=True, cap_gb=exact / 1e9).completed
    without = (exact - p.prefill_bytes[0]) / 1e9
    assert _plan("tiny-llama", kv_dtype=kv_dtype, generate=True, prefill_chunk=None, cap_gb=without).completed
    with pytest.raises(ValueError, match=rf"chunk-step buffers {p.prefill_bytes[0] / 1e9:.6f} GB exceed its cap"):
        _plan("tiny-llama", kv_dtype=kv_dtype, generate=True, cap_gb=without)
    # a wider chunk needs more; the fp8 cache adds its dequantisation workspace
    assert _plan("tiny-llama", kv_dtype=kv_dtype, prefill_chunk=2 * TC).prefill_bytes[0] > \
        _plan("tiny-llama", kv_dtype=kv_dtype).prefill_bytes[0]
    if kv_dtype == "fp8":
        a = p.tasks[[t.op.kind for t in p.tasks].index("attention")].op.attrs
        ws = 2 * 2 * B * CAP * a["n_kv_head"] * a["head_dim"]
        assert p.prefill_bytes[0] - _plan("tiny-llama", generate=True).prefill_bytes[0] == ws
    ex, _store = _executor(p, debug=True)
    m = ex.memory_bytes()
    assert m["prefill"] == p.prefill_bytes[0] and m["activations"] == max(pr.act_arena_bytes, 256)
    base, _ = _executor(_plan("tiny-llama", kv_dtype=kv_dtype, generate=True, prefill_chunk=None))
    assert "prefill" not in base.memory_bytes()
    assert m["workspace"] - base.memory_bytes()["workspace"] == ex._pp.ws_extra <= p.prefill_bytes[0]
    assert ex.prefill(2 * TC + 1) == 3  # (debug mode: every step ends in check_guards, the new slab's canary included)
    ex.step()
    ex.check_guards()
    ex._prefill_full[-1] = 0
    with pytest.raises(RuntimeError, match="prefill arena guard overwritten"):
        ex.check_guards()


def test_chunk_step_skips_everything_past_the_last_attention():
    p = _plan("tiny-llama")
    ex, _ = _executor(p)
    kinds = [[ex.tasks[t].op.kind for t in ex.prog.instrs[i].group] for i in sorted(ex._ck["runs"])]
    n_layer = sum(1 for t in p.tasks if t.op.kind == "attention")
    assert sum("attention" in k for k in kinds) == n_layer and "attention" in kinds[-1]
    assert not any("lm_head" in k for k in kinds) and sum("swiglu_mlp" in k for k in kinds) == n_layer - 1
    # no logits buffer of the chunk shape: the arena holds hidden rows only
    V, H = p.cfg.vocab_size, p.cfg.n_embd
    assert ex._pp.arena_bytes < 2 * B * TC * V and all(v.shape[-1] <= 4 * H for v in ex._ck["views"].values())
    assert ex.step_chunk().kernels == len(kinds)


# ---------------------------------------------------------------------------------------------
# the executor

def _ragged(model, kv_dtype="bf16", **kw):
    p = _plan(model, kv_dtype=kv_dtype, **kw)
    ex, store = _executor(p, debug=True)
    tokens = DC.stream(p.cfg.vocab_size, seed=5)
    ex.set_tokens("@tokens", tokens)
    P.poison_caches(ex)
    return p, ex, store, tokens


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("model", MODELS)
def test_ragged_prefill_then_token_steps(model, kv_dtype):
    p, ex, store, tokens = _ragged(model, kv_dtype)
    assert ex.prefill([13, 4]) == 3 and ex.kv_lengths() == [13, 4]
    P.check_token_steps(p, ex, store, tokens, 6, kv_dtype, what="after prefill([13, 4])")
    # a second prefill continues from the ragged lengths
    assert ex.kv_lengths() == [19, 10]
    assert ex.prefill([20, 20]) == 2 and ex.kv_lengths() == [20, 20]
    P.check_token_steps(p, ex, store, tokens, 2, kv_dtype, what="after prefill([20, 20])")


def test_prefill_targets_and_errors():
    p, ex, store, tokens = _ragged("tiny-gpt2")
    assert ex.prefill(TC) == 1 and ex.kv_lengths() == [TC, TC]
    assert ex.prefill([TC, TC]) == 0 and ex.kv_lengths() == [TC, TC]  # nothing to do: no step
    before = [c.clone() for cs in ex._kv_cache.values() for c in cs]
    pos = ex._kv[""]["pos"].clone()
    for bad, why in (([TC - 1, 9], "below its present length"), ([9, CAP + 1], "above the capacity"),
                     ([9], "2 target lengths wanted"), ({"r0/": [9, 9]}, "no target for request ''")):
        with pytest.raises(ValueError, match=why):
            ex.prefill(bad)
    with pytest.raises(ValueError, match="give the target lengths"):
        ex.prefill()  # (no prompts: not a generating plan)
    assert ex.kv_lengths() == [TC, TC] and torch.equal(ex._kv[""]["pos"], pos)
    after = [c for cs in ex._kv_cache.values() for c in cs]
    assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(after, before)), "something was launched"
    assert ex.prefill({"": [CAP, CAP - 3]}) == -(-(CAP - TC) // TC) and ex.kv_lengths() == [CAP, CAP - 3]
    with pytest.raises(RuntimeError, match="past the KV cache capacity"):
        ex.step()
    no_chunks, _ = _executor(_plan("tiny-gpt2", prefill_chunk=None))
    with pytest.raises(RuntimeError, match="no chunk step"):
        no_chunks.prefill(4)


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("sampling", [G.GREEDY, G.SAMPLING], ids=["greedy", "sampling"])
@pytest.mark.parametrize("model", MODELS)
def test_generate_after_chunked_prefill(model, sampling, kv_dtype):
    p = _plan(model, prefill_chunk=4, generate=True, kv_dtype=kv_dtype)
    ex, store = _executor(p, debug=True)
    P.poison_caches(ex)
    chunks, logits, stats, stream = P.run_generate(ex, sampling)
    assert chunks == 2 and len(logits) == G.NEW  # prompts of 3 and 7 tokens: targets 2 and 6, Tc = 4
    P.check_generate(p, store, sampling, logits, stats, stream, kv_dtype=kv_dtype)
    # generate() itself: the same ids, n per sequence, from a fresh start
    ex.set_prompts("@tokens", G.PROMPTS)
    out = ex.generate(G.NEW)
    assert ex.prefill_steps == 2 and ex.kv_lengths() == [len(pr) - 1 + G.NEW for pr in G.PROMPTS]
    assert out == [stream[b, len(pr):len(pr) + G.NEW].tolist() for b, pr in enumerate(G.PROMPTS)]
    with pytest.raises(RuntimeError, match="do not fit the KV cache capacity"):
        ex.set_prompts("@tokens", G.PROMPTS)
        ex.generate(CAP - 6)


def test_generate_without_the_option_is_unchanged():
    """The token-step-only path gives the stream the chunked path gives (greedy, tiny-llama)."""
    outs = []
    for tc in (None, 4):
        p = _plan("tiny-llama", prefill_chunk=tc, generate=True)
        ex, _ = _executor(p)
        ex.set_sampling(**G.GREEDY)
        ex.set_prompts("@tokens", G.PROMPTS)
        outs.append(ex.generate(G.NEW))
        assert getattr(ex, "prefill_steps", None) == (2 if tc else None)
    assert outs[0] == outs[1]


def test_two_requests_through_the_dict_forms():
    p = _plan("tiny-llama", replicas=2)
    ex, store = _executor(p, debug=True)
    P.poison_caches(ex)
    toks = {pre: DC.stream(p.cfg.vocab_size, seed=7 + i) for i, pre in enumerate(("r0/", "r1/"))}
    for pre, t in toks.items():
        ex.set_tokens(pre + "@tokens", t)
    with pytest.raises(ValueError, match="no target for request 'r1/'"):
        ex.prefill({"r0/": [13, 4]})
    assert ex.prefill({"r0/": [13, 4], "r1/": [0, 21]}) == 5
    assert ex.kv_lengths() == {"r0/": [13, 4], "r1/": [0, 21]}
    ex.step()
    for pre, t in toks.items():
        lens = [n - 1 for n in ex.kv_lengths()[pre]]
        ref = DC.full_reference(p, store, t, max(lens) + 1)
        logits = ex.output(pre + "output_projection").float().cpu()[:, 0]
        for b, n in enumerate(lens):
            err, scale = (logits[b] - ref[b, n]).abs().max().item(), ref[b].abs().max().item()
            assert err < DC.MARGIN * scale, f"request {pre} sequence {b}: {err:.4g} >= {DC.MARGIN} x {scale:.4g}"


def test_cli_generate_with_prefill_chunk(capsys):
    from distributed_llm_scheduler_amd.cli import main

    args = ["generate", "--model", "tiny-llama", "--kv-cache", str(CAP), "--prompt-len", "20", "--new", "4", "--batch",
            "2", "--device", "cpu"]
    assert main(args + ["--prefill-chunk", "8"]) == 0
    chunked = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert main(args) == 0
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert chunked["prefill_chunk"] == 8 and chunked["chunk_steps"] == 3 and chunked["first_token_ms"] > 0
    assert chunked["steps"] == 3 + 4 and plain["steps"] == 19 + 4 and "chunk_steps" not in plain
    assert chunked["tokens"] == plain["tokens"] and all(len(t) == 4 for t in chunked["tokens"])


def test_fp8_weights():
    p = _plan("tiny-llama", weight_dtype="fp8")
    ex, store = _executor(p)
    tokens = DC.stream(p.cfg.vocab_size, seed=9)
    ex.set_tokens("@tokens", tokens)
    P.poison_caches(ex)
    assert ex.prefill([13, 4]) == 3
    P.check_token_steps(p, ex, store, tokens, 3, what="fp8 weights")
