#!/usr/bin/env python3
"""The decode step of llama3-8b-1l (one layer of Llama-3-8B at full width, LM head included) with a
KV cache: ms per step as ONE captured hipGraph replayed over a growing sequence, the launches of
that graph, and where the time goes — per kernel group of the program (an event pair around every
group of an eager step; the groups are a launch or a few, so each figure carries about a
microsecond of event overhead) — for T new tokens per step from a context of P random cache rows
(executor.kv_randomize). The M = B*T <= 16 GEMMs run on the tiles the prefill shapes use: their
share of the step is the baseline a GEMV path would be measured against.

    python benchmarks/decode_step.py [--model llama3-8b-1l] [--kv-cache 8192] [--kv-dtype fp8] [--only B,T,past]
                                     [--out FILE] [--generate] [--skinny-gemm [--max-rows N]]

--kv-dtype fp8: the caches hold e4m3 bytes and per-(position, KV head) scales (runtime.plan kv_dtype).
--generate: instead of the breakdown, the T = 1 cases with and without on-device sampling
(runtime.plan generate=True; temperature 0.8, top_k 50, top_p 0.9, and greedy) in one session, the
captured steps alternating, and the difference.

--skinny-gemm: instead of the breakdown, every case as one captured graph of the plan with
skinny_gemm=True and one of the plan without it, in one process: five alternating rounds of ten
steps, the medians, the ratio and in how many rounds the step with the option was the faster. The
default cases are then SKINNY_CASES (llama3-8b-1l) or GPT2_SKINNY_CASES (--model gpt2). --max-rows N
sets ops.SKINNY_MAX_ROWS for the run (a bound search; the default measures what the executor does),
--lm-head 0/1 ops.SKINNY_LMHEAD.

Needs a GPU.
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_llm_scheduler_amd.models import registry  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402

CASES = [(1, 1, 512), (1, 1, 8000), (1, 16, 8000), (8, 1, 8000)]  # (batch, T, past)
SKINNY_CASES = [(1, 1, 512), (1, 1, 8000), (2, 1, 8000), (4, 1, 8000), (8, 1, 8000), (16, 1, 8000), (1, 16, 8000)]
GPT2_SKINNY_CASES = [(1, 1, 512), (8, 1, 1000)]


def one(model, C, B, T, past, steps=10, rounds=5, kv_dtype="bf16"):
    dev = torch.device("cuda:0")
    moe = bool(registry.get_config(model).n_experts)  # an MoE model's decode steps are the plan option moe_decode
    p = runtime.plan(model, world=1, seq=T, batch=B, kv_cache=C, kv_dtype=kv_dtype, moe_decode=moe)
    ex = runtime.make_executor(p, 0, dev, runtime.make_store(p, device_init=runtime.device_init_ok(p, 0)))
    ex.kv_randomize(past)
    ex.step()
    ex.kv_reset(past)
    if not ex.capture():
        raise RuntimeError("the decode step was not captured")
    assert past + steps * T <= C
    ms = []
    for _ in range(rounds):
        ex.kv_reset(past)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            ex.step()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / steps)
    ex.kv_reset(past)
    ex.step(profile=True)  # (leaves the graph; warms the eager path)
    ex.kv_reset(past)
    tl = ex.step(profile=True).timeline
    total = sum(t1 - t0 for _, t0, t1 in tl)
    kinds = {i.task: i.kind for i in p.programs[0].instrs if i.op == "run"}
    lines = [f"{model}  B {B}  T {T}  past {past}  cache {C} ({kv_dtype}, {sum(p.kv_cache_bytes) / 1e6:.1f} MB): "
             f"{statistics.median(ms) * 1e3:.1f} us per step as one hipGraph of {ex.launches} kernel launches "
             f"(min {min(ms) * 1e3:.1f}, max {max(ms) * 1e3:.1f} over {rounds} rounds of {steps} steps)",
             f"  {'kernel group (eager, event pairs)':58s} {'us':>8s} {'share':>6s}"]
    gemm = 0.0
    for name, t0, t1 in tl:
        kind = kinds.get(name, "")
        lines.append(f"  {name + '  [' + kind + ']':58s} {(t1 - t0) * 1e3:8.1f} {(t1 - t0) / total * 100:5.1f}%")
        if any(k in kind for k in ("linear", "lm_head", "swiglu_mlp")):
            gemm += t1 - t0
    attn = sum(t1 - t0 for name, t0, t1 in tl if "attention" in kinds.get(name, ""))
    lines.append(f"  groups that are GEMMs only (MLP, LM head): {gemm / total * 100:.1f}% of the eager step; the attention "
                 f"group (QKV GEMM, kv_append, attn_decode, out-projection): {attn / total * 100:.1f}%")
    del ex
    torch.cuda.empty_cache()
    return lines


def generate_delta(model, C, B, past, kv_dtype="bf16", steps=10, rounds=5):
    """us per captured step without sampling, with greedy sampling and with (0.8, 50, 0.9), alternating."""
    dev = torch.device("cuda:0")
    exs = {}
    for what, gen in (("plain", False), ("generate", True)):
        p = runtime.plan(model, world=1, seq=1, batch=B, kv_cache=C, kv_dtype=kv_dtype, generate=gen,
                         moe_decode=bool(registry.get_config(model).n_experts))
        ex = runtime.make_executor(p, 0, dev, runtime.make_store(p, device_init=runtime.device_init_ok(p, 0)))
        ex.kv_randomize(past)
        ex.step()
        ex.kv_reset(past)
        if not ex.capture():
            raise RuntimeError("the decode step was not captured")
        exs[what] = ex
    assert past + steps <= C

    def timed(ex):
        ex.kv_reset(past)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            ex.step()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps * 1e3

    t = {"plain": [], "greedy": [], "sampled": []}
    for _ in range(rounds):
        t["plain"].append(timed(exs["plain"]))
        exs["generate"].set_sampling()
        t["greedy"].append(timed(exs["generate"]))
        exs["generate"].set_sampling(temperature=0.8, top_k=50, top_p=0.9, seed=1)
        t["sampled"].append(timed(exs["generate"]))
    med = {k: statistics.median(v) for k, v in t.items()}
    line = (f"{model}  B {B}  T 1  past {past}  cache {C} ({kv_dtype}): {med['plain']:.1f} us per step without sampling "
            f"({exs['plain'].launches} launches), {med['greedy']:.1f} us greedy ({med['greedy'] - med['plain']:+.1f}), "
            f"{med['sampled']:.1f} us at (0.8, 50, 0.9) ({med['sampled'] - med['plain']:+.1f}; "
            f"{exs['generate'].launches} launches); medians of {rounds} alternating rounds of {steps} steps")
    del exs
    torch.cuda.empty_cache()
    return [line]


def skinny_delta(model, C, B, T, past, kv_dtype="bf16", steps=10, rounds=5):
    """us per captured step of the plan without and with skinny_gemm=True, the two graphs alternating."""
    from distributed_llm_scheduler_amd import ops

    dev = torch.device("cuda:0")
    moe = bool(registry.get_config(model).n_experts)
    exs, store = {}, None
    for what, flag in (("tiles", False), ("skinny", True)):
        p = runtime.plan(model, world=1, seq=T, batch=B, kv_cache=C, kv_dtype=kv_dtype, moe_decode=moe,
                         **(dict(skinny_gemm=True) if flag else {}))
        store = store or runtime.make_store(p, device_init=runtime.device_init_ok(p, 0))
        ex = runtime.make_executor(p, 0, dev, store)
        ex.kv_randomize(past)
        ex.step()
        ex.kv_reset(past)
        if not ex.capture():
            raise RuntimeError("the decode step was not captured")
        exs[what] = ex
    assert past + steps * T <= C
    ran = sorted(w for (_, w), v in exs["skinny"]._skinny.items() if v == "skinny")
    fell = sorted({v for v in exs["skinny"]._skinny.values() if v != "skinny"})

    def timed(ex):
        ex.kv_reset(past)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(steps):
            ex.step()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps * 1e3

    t = {"tiles": [], "skinny": []}
    for _ in range(rounds):
        for what in ("tiles", "skinny"):
            t[what].append(timed(exs[what]))
    med = {k: statistics.median(v) for k, v in t.items()}
    wins = sum(a < b for a, b in zip(t["skinny"], t["tiles"]))
    line = (f"{model}  B {B}  T {T}  past {past}  cache {C} ({kv_dtype}): {med['tiles']:.1f} us per step on the tiles "
            f"({exs['tiles'].launches} launches; min {min(t['tiles']):.1f}, max {max(t['tiles']):.1f}), "
            f"{med['skinny']:.1f} us with skinny_gemm ({exs['skinny'].launches} launches; min {min(t['skinny']):.1f}, "
            f"max {max(t['skinny']):.1f}): {med['tiles'] / med['skinny']:.3f}x, faster in {wins} of {rounds} rounds; "
            f"{len(ran)} GEMMs skinny (stream={exs['skinny']._skinny_stream}), fallbacks: {fell or 'none'}; "
            f"SKINNY_MAX_ROWS {ops.SKINNY_MAX_ROWS}, SKINNY_LMHEAD {ops.SKINNY_LMHEAD}; medians of {rounds} alternating "
            f"rounds of {steps} steps")
    del exs, store
    torch.cuda.empty_cache()
    return [line]


def step_breakdown(model="llama3-8b-1l", C=8192, kv_dtype="bf16", cases=CASES):
    out = []
    for B, T, past in cases:
        out += one(model, C, B, T, past, kv_dtype=kv_dtype) + [""]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b-1l")
    ap.add_argument("--kv-cache", type=int, default=8192)
    ap.add_argument("--kv-dtype", default="bf16", choices=["bf16", "fp8"])
    ap.add_argument("--only", default=None, help="B,T,past: one case")
    ap.add_argument("--out", default=None)
    ap.add_argument("--generate", action="store_true",
                    help="the T = 1 cases with and without on-device sampling, alternating, and the difference")
    ap.add_argument("--skinny-gemm", action="store_true",
                    help="every case with and without the plan option skinny_gemm, the captured steps alternating")
    ap.add_argument("--max-rows", type=int, default=None, help="with --skinny-gemm: ops.SKINNY_MAX_ROWS for this run")
    ap.add_argument("--lm-head", type=int, default=None, help="with --skinny-gemm: ops.SKINNY_LMHEAD for this run (0 / 1)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("decode_step.py needs a GPU")
    cases = [tuple(int(x) for x in a.only.split(","))] if a.only else CASES
    if a.skinny_gemm:
        from distributed_llm_scheduler_amd import ops

        if a.max_rows is not None:
            ops.SKINNY_MAX_ROWS = a.max_rows  # (read by the executor at every launch)
        if a.lm_head is not None:
            ops.SKINNY_LMHEAD = bool(a.lm_head)
        if not a.only:
            cases = GPT2_SKINNY_CASES if a.model.startswith("gpt2") else SKINNY_CASES
        lines = []
        for B, T, past in cases:
            lines += skinny_delta(a.model, min(a.kv_cache, registry.get_config(a.model).n_positions), B, T, past,
                                  a.kv_dtype)
            print(lines[-1], flush=True)
    elif a.generate:
        lines = []
        for B, T, past in cases:
            if T == 1:
                lines += generate_delta(a.model, a.kv_cache, B, past, a.kv_dtype)
    else:
        lines = step_breakdown(a.model, a.kv_cache, a.kv_dtype, cases)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
