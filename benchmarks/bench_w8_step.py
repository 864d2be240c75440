#!/usr/bin/env python3
"""One model's step on one GPU under a parameter cap, in bf16 and with fp8 weight storage, the
two modes alternating on the same device: step time, tasks completed, GB the plan re-fills per
step and kernel launches of the captured step. One JSON line per run.

    python benchmarks/bench_w8_step.py --model llama3-8b --cap 10.3 [--scheduler EFT] [--rounds 2]
    python benchmarks/bench_w8_step.py --model mixtral-8x7b --weight-dtype fp8-experts [--cap 65.4]

    python benchmarks/bench_w8_step.py --model llama3-8b --modes bf16,fp8,fp8+a8
    python benchmarks/bench_w8_step.py --model llama3-8b --cap 5.993 --modes fp8+a8,mxfp4+a8
    python benchmarks/bench_w8_step.py --model mixtral-8x7b --modes bf16,fp8-experts,mxfp4-experts+a8
    python benchmarks/bench_w8_step.py --model mixtral-8x7b --weight-dtype mxfp4-experts [--cap 40]

``--weight-dtype D`` runs bf16 next to D (``--modes`` lists the modes explicitly). Mode ``fp8+a8``
is fp8 weights with fp8 activations (``act_dtype="fp8"``: the fp8 x fp8 GEMM); ``--act-dtype fp8``
adds it to the default modes. Mode ``mxfp4+a8`` is MXFP4 weights with fp8 activations (the W4A8
GEMM; MXFP4 weights have no other mode), ``mxfp4-experts+a8`` the same for the expert weights of an
MoE model (the grouped W4A8 GEMM); ``--weight-dtype mxfp4`` / ``mxfp4-experts`` mean these modes.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402


def run(model, cap, sched, mode, steps, warmup):
    dev = torch.device("cuda:0")
    wd, ad = (mode[:-3], "fp8") if mode.endswith("+a8") else (mode, "bf16")
    p = runtime.plan(model, world=1, scheduler=sched, cap_gb=cap, cost_model="bytes", weight_dtype=wd, act_dtype=ad)
    store = runtime.make_store(p, device_init=runtime.device_init_ok(p, 0))
    ex = runtime.make_executor(p, 0, dev, store)
    for _ in range(warmup):
        ex.step()
    torch.cuda.synchronize()
    ex.capture()
    st = ex.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        st = ex.step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    out = {"model": model, "weight_dtype": wd, "act_dtype": ad, "scheduler": p.scheduler_name, "cap_gb": cap,
           "param_gb": round(sum(p.param_bytes.values()) / 1e9, 3), "tasks_completed": p.completed,
           "tasks_total": p.total, "ms_per_step": round(ms, 3),
           "refill_gb_per_step_planned": round(p.stats["refill_gb_per_step_per_rank"][0], 3),
           "launches": ex.launches}
    del ex, store, p
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="llama3-8b")
    ap.add_argument("--cap", type=float, default=288.0)
    ap.add_argument("--scheduler", default="EFT")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--weight-dtype", default="fp8", choices=["fp8", "fp8-experts", "mxfp4", "mxfp4-experts"],
                    help="the quantised mode measured next to bf16 (fp8-experts, mxfp4-experts: the MoE models; the "
                         "mxfp4 modes always run with fp8 activations)")
    ap.add_argument("--act-dtype", default="bf16", choices=["bf16", "fp8"],
                    help="fp8: also run <--weight-dtype>+a8 (fp8 activations; with --weight-dtype fp8)")
    ap.add_argument("--modes", default=None,
                    help="comma-separated modes: a weight dtype, fp8+a8 or mxfp4+a8 (default: bf16,<--weight-dtype>)")
    a = ap.parse_args()
    if a.modes is None and a.weight_dtype.startswith("mxfp4"):
        a.modes = "bf16," + a.weight_dtype + "+a8"
    if a.modes is None:
        a.modes = "bf16," + a.weight_dtype + ("," + a.weight_dtype + "+a8" if a.act_dtype == "fp8" else "")
    for _ in range(a.rounds):
        for mode in a.modes.split(","):
            print(json.dumps(run(a.model, a.cap, a.scheduler, mode, a.steps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
