#!/usr/bin/env python3
"""fp8-weight GEMM (ops.linear_w8, csrc/kernels/gemm_w8.hip) against the bf16 GEMM (ops.linear
with the shipped tuning table) on the Llama-3-8B and GPT-2 layer shapes at M = 512, weights
COLD: each call reads another copy of its weight, the copies rotating over more than the
256 MB Infinity Cache, as a once-per-step DAG layer streams it. The two kernels alternate on
the same device; every fp8 result is checked against the fp32 product of the same e4m3 values.

    python benchmarks/bench_gemm_w8.py [--shapes llama|gpt2|all] [--rounds 3] [--out FILE]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_llm_scheduler_amd import ops  # noqa: E402
from distributed_llm_scheduler_amd.ops import tuning  # noqa: E402

# (name, M, N, K, act): the GEMMs fp8 storage covers (GPT-2's LM head reads the tied bf16 wte)
SHAPES = {
    "gpt2": [("qkv", 512, 2304, 768, None), ("attn_proj", 512, 768, 768, None), ("fc", 512, 3072, 768, "gelu"),
             ("mlp_proj", 512, 768, 3072, None)],
    "llama": [("qkv", 512, 6144, 4096, None), ("wo", 512, 4096, 4096, None), ("gate_up", 512, 28672, 4096, "swiglu"),
              ("down", 512, 4096, 14336, None), ("lm_head", 512, 128256, 4096, None)],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fams = list(SHAPES) if a.shapes == "all" else [a.shapes]
    lines = [f"{'model':6s} {'gemm':9s} {'M':>4s} {'N':>6s} {'K':>5s} {'bf16 us':>8s} {'fp8 us':>8s} {'fp8/bf16':>8s} "
             f"{'fp8 cfg':>8s} {'best us':>8s} {'best cfg':>8s} {'bf16 TB/s':>9s} {'fp8 TB/s':>8s} {'rel err':>8s}"]
    print(lines[0], flush=True)
    for fam in fams:
        tuning.set_model({"gpt2": "gpt2", "llama": "llama3-8b"}[fam])
        for name, M, N, K, act in SHAPES[fam]:
            g = torch.Generator(device="cuda").manual_seed(1)
            x = (torch.randn(M, K, device="cuda", generator=g) * 0.5).bfloat16()
            copies = max(2, min(64, (768 << 20) // (N * K * 2) + 1))
            w16, w8, sc = [], [], []
            for _ in range(copies):
                w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).bfloat16()
                q, s = ops.quantize_fp8(w)
                if act == "swiglu":
                    w = ops.interleave_gate_up(w)
                    q = ops.interleave_gate_up(q.view(torch.uint8)).view(torch.float8_e4m3fn)
                    s = ops.interleave_gate_up(s)
                w16.append(w), w8.append(q), sc.append(s)
                del w
            NO = N // 2 if act == "swiglu" else N
            out = torch.empty(M, NO, device="cuda", dtype=torch.bfloat16)
            ws = torch.empty(8 * M * N, device="cuda", dtype=torch.float32)
            # correctness of the fp8 kernel (automatic config) against the same e4m3 values
            y = ops.linear_w8(x, w8[0], sc[0], act=act, workspace=ws).float()
            ref = torch.empty(M, N, device="cuda")
            for n0 in range(0, N, 16384):  # (the reference product in column blocks: fp32 temporaries)
                ref[:, n0:n0 + 16384] = (x.float() @ w8[0][n0:n0 + 16384].float().t()) * sc[0][n0:n0 + 16384]
            ref = ops._swiglu_interleaved(ref) if act == "swiglu" else ops._act_ref(ref, act)
            err = ((y - ref).abs().max() / ref.abs().max()).item()
            assert err < 2e-2, (name, err)
            del ref, y
            auto = tuple(ops.ext().gemm_w8_pick(M, N, K))
            cands = {auto} | {(c, s) for c in range(ops.w8_configs()) for s in ops.W8_SPLITS if s * 256 <= K}
            t16, t8 = [], []
            for _ in range(a.rounds):  # alternate the two kernels
                t16.append(tuning._graph_time(lambda i: ops.linear(x, w16[i % copies], act=act, out=out), reps=copies))
                t8.append(tuning._graph_time(
                    lambda i: ops.linear_w8(x, w8[i % copies], sc[i % copies], act=act, out=out, workspace=ws),
                    reps=copies))
            best = min(((tuning._graph_time(
                lambda i: ops.linear_w8(x, w8[i % copies], sc[i % copies], act=act, out=out, config=c, workspace=ws),
                reps=copies), c) for c in sorted(cands)), key=lambda v: v[0])
            b16, b8 = statistics.median(t16), statistics.median(t8)
            line = (f"{fam:6s} {name:9s} {M:4d} {N:6d} {K:5d} {b16:8.1f} {b8:8.1f} {b8 / b16:8.2f} "
                    f"{'c%ds%d' % auto:>8s} {best[0]:8.1f} {'c%ds%d' % best[1]:>8s} {N * K * 2 / b16 / 1e6:9.2f} "
                    f"{N * K / b8 / 1e6:8.2f} {err:8.1e}")
            print(line, flush=True)
            lines.append(line)
            del w16, w8, sc, out, ws
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("fp8-weight GEMM vs bf16 GEMM, cold weights, M = 512 (us per call, median of "
                    f"{a.rounds} alternating rounds; weight TB/s = weight bytes / time)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
