#!/usr/bin/env python3
"""MXFP4 x fp8 GEMM (ops.linear_w4a8, csrc/kernels/gemm_w4a8.hip: fp4 x fp8 on the block-scaled
MFMA with the stored e8m0 block scales) against the W8A8 GEMM (ops.linear_w8a8) and the bf16 GEMM
(ops.linear with the shipped tuning table) on the Llama-3-8B and GPT-2 layer shapes of
bench_gemm_w8a8.py at M = 512, weights COLD: each call reads another copy of its weight, and the
copies of EVERY format rotate over more than the 256 MB Infinity Cache (the copy count is sized by
the smallest format, MXFP4 at 0.53 bytes per element), as a once-per-step DAG layer streams it.
The three kernels alternate on the same device; every W4A8 result is checked against the fp32
product of the same dequantised values.

    python benchmarks/bench_gemm_w4a8.py [--shapes llama|gpt2|all] [--rounds 3] [--out FILE]
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
from bench_gemm_w8a8 import SHAPES  # noqa: E402  (the nine shapes)

F8 = torch.float8_e4m3fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fams = list(SHAPES) if a.shapes == "all" else [a.shapes]
    lines = [f"{'model':6s} {'gemm':9s} {'M':>4s} {'N':>6s} {'K':>5s} {'copies':>6s} {'w4 MB':>6s} {'bf16 us':>8s} "
             f"{'w8a8 us':>8s} {'w4a8 us':>8s} {'w4/bf16':>7s} {'w4/w8':>6s} {'w4 cfg':>7s} {'best us':>8s} "
             f"{'best cfg':>8s} {'w4 PF':>6s} {'w4 GB/s':>8s} {'rel err':>8s}"]
    print(lines[0], flush=True)
    for fam in fams:
        tuning.set_model({"gpt2": "gpt2", "llama": "llama3-8b"}[fam])
        for name, M, N, K, act, _norm in SHAPES[fam]:
            g = torch.Generator(device="cuda").manual_seed(1)
            x = (torch.randn(M, K, device="cuda", generator=g) * 0.5).bfloat16()
            xq, xs = ops.quantize_rows_fp8(x)
            w4_bytes = N * K // 2 + N * K // 32
            copies = max(2, min(1024, (288 << 20) // w4_bytes + 1))  # > 256 MB of the smallest format
            w16, w8, sc, w4, s4 = [], [], [], [], []
            for _ in range(copies):
                w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).bfloat16()
                q, s = ops.quantize_fp8(w)
                q4, e4 = ops.quantize_mxfp4(w)
                if act == "swiglu":
                    w = ops.interleave_gate_up(w)
                    q = ops.interleave_gate_up(q.view(torch.uint8)).view(F8)
                    s = ops.interleave_gate_up(s)
                    q4, e4 = ops.interleave_gate_up(q4), ops.interleave_gate_up(e4)
                w16.append(w), w8.append(q), sc.append(s), w4.append(q4), s4.append(e4)
                del w
            NO = N // 2 if act == "swiglu" else N
            out = torch.empty(M, NO, device="cuda", dtype=torch.bfloat16)
            ws = torch.empty(8 * M * N, device="cuda", dtype=torch.float32)
            # correctness of the W4A8 kernel (automatic config) against the same dequantised values
            y = ops.linear_w4a8(xq, xs, w4[0], s4[0], act=act, workspace=ws).float()
            ref = torch.empty(M, N, device="cuda")
            xd = xq.float() * xs[:, None]
            for n0 in range(0, N, 16384):  # (the reference product in column blocks: fp32 temporaries)
                ref[:, n0:n0 + 16384] = xd @ ops.dequantize_mxfp4(w4[0][n0:n0 + 16384], s4[0][n0:n0 + 16384],
                                                                  torch.float32).t()
            ref = ops._swiglu_interleaved(ref) if act == "swiglu" else ops._act_ref(ref, act)
            err = ((y - ref).abs().max() / ref.abs().max()).item()
            assert err < 2e-2, (name, err)
            del ref, y, xd
            auto = tuple(ops.ext().gemm_w4a8_pick(M, N, K))
            cands = {auto} | {(c, s) for c in range(ops.w4a8_configs()) for s in ops.W4A8_SPLITS if s * 256 <= K}
            t16, t8, t4 = [], [], []
            for _ in range(a.rounds):  # alternate the three kernels
                t16.append(tuning._graph_time(lambda i: ops.linear(x, w16[i % copies], act=act, out=out), reps=copies))
                t8.append(tuning._graph_time(
                    lambda i: ops.linear_w8a8(xq, xs, w8[i % copies], sc[i % copies], act=act, out=out, workspace=ws),
                    reps=copies))
                t4.append(tuning._graph_time(
                    lambda i: ops.linear_w4a8(xq, xs, w4[i % copies], s4[i % copies], act=act, out=out, workspace=ws),
                    reps=copies))
            best = min(((tuning._graph_time(
                lambda i: ops.linear_w4a8(xq, xs, w4[i % copies], s4[i % copies], act=act, out=out, config=c,
                                          workspace=ws),
                reps=copies), c) for c in sorted(cands)), key=lambda v: v[0])
            b16, b8, b4 = statistics.median(t16), statistics.median(t8), statistics.median(t4)
            line = (f"{fam:6s} {name:9s} {M:4d} {N:6d} {K:5d} {copies:6d} {copies * w4_bytes / 2 ** 20:6.0f} {b16:8.1f} "
                    f"{b8:8.1f} {b4:8.1f} {b4 / b16:7.2f} {b4 / b8:6.2f} {'c%ds%d' % auto:>7s} {best[0]:8.1f} "
                    f"{'c%ds%d' % best[1]:>8s} {2.0 * M * N * K / b4 / 1e9:6.2f} {w4_bytes / b4 / 1e3:8.0f} {err:8.1e}")
            print(line, flush=True)
            lines.append(line)
            del w16, w8, sc, w4, s4, out, ws
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("bf16 GEMM vs W8A8 GEMM vs W4A8 GEMM (MXFP4 x fp8 on the block-scaled MFMA), cold weights, M = 512 "
                    f"(us per call, median of {a.rounds} alternating rounds; copies / w4 MB: weight copies each call "
                    "rotates over and their MXFP4 bytes; w4 PF = 2MNK / W4A8 time; w4 GB/s = MXFP4 weight bytes / "
                    "W4A8 time; best: the fastest forced W4A8 config, one run each)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
