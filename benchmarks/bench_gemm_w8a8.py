#!/usr/bin/env python3
"""fp8 x fp8 GEMM (ops.linear_w8a8, csrc/kernels/gemm_w8a8.hip: block-scaled fp8 MFMA) against the
W8A16 GEMM (ops.linear_w8) and the bf16 GEMM (ops.linear with the shipped tuning table) on the
Llama-3-8B and GPT-2 layer shapes at M = 512, weights COLD: each call reads another copy of its
weight, the copies rotating over more than the 256 MB Infinity Cache, as a once-per-step DAG
layer streams it. The three kernels alternate on the same device; every W8A8 result is checked
against the fp32 product of the same e4m3 values. Also timed alone: the row quantiser
(ops.quantize_rows_fp8) on the GEMM's input, and for the GEMMs that follow a norm the norm
(ops.layernorm / ops.rmsnorm) next to its quantising form (ops.*_q8).

    python benchmarks/bench_gemm_w8a8.py [--shapes llama|gpt2|all] [--rounds 3] [--out FILE]
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

# (name, M, N, K, act, norm in front): the shapes of profiles/w8/gemm_w8.txt
SHAPES = {
    "gpt2": [("qkv", 512, 2304, 768, None, "layernorm"), ("attn_proj", 512, 768, 768, None, None),
             ("fc", 512, 3072, 768, "gelu", "layernorm"), ("mlp_proj", 512, 768, 3072, None, None)],
    "llama": [("qkv", 512, 6144, 4096, None, "rmsnorm"), ("wo", 512, 4096, 4096, None, None),
              ("gate_up", 512, 28672, 4096, "swiglu", "rmsnorm"), ("down", 512, 4096, 14336, None, None),
              ("lm_head", 512, 128256, 4096, None, "rmsnorm")],
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fams = list(SHAPES) if a.shapes == "all" else [a.shapes]
    lines = [f"{'model':6s} {'gemm':9s} {'M':>4s} {'N':>6s} {'K':>5s} {'bf16 us':>8s} {'w8a16 us':>8s} {'w8a8 us':>8s} "
             f"{'a8/bf16':>7s} {'a8/a16':>7s} {'a8 cfg':>7s} {'best us':>8s} {'best cfg':>8s} {'a8 PF':>6s} "
             f"{'quant us':>8s} {'norm us':>8s} {'normq us':>8s} {'rel err':>8s}"]
    print(lines[0], flush=True)
    for fam in fams:
        tuning.set_model({"gpt2": "gpt2", "llama": "llama3-8b"}[fam])
        for name, M, N, K, act, norm in SHAPES[fam]:
            g = torch.Generator(device="cuda").manual_seed(1)
            x = (torch.randn(M, K, device="cuda", generator=g) * 0.5).bfloat16()
            xq, xs = ops.quantize_rows_fp8(x)
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
            # correctness of the W8A8 kernel (automatic config) against the same e4m3 values
            y = ops.linear_w8a8(xq, xs, w8[0], sc[0], act=act, workspace=ws).float()
            ref = torch.empty(M, N, device="cuda")
            xd = xq.float() * xs[:, None]
            for n0 in range(0, N, 16384):  # (the reference product in column blocks: fp32 temporaries)
                ref[:, n0:n0 + 16384] = (xd @ w8[0][n0:n0 + 16384].float().t()) * sc[0][n0:n0 + 16384]
            ref = ops._swiglu_interleaved(ref) if act == "swiglu" else ops._act_ref(ref, act)
            err = ((y - ref).abs().max() / ref.abs().max()).item()
            assert err < 2e-2, (name, err)
            del ref, y, xd
            auto = tuple(ops.ext().gemm_w8a8_pick(M, N, K))
            cands = {auto} | {(c, s) for c in range(ops.w8a8_configs()) for s in ops.W8A8_SPLITS if s * 256 <= K}
            t16, t8, ta8 = [], [], []
            for _ in range(a.rounds):  # alternate the three kernels
                t16.append(tuning._graph_time(lambda i: ops.linear(x, w16[i % copies], act=act, out=out), reps=copies))
                t8.append(tuning._graph_time(
                    lambda i: ops.linear_w8(x, w8[i % copies], sc[i % copies], act=act, out=out, workspace=ws),
                    reps=copies))
                ta8.append(tuning._graph_time(
                    lambda i: ops.linear_w8a8(xq, xs, w8[i % copies], sc[i % copies], act=act, out=out, workspace=ws),
                    reps=copies))
            best = min(((tuning._graph_time(
                lambda i: ops.linear_w8a8(xq, xs, w8[i % copies], sc[i % copies], act=act, out=out, config=c,
                                          workspace=ws),
                reps=copies), c) for c in sorted(cands)), key=lambda v: v[0])
            # the launches fp8 activations add in front of the GEMM, alone (inputs L2 / MALL warm,
            # as they are right behind their producer)
            oq, osc = torch.empty(M, K, dtype=torch.uint8, device="cuda"), torch.empty(M, device="cuda")
            tq = tuning._graph_time(lambda i: ops.quantize_rows_fp8(x, oq, osc), reps=16)
            tn = tnq = float("nan")
            if norm is not None:
                nw, nb, xn = torch.ones(K, device="cuda").bfloat16(), torch.zeros(K, device="cuda").bfloat16(), \
                    torch.empty_like(x)
                if norm == "layernorm":
                    tn = tuning._graph_time(lambda i: ops.layernorm(x, nw, nb, 1e-5, out=xn), reps=16)
                    tnq = tuning._graph_time(lambda i: ops.layernorm_q8(x, nw, nb, 1e-5, out_q=oq, out_scale=osc), reps=16)
                else:
                    tn = tuning._graph_time(lambda i: ops.rmsnorm(x, nw, 1e-5, out=xn), reps=16)
                    tnq = tuning._graph_time(lambda i: ops.rmsnorm_q8(x, nw, 1e-5, out_q=oq, out_scale=osc), reps=16)
            b16, b8, ba8 = statistics.median(t16), statistics.median(t8), statistics.median(ta8)
            line = (f"{fam:6s} {name:9s} {M:4d} {N:6d} {K:5d} {b16:8.1f} {b8:8.1f} {ba8:8.1f} {ba8 / b16:7.2f} "
                    f"{ba8 / b8:7.2f} {'c%ds%d' % auto:>7s} {best[0]:8.1f} {'c%ds%d' % best[1]:>8s} "
                    f"{2.0 * M * N * K / ba8 / 1e9:6.2f} {tq:8.1f} {tn:8.1f} {tnq:8.1f} {err:8.1e}")
            print(line, flush=True)
            lines.append(line)
            del w16, w8, sc, out, ws
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("bf16 GEMM vs W8A16 GEMM vs W8A8 GEMM (fp8 MFMA), cold weights, M = 512 (us per call, median of "
                    f"{a.rounds} alternating rounds; a8 PF = 2MNK / W8A8 time; quant / norm / normq: the row quantiser, "
                    "the norm and the quantising norm on the GEMM's input, alone)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
