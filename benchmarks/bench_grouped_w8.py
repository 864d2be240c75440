#!/usr/bin/env python3
"""Grouped fp8-weight GEMM (ops.gemm_grouped_w8, csrc/kernels/gemm_w8_grouped.hip) against the
bf16 grouped GEMM (ops.gemm_grouped with the shipped tuning table) on Mixtral-8x7B's expert
shapes: gate/up (N 28672, K 4096, SwiGLU, rows gathered by a_rows) and down (N 4096, K 14336,
compact outputs), 8 groups over 1024 routed rows split as a real step's routing
(profiles/r6_mixtral/rows_vs_time.txt: one balanced layer, one with a heavy expert). Weights
COLD: each call reads another set of the 8 experts' weights (one set is 0.9 - 1.9 GB, several
times the 256 MB Infinity Cache). Every config of the new kernel; the kernels alternate on the
same device; the fp8 result is checked against the fp32 product of the same e4m3 values.

    python benchmarks/bench_grouped_w8.py [--rounds 3] [--sets 2] [--out FILE]
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

SPLITS = {"balanced": [105, 153, 130, 107, 131, 124, 138, 136],  # layer 1
          "heavy": [98, 156, 227, 110, 133, 81, 117, 102]}       # layer 23
M, TOPK, H, F = 512, 2, 4096, 14336
GEMMS = [("gate_up", 2 * F, H, "swiglu"), ("down", H, F, None)]


def ptrs(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tuning.set_model("mixtral-8x7b")
    E, R = 8, M * TOPK
    ncfg = ops.w8_grouped_configs()
    head = (f"{'gemm':8s} {'split':9s} {'bf16 us':>8s} {'fp8 us':>8s} {'fp8/bf16':>8s} {'auto':>5s} "
            + " ".join(f"{'c%d(%d) us' % (c, ops.w8_grouped_tile_rows(c)):>11s}" for c in range(ncfg))
            + f" {'bf16 TB/s':>9s} {'fp8 TB/s':>8s} {'rel err':>8s}")
    lines = [head]
    print(head, flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    for name, N, K, act in GEMMS:
        NO = N // 2 if act else N
        w16, w8, sc = [], [], []
        for _ in range(a.sets):
            s16, s8, ssc = [], [], []
            for _ in range(E):
                w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).bfloat16()
                q, s = ops.quantize_fp8(w)
                if act:
                    w = ops.interleave_gate_up(w)
                    q = ops.interleave_gate_up(q.view(torch.uint8)).view(torch.float8_e4m3fn)
                    s = ops.interleave_gate_up(s)
                s16.append(w), s8.append(q), ssc.append(s)
                del w
            w16.append(s16), w8.append(s8), sc.append(ssc)
        p16 = [ptrs(s) for s in w16]
        p8 = [ptrs(s) for s in w8]
        ps = [ptrs(s) for s in sc]
        for split, counts in SPLITS.items():
            assert sum(counts) == R
            off = torch.tensor([0] + torch.tensor(counts).cumsum(0).tolist(), dtype=torch.int32, device="cuda")
            hint = R // E
            if act:  # gate/up: token matrix + gather, rows written in place
                x = (torch.randn(M, K, device="cuda", generator=g) * 0.5).bfloat16()
                a_rows = torch.arange(M, device="cuda").repeat(TOPK)[torch.randperm(R, device="cuda", generator=g)].int()
                out = torch.empty(R, NO, device="cuda", dtype=torch.bfloat16)
                kw16 = [dict(act=act, out=out, a_rows=a_rows, w_ptrs=p16[i], rows_hint=hint) for i in range(a.sets)]
                kw8 = [dict(act=act, out=out, a_rows=a_rows, w_ptrs=p8[i], s_ptrs=ps[i], rows_hint=hint)
                       for i in range(a.sets)]
                xs = x.float()[a_rows.long()]
            else:  # down: sorted rows in, compact outputs
                x = (torch.randn(R, K, device="cuda", generator=g) * 0.5).bfloat16()
                outs = [torch.empty(M, NO, device="cuda", dtype=torch.bfloat16) for _ in range(E)]
                po = ptrs(outs)
                kw16 = [dict(outs=outs, out_ptrs=po, w_ptrs=p16[i], rows_hint=hint) for i in range(a.sets)]
                kw8 = [dict(outs=outs, out_ptrs=po, w_ptrs=p8[i], s_ptrs=ps[i], rows_hint=hint) for i in range(a.sets)]
                xs = x.float()
            # correctness (automatic config), group by group against the same e4m3 values
            res = ops.gemm_grouped_w8(x, w8[0], sc[0], off, **kw8[0])
            err, lo = 0.0, 0
            for e, c in enumerate(counts):
                ref = torch.empty(c, N, device="cuda")
                for n0 in range(0, N, 8192):
                    ref[:, n0:n0 + 8192] = (xs[lo:lo + c] @ w8[0][e][n0:n0 + 8192].float().t()) * sc[0][e][n0:n0 + 8192]
                ref = ops._swiglu_interleaved(ref) if act else ref
                got = res[lo:lo + c] if act else res[e][:c]
                err = max(err, ((got.float() - ref).abs().max() / ref.abs().max()).item())
                lo += c
                del ref
            assert err < 2e-2, (name, split, err)

            def f16(i):
                ops.gemm_grouped(x, w16[i % a.sets], off, **kw16[i % a.sets])

            def f8(cfg):
                return lambda i: ops.gemm_grouped_w8(x, w8[i % a.sets], sc[i % a.sets], off, config=cfg, **kw8[i % a.sets])

            reps = 2 * a.sets
            t16, t8 = [], {c: [] for c in [None] + list(range(ncfg))}
            for _ in range(a.rounds):  # same-box pairs: bf16, then every fp8 config, alternating
                for c in t8:
                    t16.append(tuning._graph_time(f16, reps=reps))
                    t8[c].append(tuning._graph_time(f8(c), reps=reps))
            b16 = statistics.median(t16)
            b8 = {c: statistics.median(v) for c, v in t8.items()}
            auto = int(ops.ext().gemm_w8_grouped_pick(hint, N, K, E))
            line = (f"{name:8s} {split:9s} {b16:8.1f} {b8[None]:8.1f} {b8[None] / b16:8.2f} {'c%d' % auto:>5s} "
                    + " ".join(f"{b8[c]:11.1f}" for c in range(ncfg))
                    + f" {E * N * K * 2 / b16 / 1e6:9.2f} {E * N * K / b8[None] / 1e6:8.2f} {err:8.1e}")
            print(line, flush=True)
            lines.append(line)
        del w16, w8, sc
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("grouped fp8-weight GEMM vs bf16 grouped GEMM, Mixtral-8x7B expert shapes, 8 groups over 1024 routed\n"
                    "rows, cold weights (us per launch, median of alternating same-device rounds; c<i>(<tile rows>):\n"
                    "config i of the fp8 kernel; weight TB/s = the 8 experts' weight bytes / time)\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
