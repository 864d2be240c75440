#!/usr/bin/env python3
"""Grouped MXFP4 x fp8 GEMM (ops.gemm_grouped_w4a8, csrc/kernels/gemm_w4a8_grouped.hip) against the
bf16 grouped GEMM (ops.gemm_grouped with the shipped tuning table) and the grouped fp8-weight GEMM
(ops.gemm_grouped_w8) on Mixtral-8x7B's expert shapes: gate/up (N 28672, K 4096, SwiGLU, rows
gathered by a_rows) and down (N 4096, K 14336, compact outputs), 8 groups over 1024 routed rows
split as a real step's routing (one balanced layer, one with a heavy expert). Weights COLD: each
call reads another set of the 8 experts' weights (one bf16 set is 0.9 - 1.9 GB, one MXFP4 set
0.25 - 0.5 GB: --sets rotates over more than the 256 MB Infinity Cache in every format). Every
config of the new kernel next to the picked one; the three kernels alternate on the same device;
the MXFP4 result is checked against the fp32 product of the same dequantised values. Also the two
row-quantiser launches the mode adds per layer, on their own.

    python benchmarks/bench_grouped_w4a8.py [--rounds 3] [--sets 2] [--out FILE]
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
    ncfg = ops.w4a8_grouped_configs()
    head = (f"{'gemm':8s} {'split':9s} {'bf16 us':>8s} {'fp8 us':>8s} {'mx4 us':>8s} {'mx4/bf16':>8s} {'mx4/fp8':>8s} "
            f"{'auto':>5s} " + " ".join(f"{'c%d(%d) us' % (c, ops.w4a8_grouped_tile_rows(c)):>11s}" for c in range(ncfg))
            + f" {'bf16 TB/s':>9s} {'fp8 TB/s':>8s} {'mx4 TB/s':>8s} {'rel err':>8s}")
    lines = [head]
    print(head, flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    for name, N, K, act in GEMMS:
        NO = N // 2 if act else N
        w16, w8, sc8, w4, sc4 = [], [], [], [], []
        for _ in range(a.sets):
            s16, s8, ss8, s4, ss4 = [], [], [], [], []
            for _ in range(E):
                w = (torch.randn(N, K, device="cuda", generator=g) * 0.02).bfloat16()
                q8, c8 = ops.quantize_fp8(w)
                q4, c4 = ops.quantize_mxfp4(w)
                if act:
                    w = ops.interleave_gate_up(w)
                    q8 = ops.interleave_gate_up(q8.view(torch.uint8)).view(torch.float8_e4m3fn)
                    c8 = ops.interleave_gate_up(c8)
                    q4, c4 = ops.interleave_gate_up(q4), ops.interleave_gate_up(c4)
                s16.append(w), s8.append(q8), ss8.append(c8), s4.append(q4.contiguous()), ss4.append(c4.contiguous())
                del w
            w16.append(s16), w8.append(s8), sc8.append(ss8), w4.append(s4), sc4.append(ss4)
        p16, p8, ps8 = [ptrs(s) for s in w16], [ptrs(s) for s in w8], [ptrs(s) for s in sc8]
        p4, ps4 = [ptrs(s) for s in w4], [ptrs(s) for s in sc4]
        for split, counts in SPLITS.items():
            assert sum(counts) == R
            off = torch.tensor([0] + torch.tensor(counts).cumsum(0).tolist(), dtype=torch.int32, device="cuda")
            hint = R // E
            if act:  # gate/up: token matrix + gather, rows written in place
                x = (torch.randn(M, K, device="cuda", generator=g) * 0.5).bfloat16()
                a_rows = torch.arange(M, device="cuda").repeat(TOPK)[torch.randperm(R, device="cuda", generator=g)].int()
                out = torch.empty(R, NO, device="cuda", dtype=torch.bfloat16)
                io = dict(act=act, out=out, a_rows=a_rows, rows_hint=hint)
            else:  # down: sorted rows in, compact outputs
                x = (torch.randn(R, K, device="cuda", generator=g) * 0.5).bfloat16()
                a_rows = None
                outs = [torch.empty(M, NO, device="cuda", dtype=torch.bfloat16) for _ in range(E)]
                io = dict(outs=outs, out_ptrs=ptrs(outs), rows_hint=hint)
            xq, xs = ops.quantize_rows_fp8(x)
            kw16 = [dict(w_ptrs=p16[i], **io) for i in range(a.sets)]
            kw8 = [dict(w_ptrs=p8[i], s_ptrs=ps8[i], **io) for i in range(a.sets)]
            kw4 = [dict(w_ptrs=p4[i], s_ptrs=ps4[i], **io) for i in range(a.sets)]
            # correctness (automatic config), group by group against the same dequantised values
            res = ops.gemm_grouped_w4a8(xq, xs, w4[0], sc4[0], off, **kw4[0])
            xd = xq.float() * xs[:, None]
            xd = xd[a_rows.long()] if act else xd
            err, lo = 0.0, 0
            for e, c in enumerate(counts):
                ref = torch.empty(c, N, device="cuda")
                for n0 in range(0, N, 8192):
                    wd = ops.dequantize_mxfp4(w4[0][e][n0:n0 + 8192], sc4[0][e][n0:n0 + 8192], torch.float32)
                    ref[:, n0:n0 + 8192] = xd[lo:lo + c] @ wd.t()
                    del wd
                ref = ops._swiglu_interleaved(ref) if act else ref
                got = res[lo:lo + c] if act else res[e][:c]
                err = max(err, ((got.float() - ref).abs().max() / ref.abs().max()).item())
                lo += c
                del ref
            assert err < 2e-2, (name, split, err)

            def f16(i):
                ops.gemm_grouped(x, w16[i % a.sets], off, **kw16[i % a.sets])

            def f8(i):
                ops.gemm_grouped_w8(x, w8[i % a.sets], sc8[i % a.sets], off, **kw8[i % a.sets])

            def f4(cfg):
                return lambda i: ops.gemm_grouped_w4a8(xq, xs, w4[i % a.sets], sc4[i % a.sets], off, config=cfg,
                                                       **kw4[i % a.sets])

            reps = 2 * a.sets
            t16, t8, t4 = [], [], {c: [] for c in [None] + list(range(ncfg))}
            for _ in range(a.rounds):  # same-box triples: bf16, fp8, then an MXFP4 config, alternating
                for c in t4:
                    t16.append(tuning._graph_time(f16, reps=reps))
                    t8.append(tuning._graph_time(f8, reps=reps))
                    t4[c].append(tuning._graph_time(f4(c), reps=reps))
            b16, b8 = statistics.median(t16), statistics.median(t8)
            b4 = {c: statistics.median(v) for c, v in t4.items()}
            auto = int(ops.ext().gemm_w4a8_grouped_pick(hint, N, K, E))
            wbytes4 = E * (N * K // 2 + N * K // 32)
            line = (f"{name:8s} {split:9s} {b16:8.1f} {b8:8.1f} {b4[None]:8.1f} {b4[None] / b16:8.2f} "
                    f"{b4[None] / b8:8.2f} {'c%d' % auto:>5s} " + " ".join(f"{b4[c]:11.1f}" for c in range(ncfg))
                    + f" {E * N * K * 2 / b16 / 1e6:9.2f} {E * N * K / b8 / 1e6:8.2f} {wbytes4 / b4[None] / 1e6:8.2f} "
                    f"{err:8.1e}")
            print(line, flush=True)
            lines.append(line)
        del w16, w8, sc8, w4, sc4
        torch.cuda.empty_cache()
    # the two row-quantiser launches the mode adds per MoE layer: the token matrix, the SwiGLU output
    qlines = []
    for what, rows, cols in (("tokens [512, 4096]", M, H), ("moe_h [1024, 14336]", R, F)):
        x = (torch.randn(rows, cols, device="cuda", generator=g) * 0.5).bfloat16()
        oq = torch.empty(rows, cols, dtype=torch.uint8, device="cuda")
        osc = torch.empty(rows, dtype=torch.float32, device="cuda")
        ts = [tuning._graph_time(lambda i: ops.quantize_rows_fp8(x, oq, osc), reps=8) for _ in range(a.rounds)]
        qlines.append(f"quantize_rows_fp8 {what:20s} {statistics.median(ts):8.1f} us")
        print(qlines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("grouped MXFP4 x fp8 GEMM vs the bf16 and the fp8-weight grouped GEMMs, Mixtral-8x7B expert shapes, 8\n"
                    "groups over 1024 routed rows, cold weights (us per launch, median of alternating same-device rounds;\n"
                    "c<i>(<tile rows>): config i of the MXFP4 kernel; weight TB/s = the 8 experts' weight bytes in the\n"
                    "kernel's own format / time)\n")
            f.write("\n".join(lines) + "\n\nthe row quantiser launches the mode adds per MoE layer\n" + "\n".join(qlines) + "\n")


if __name__ == "__main__":
    main()
