#!/usr/bin/env python3
"""The e4m3 prompt-chunk attention (csrc/kernels/attn_chunk_fp8.hip) against the path it replaces.

One call of ``ops.attention_chunk`` on fp8 caches, two ways: ``workspace=`` (two
``kv_dequantize_rows`` launches, then the bf16 chunk kernel on the bf16 copy) and ``native=True``
(one launch on the bytes). Llama-3-8B's attention shape (32/8 heads, D 128) at B in {1, 8}, Tc in
{64, 256, 1024} after a prefix of P in {1024, 8192} keys, and GPT-2's (12/12, D 64) at Tc 256;
C = P + Tc. Protocol of bench_prefill.py: every figure is the median device time per call of a
hipGraph of calls, every call of a graph reads another copy of the caches, and the two paths
alternate on one device for --rounds rounds. Next to the difference stands the workspace path's own
round-to-round spread (max - min). ``--layouts`` adds one column per layout of
``ops.CHUNK_FP8_LAYOUTS`` (how the launcher's choice per head_dim was made). The native output is
compared with the workspace path's first (same keys, same arithmetic up to the summation order).

    python benchmarks/bench_chunk_fp8.py [--rounds 5] [--out FILE] [--layouts] [--quick]

Needs a GPU: there is no fallback.
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

MODELS = {"llama3-8b": (32, 8, 128), "gpt2": (12, 12, 64)}
DEV = "cuda"


def bench(model, B, T, P, rounds, layouts, max_sets=16):
    nh, nkv, D = MODELS[model]
    C, E = P + T, nkv * D
    sets = max(2, min(max_sets, -(-(512 << 20) // (2 * B * C * nkv * (D + 4)))))
    g = torch.Generator(device=DEV).manual_seed(1)
    c8 = []
    for _ in range(sets):
        qs = [ops.quantize_fp8(torch.randn(B * C * nkv, D, device=DEV, generator=g).bfloat16()) for _ in range(2)]
        c8.append(tuple(q.view(torch.uint8).view(B, C, E) for q, _ in qs)
                  + tuple(s.view(B, C, nkv).transpose(1, 2).contiguous() for _, s in qs))
    q = torch.randn(B * T, nh * D, device=DEV, generator=g).bfloat16()
    pos = torch.full((B,), P, dtype=torch.int32, device=DEV)
    out = torch.empty(B * T, nh * D, dtype=torch.bfloat16, device=DEV)
    ws = tuple(torch.empty(B, C, E, dtype=torch.bfloat16, device=DEV) for _ in range(2))

    def parent(i):
        kc, vc, ks, vs = c8[i % sets]
        return ops.attention_chunk(q, kc, vc, pos, T, nh, nkv, D, out=out, k_scale=ks, v_scale=vs, workspace=ws)

    def native(layout):
        def f(i):
            kc, vc, ks, vs = c8[i % sets]
            return ops.attention_chunk(q, kc, vc, pos, T, nh, nkv, D, out=out, k_scale=ks, v_scale=vs, native=True,
                                       layout=layout)
        return f

    ref = parent(0).float().clone()
    cols = [0] + [lay for lay in layouts if lay != 14 or D == 64]
    for lay in cols:
        err = ((native(lay)(0).float() - ref).abs().max() / ref.abs().max()).item()
        assert err < 2e-2, (model, B, T, P, lay, err)
    t = {"ws": [], **{lay: [] for lay in cols}}
    reps = max(4, sets)
    for _ in range(rounds):  # same-device rounds, alternating
        t["ws"].append(tuning._graph_time(parent, reps=reps))
        for lay in cols:
            t[lay].append(tuning._graph_time(native(lay), reps=reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    wins = all(n < w for n, w in zip(t[0], t["ws"]))
    line = (f"{model:10s} {B:2d} {T:5d} {P:5d} {med['ws']:10.1f} {max(t['ws']) - min(t['ws']):8.1f} {med[0]:10.1f} "
            f"{med['ws'] - med[0]:8.1f} {med['ws'] / med[0]:7.2f} {'yes' if wins else 'NO':>10s}")
    for lay in layouts:
        line += f" {med[lay]:8.1f}" if lay in med else f" {'-':>8s}"
    return line + f"  {sets}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="file for the table")
    ap.add_argument("--layouts", action="store_true", help="one more column per layout of ops.CHUNK_FP8_LAYOUTS")
    ap.add_argument("--quick", action="store_true", help="B 1, P 8192 only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_chunk_fp8.py needs a GPU")
    layouts = list(ops.CHUNK_FP8_LAYOUTS) if a.layouts else []
    head = (f"{'model':10s} {'B':>2s} {'Tc':>5s} {'P':>5s} {'ws us':>10s} {'ws span':>8s} {'native us':>10s} {'saved us':>8s} "
            f"{'ratio':>7s} {'every pair':>10s}" + "".join(f" {'L' + str(x):>8s}" for x in layouts) + "  sets")
    lines = ["attention_chunk on fp8 caches, us per call, median of alternating same-device rounds", head]
    print(head, flush=True)
    pts = [("llama3-8b", B, T, P) for P in (1024, 8192) for B in (1, 8) for T in (64, 256, 1024)]
    pts += [("gpt2", B, 256, P) for P in (1024, 8192) for B in (1, 8)]
    if a.quick:
        pts = [p for p in pts if p[1] == 1 and p[3] == 8192]
    for m, B, T, P in pts:
        line = bench(m, B, T, P, a.rounds, layouts)
        print(line, flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    lines.append("ws: workspace=(k, v), two kv_dequantize_rows launches plus the bf16 chunk kernel (its K/V come from the ONE "
                 "workspace, which stays in the Infinity Cache between calls); native: native=True, one launch of "
                 "attn_chunk_fp8.hip with the launcher's layout; ws span: max - min of the ws column over the rounds; saved, "
                 "ratio: ws - native, ws / native (medians); every pair: native was the faster in every round; "
                 + ("Lxy: layout 10*NW + KS (NW query tiles x KS key groups per workgroup); " if layouts else "")
                 + "sets: cache copies a graph cycles through.")
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
