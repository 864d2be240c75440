#!/usr/bin/env python3
"""Decode attention (ops.attention_decode, csrc/kernels/attn_decode.hip) against the path the tree
had for it: ``ops.attention(..., Sq=T, q_off=P)`` with the launcher's choice (variant 0) and the
key-split variant 14, on the same K/V bytes. Shapes: Llama-3-8B (32/8 heads, D 128) and GPT-2
(12/12, D 64), B in {1, 8}, T in {1, 4, 16}, a context of P keys before the step (the cache
capacity is C = P + T, so the caches are also the prefill kernel's [B*S] key rows).

Protocol: the three kernels alternate on one device, --rounds times; every figure is the median
device time per call of a hipGraph of calls (ops.tuning._graph_time), and every call of a graph
reads another of --sets copies of the caches, more than the 256 MB Infinity Cache in total where
16 copies reach that. Every result is checked against the fp32 reference of ops first. The
table also gives the kernel's K/V bytes over its time, next to a device-to-device copy of 1 GB.

    python benchmarks/bench_decode.py [--rounds 3] [--out FILE] [--step] [--kv-dtype fp8]

--kv-dtype fp8: the table is instead the fp8 attn_decode (csrc/kernels/attn_decode_fp8.hip: e4m3
caches, one scale per position and KV head) next to the bf16 attn_decode on the same shapes, in
alternating pairs with the same protocol (each kernel cycles through enough copies of ITS caches to
pass the Infinity Cache), plus kv_append in both forms. Exit status 2 if fp8 is not the faster in
every pair at llama3-8b, B 8, T 1, P 8192.

--step adds the decode step of llama3-8b-1l (one hipGraph) with its breakdown per kernel GROUP of
the program (benchmarks/decode_step.py: event pairs, not a per-kernel trace — the attention group's
QKV GEMM, kv_append, attn_decode and out-projection are one figure). Needs a GPU: there is no fallback.
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

MODELS = {"llama3-8b": (32, 8, 128, (512, 8192)), "gpt2": (12, 12, 64, (512, 1008))}
DEV = "cuda"


def copy_rate():
    """TB/s (bytes read + bytes written) of a 1 GB device-to-device copy."""
    src = torch.empty(1 << 28, dtype=torch.float32, device=DEV).normal_()
    dst = torch.empty_like(src)
    us = tuning._graph_time(lambda i: dst.copy_(src), reps=4)
    return 2 * src.numel() * 4 / us / 1e6


def bench_shape(model, B, T, P, rounds, max_sets=16):
    nh, nkv, D, _ = MODELS[model]
    C = P + T
    E = nkv * D
    kv_bytes = 2 * B * C * E * 2
    sets = max(2, min(max_sets, -(-(512 << 20) // kv_bytes)))
    g = torch.Generator(device=DEV).manual_seed(1)
    caches = [(torch.randn(B, C, E, device=DEV, generator=g).bfloat16(),
               torch.randn(B, C, E, device=DEV, generator=g).bfloat16()) for _ in range(sets)]
    q = torch.randn(B * T, nh * D, device=DEV, generator=g).bfloat16()
    pos = torch.full((B,), P, dtype=torch.int32, device=DEV)
    ws = ops.attention_decode_workspace(B, T, C, nh, nkv, D, DEV)
    out = torch.empty(B * T, nh * D, dtype=torch.bfloat16, device=DEV)

    def dec(i):
        kc, vc = caches[i % sets]
        return ops.attention_decode(q, kc, vc, pos, T, nh, nkv, D, out=out, workspace=ws)

    def old(variant):
        def f(i):
            kc, vc = caches[i % sets]
            return ops.ext().attention(q, kc.view(B * C, E), vc.view(B * C, E), B, C, nh, nkv, D, True, D ** -0.5, out,
                                       variant, T, P, 0)
        return f

    ref = ops.ref_attention(q, caches[0][0].view(B * C, E), caches[0][1].view(B * C, E), B, C, nh, nkv, D, True,
                            Sq=T, q_off=P).float().cpu()  # fp32 torch on the device: the check, not a timed path
    for what, f in (("attn_decode", dec), ("variant 0", old(0)), ("variant 14", old(14))):
        err = ((f(0).float().cpu() - ref).abs().max() / ref.abs().max()).item()
        assert err < 2e-2, (what, model, B, T, P, err)
    reps = max(4, sets)
    t = {"dec": [], "v0": [], "v14": []}
    for _ in range(rounds):  # same-device triples, alternating
        t["dec"].append(tuning._graph_time(dec, reps=reps))
        t["v0"].append(tuning._graph_time(old(0), reps=reps))
        t["v14"].append(tuning._graph_time(old(14), reps=reps))
    med = {k: statistics.median(v) for k, v in t.items()}
    best_old = [min(a, b) for a, b in zip(t["v0"], t["v14"])]
    faster = all(d < o for d, o in zip(t["dec"], best_old))
    chunk = ops.ext().attention_decode_chunk(B, C, nkv, D)
    return (f"{model:10s} {B:2d} {T:3d} {P:5d} {chunk:6d} {-(-C // chunk) * nkv * B:6d} {med['dec']:9.1f} "
            f"{med['v0']:9.1f} {med['v14']:9.1f} {min(med['v0'], med['v14']) / med['dec']:7.2f} "
            f"{'yes' if faster else 'NO':>10s} {kv_bytes / med['dec'] / 1e6:8.2f} {sets:4d}"), faster


def bench_shape_fp8(model, B, T, P, rounds, max_sets=16):
    """One row: fp8 against bf16 attn_decode, and kv_append in both forms."""
    nh, nkv, D, _ = MODELS[model]
    C = P + T
    E = nkv * D
    bytes16, bytes8 = 2 * B * C * E * 2, 2 * B * C * nkv * (D + 4)
    sets16 = max(2, min(max_sets, -(-(512 << 20) // bytes16)))
    sets8 = max(2, min(max_sets, -(-(512 << 20) // bytes8)))
    g = torch.Generator(device=DEV).manual_seed(1)
    c16, c8 = [], []
    for i in range(max(sets16, sets8)):
        kv = [torch.randn(B, C, E, device=DEV, generator=g).bfloat16() for _ in range(2)]
        if i < sets8:
            qs = [ops.quantize_fp8(x.view(B * C * nkv, D)) for x in kv]
            c8.append(tuple(q.view(torch.uint8).view(B, C, E) for q, _ in qs)
                      + tuple(s.view(B, C, nkv).transpose(1, 2).contiguous() for _, s in qs))
        if i < sets16:
            c16.append(tuple(kv))
    q = torch.randn(B * T, nh * D, device=DEV, generator=g).bfloat16()
    new = torch.randn(B * T, (nh + 2 * nkv) * D, device=DEV, generator=g).bfloat16()
    k_new, v_new = new[:, nh * D:(nh + nkv) * D], new[:, (nh + nkv) * D:]
    pos = torch.full((B,), P, dtype=torch.int32, device=DEV)
    ws = ops.attention_decode_workspace(B, T, C, nh, nkv, D, DEV)
    out = torch.empty(B * T, nh * D, dtype=torch.bfloat16, device=DEV)

    def dec16(i):
        kc, vc = c16[i % sets16]
        return ops.attention_decode(q, kc, vc, pos, T, nh, nkv, D, out=out, workspace=ws)

    def dec8(i):
        kc, vc, ks, vs = c8[i % sets8]
        return ops.attention_decode(q, kc, vc, pos, T, nh, nkv, D, out=out, workspace=ws, k_scale=ks, v_scale=vs)

    def app16(i):
        kc, vc = c16[i % sets16]
        ops.kv_append(k_new, v_new, kc, vc, pos, T)

    def app8(i):
        kc, vc, ks, vs = c8[i % sets8]
        ops.kv_append(k_new, v_new, kc, vc, pos, T, k_scale=ks, v_scale=vs)

    for what, f, (kc, vc) in (("bf16", dec16, c16[0]),
                              ("fp8", dec8, (ops.kv_dequantize(c8[0][0], c8[0][2]), ops.kv_dequantize(c8[0][1], c8[0][3])))):
        ref = ops.ref_attention(q, kc.view(B * C, E), vc.view(B * C, E), B, C, nh, nkv, D, True, Sq=T,
                                q_off=P).float().cpu()  # fp32 torch on the device: the check, not a timed path
        err = ((f(0).float().cpu() - ref).abs().max() / ref.abs().max()).item()
        assert err < 2e-2, (what, model, B, T, P, err)
        del ref, kc, vc
    t = {"d16": [], "d8": [], "a16": [], "a8": []}
    for _ in range(rounds):  # same-device pairs, alternating
        t["d16"].append(tuning._graph_time(dec16, reps=max(4, sets16)))
        t["d8"].append(tuning._graph_time(dec8, reps=max(4, sets8)))
        t["a16"].append(tuning._graph_time(app16, reps=max(4, sets16)))
        t["a8"].append(tuning._graph_time(app8, reps=max(4, sets8)))
    med = {k: statistics.median(v) for k, v in t.items()}
    faster = all(a < b for a, b in zip(t["d8"], t["d16"]))
    return (f"{model:10s} {B:2d} {T:3d} {P:5d} {med['d16']:9.1f} {med['d8']:9.1f} {med['d16'] / med['d8']:7.2f} "
            f"{'yes' if faster else 'NO':>10s} {bytes16 / med['d16'] / 1e6:9.2f} {bytes8 / med['d8'] / 1e6:8.2f} "
            f"{med['a16']:9.1f} {med['a8']:9.1f} {sets16:3d}/{sets8:<3d}"), faster


def main_fp8(a, shapes):
    head = (f"{'model':10s} {'B':>2s} {'T':>3s} {'P':>5s} {'bf16 us':>9s} {'fp8 us':>9s} {'speedup':>7s} {'every pair':>10s} "
            f"{'bf16 TB/s':>9s} {'fp8 TB/s':>8s} {'app16 us':>9s} {'app8 us':>9s} {'sets':>7s}")
    lines = [head]
    print(head, flush=True)
    gate = None
    for m, B, T, P in shapes:
        line, faster = bench_shape_fp8(m, B, T, P, a.rounds)
        if (m, B, T, P) == ("llama3-8b", 8, 1, 8192):
            gate = faster
        print(line, flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    tail = [f"device-to-device copy of 1 GB (read + write): {copy_rate():.2f} TB/s",
            "speedup: bf16 attn_decode over fp8 attn_decode (medians); every pair: fp8 was the faster in every "
            "alternating round; TB/s: the kernel's own K/V bytes (fp8: bytes and scales) over its time; app: kv_append",
            f"pass condition (llama3-8b, B 8, T 1, P 8192, fp8 faster in every pair): "
            f"{'not measured' if gate is None else 'met' if gate else 'NOT met'}"]
    for x in tail:
        print(x, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("fp8 against bf16 decode attention, us per call, median of alternating same-device rounds\n"
                    + "\n".join(lines + tail) + "\n")
    if gate is False:
        sys.exit(2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="model,B,T,P: one shape")
    ap.add_argument("--step", action="store_true", help="also the llama3-8b-1l decode step and its breakdown per kernel group")
    ap.add_argument("--kv-dtype", default="bf16", choices=["bf16", "fp8"],
                    help="fp8: the fp8 attn_decode and kv_append next to the bf16 ones")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_decode.py needs a GPU")
    if a.kv_dtype == "fp8":
        if a.only:
            m, B, T, P = a.only.split(",")
            return main_fp8(a, [(m, int(B), int(T), int(P))])
        return main_fp8(a, [(m, B, T, P) for m in MODELS for P in MODELS[m][3] for B in (1, 8) for T in (1, 4, 16)])
    head = (f"{'model':10s} {'B':>2s} {'T':>3s} {'P':>5s} {'chunk':>6s} {'blocks':>6s} {'decode us':>9s} {'v0 us':>9s} "
            f"{'v14 us':>9s} {'speedup':>7s} {'every pair':>10s} {'KV TB/s':>8s} {'sets':>4s}")
    lines = [head]
    print(head, flush=True)
    if a.only:
        m, B, T, P = a.only.split(",")
        shapes = [(m, int(B), int(T), int(P))]
    else:
        shapes = [(m, B, T, P) for m in MODELS for P in MODELS[m][3] for B in (1, 8) for T in (1, 4, 16)]
    gate = None
    for m, B, T, P in shapes:
        line, faster = bench_shape(m, B, T, P, a.rounds)
        if (m, B, T, P) == ("llama3-8b", 1, 1, 8192):
            gate = faster
        print(line, flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    cr = copy_rate()
    tail = [f"device-to-device copy of 1 GB (read + write): {cr:.2f} TB/s",
            "speedup: the faster of variants 0 and 14 over attn_decode (medians); every pair: attn_decode was the "
            "faster in every alternating round",
            f"pass condition (llama3-8b, B 1, T 1, P 8192, faster in every pair): "
            f"{'not measured' if gate is None else 'met' if gate else 'NOT met'}"]
    for x in tail:
        print(x, flush=True)
    if a.step:
        from benchmarks.decode_step import step_breakdown  # noqa: E402
        tail += [""] + step_breakdown()
        print("\n".join(tail[tail.index(""):]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("decode attention against ops.attention(Sq=T, q_off=P), us per call, median of alternating "
                    "same-device rounds\n" + "\n".join(lines + tail) + "\n")
    if gate is False:
        sys.exit(2)


if __name__ == "__main__":
    main()
