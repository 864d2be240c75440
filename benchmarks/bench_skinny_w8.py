#!/usr/bin/env python3
"""The skinny fp8-weight GEMM (ops.linear_skinny_w8, csrc/kernels/gemm_skinny_w8.hip) against the path
a decode step of an fp8-weight plan takes without it: ``ops.linear_w8`` with its automatic config
(tile, split-K slabs in a workspace and the reduce launch), on the same e4m3 weight. Next to both,
the bf16 skinny kernel (ops.linear_skinny) on the dequantised weight: twice the bytes. Shapes: the
dense GEMMs of a Llama-3-8B layer and its LM head and of GPT-2 (bench_skinny.py's table, without the
folded norms and RoPE an fp8 plan runs as launches of their own), M in {1, 2, 4, 8, 16}, every W.

Protocol (that of bench_skinny.py): the kernels alternate on one device, --rounds times; every
figure is the median device time per call of a hipGraph of calls (ops.tuning._graph_time), and call
i of a graph reads copy i % n of the weight, n the fewest fp8 copies that pass 512 MB (the Infinity
Cache is 256 MB; the bf16 copies are as many, twice the bytes), so no call finds its weight cached.
All outputs are checked against the fp32 reference on the dequantised weight first. "every": the
launch the executor issues — W of ops.skinny_w8_waves — was faster than the tiles in every round.

    python benchmarks/bench_skinny_w8.py [--rounds 3] [--only llama|gpt2] [--m 1,2,4,8,16] [--out DIR]

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

DEV = "cuda"
BF = torch.bfloat16
PASS_BYTES = 512e6
# (model, name, N, K, kind): kind in plain / res / bias_res / bias_gelu / swiglu
SHAPES = [
    ("llama3-8b-1l", "qkv", 6144, 4096, "plain"), ("llama3-8b-1l", "wo+res", 4096, 4096, "res"),
    ("llama3-8b-1l", "gate/up", 28672, 4096, "swiglu"), ("llama3-8b-1l", "down+res", 4096, 14336, "res"),
    ("llama3-8b-1l", "lm head", 128256, 4096, "plain"),
    ("gpt2", "qkv", 2304, 768, "bias"), ("gpt2", "proj+res", 768, 768, "bias_res"),
    ("gpt2", "fc1 gelu", 3072, 768, "bias_gelu"), ("gpt2", "fc2+res", 768, 3072, "bias_res"),
    ("gpt2", "lm head", 50257, 768, "plain"),
]


def operands(N, K, M, kind):
    g = torch.Generator(device=DEV).manual_seed(N + K + M)
    n = max(1, -(-int(PASS_BYTES) // (N * K)))
    w0 = torch.empty(N, K, dtype=BF, device=DEV).normal_(0, 0.02, generator=g)
    q0, s = ops.quantize_fp8(w0)
    qs = [q0] + [q0.clone() for _ in range(n - 1)]  # timing only needs n distinct addresses
    wd = ops.dequantize_fp8(q0, s)
    ws = [wd] + [wd.clone() for _ in range(n - 1)]
    x = (torch.randn(M, K, device=DEV, generator=g) + 0.3).to(BF)
    n_out = N // 2 if kind == "swiglu" else N
    ld = -(-n_out // 64) * 64  # the executor's rows are padded (50257 -> 50304)
    kw = {}
    if kind in ("res", "bias_res"):
        kw["residual"] = torch.randn(M, n_out, device=DEV, generator=g).to(BF)
    if kind.startswith("bias"):
        kw["bias"] = (0.1 * torch.randn(N, device=DEV, generator=g)).to(BF)
    if kind == "swiglu":
        kw["act"] = "swiglu"
    if kind == "bias_gelu":
        kw["act"] = "gelu"
    outs = [torch.empty(M, ld, dtype=BF, device=DEV)[:, :n_out] for _ in range(3)]
    return qs, s, ws, x, kw, outs


def bench_shape(model, name, N, K, kind, Ms, rounds):
    tuning.set_model(model)
    lines, wins = [], {}
    for M in Ms:
        qs, s, ws, x, kw, outs = operands(N, K, M, kind)
        n = len(qs)
        need = ops.w8_workspace_elems(M, N, K)  # the executor's split-K slabs, allocated before the capture
        wsp = torch.empty(need, dtype=torch.float32, device=DEV) if need else None

        def old(i, o=outs[0]):
            ops.linear_w8(x, qs[i % n], s, out=o, workspace=wsp, **kw)

        def new(W, o=outs[1]):
            def f(i):
                ops.linear_skinny_w8(x, qs[i % n], s, out=o, waves=W, **kw)
            return f

        def bf(i, o=outs[2]):
            ops.linear_skinny(x, ws[i % n], out=o, **kw)

        ref = ops.ref_linear(x.cpu(), ws[0].cpu(), kw["bias"].cpu() if "bias" in kw else None, kw.get("act"),
                             kw["residual"].cpu() if "residual" in kw else None).float()
        scale = ref.abs().max().item()
        for o in outs:
            o.fill_(float("nan"))
        old(0)
        bf(0)
        for what, o in (("tiles", outs[0]), ("bf16 skinny", outs[2])):
            assert (o.float().cpu() - ref).abs().max().item() < 2e-2 * scale, (name, M, what)
        for W in ops.SKINNY_WAVES:
            outs[1].fill_(float("nan"))
            new(W)(0)
            assert (outs[1].float().cpu() - ref).abs().max().item() < 2e-2 * scale, (name, M, W)
        reps = max(4, min(n, 512))
        t = {"old": [], "bf16": []}
        t.update({W: [] for W in ops.SKINNY_WAVES})
        for _ in range(rounds):  # same-device, alternating
            t["old"].append(tuning._graph_time(old, reps=reps))
            for W in ops.SKINNY_WAVES:
                t[W].append(tuning._graph_time(new(W), reps=reps))
            t["bf16"].append(tuning._graph_time(bf, reps=reps))
        med = {k: statistics.median(v) for k, v in t.items()}
        auto = ops.skinny_w8_waves(N, K, kw.get("act"))
        every = all(a < b for a, b in zip(t[auto], t["old"]))
        wins[M] = every
        best = min(ops.SKINNY_WAVES, key=lambda W: med[W])
        wb = N * K
        cfg, sk = ops.ext().gemm_w8_pick(M, N, K)
        cells = " ".join(f"{med[W]:7.1f}" for W in ops.SKINNY_WAVES)
        lines.append(f"{model:13s} {name:10s} {M:3d} {med['old']:8.1f} c{cfg}k{sk:<2d} {cells}  W{auto:<2d} {med[auto]:7.1f} "
                     f"{med['old'] / med[auto]:6.2f} {'yes' if every else 'NO':>5s} {wb / med['old'] / 1e6:6.2f} "
                     f"{wb / med[auto] / 1e6:6.2f}  W{best:<2d} {med['bf16']:8.1f} {2 * wb / med['bf16'] / 1e6:6.2f} {wb / 1e6:8.1f}")
        print(lines[-1], flush=True)
        del qs, ws, x, kw, outs, wsp
        torch.cuda.empty_cache()
    return lines, wins


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, choices=["llama", "gpt2"])
    ap.add_argument("--m", default="1,2,4,8,16")
    ap.add_argument("--out", default=None, help="directory for kernels.txt")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_skinny_w8.py needs a GPU")
    Ms = [int(v) for v in a.m.split(",")]
    head = (f"{'model':13s} {'gemm':10s} {'M':>3s} {'tiles us':>8s} {'cfg':5s} " + " ".join(
        f"{'W' + str(W):>7s}" for W in ops.SKINNY_WAVES) +
        f"  {'auto':3s} {'us':>7s} {'x':>6s} {'every':>5s} {'TB/s t':>6s} {'TB/s s':>6s}  {'best':3s} {'bf16 us':>8s} {'TB/s b':>6s} {'MB':>8s}")
    print(head, flush=True)
    lines, allwins = [head], {}
    for model, name, N, K, kind in SHAPES:
        if a.only and not model.startswith(a.only):
            continue
        ls, wins = bench_shape(model, name, N, K, kind, Ms, a.rounds)
        lines += ls
        allwins[f"{model} {name}"] = wins
    lost = [f"{k} M {m}" for k, w in allwins.items() for m, v in w.items() if not v]
    tail = ["tiles: ops.linear_w8 with its automatic config (cfg: tile config c, split-K k) and workspace; W4 .. W16: "
            "ops.linear_skinny_w8 with that many waves, us per call (medians of alternating rounds); auto: the launch the "
            "executor issues (W of ops.skinny_w8_waves), x = tiles / auto, every: auto was the faster in every round; TB/s: "
            "fp8 weight bytes over the time (t tiles, s auto); best: the fastest W; bf16: ops.linear_skinny on the "
            "dequantised weight (its automatic W), TB/s b over twice the bytes; MB: fp8 weight bytes",
            "auto NOT faster than the tiles in every round: " + (", ".join(lost) or "none")]
    for x in tail:
        print(x, flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "kernels.txt"), "w") as f:
            f.write("\n".join(lines + tail) + "\n")


if __name__ == "__main__":
    main()
