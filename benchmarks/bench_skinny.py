#!/usr/bin/env python3
"""The dense skinny GEMM (ops.linear_skinny, csrc/kernels/gemm_skinny.hip) against the path a decode
step takes without it: ``ops.linear`` / ``ops.linear_norm`` on the same operands with the config the
tuning table gives them. Shapes: the dense GEMMs of a Llama-3-8B layer and its LM head (QKV with
RoPE, wo + residual, gate/up SwiGLU, down + residual, LM head) and of GPT-2 (QKV with a folded
LayerNorm, out-projection + residual, fc1 with a folded LayerNorm + GELU, fc2 + residual, the LM
head with a folded LayerNorm), M in {1, 2, 4, 8, 16}, every W in {4, 8, 16}, streaming (nt) and
default-policy weight loads.

Protocol (that of bench_decode.py): the kernels alternate on one device, --rounds times; every
figure is the median device time per call of a hipGraph of calls (ops.tuning._graph_time), and call
i of a graph reads copy i % n of the weight, n the fewest copies that pass 512 MB (the Infinity
Cache is 256 MB), so no call finds its weight cached. Both outputs are checked against the fp32
reference first. The tiles run the config the parent's executor would (it tunes a shape its table
lacks at setup: tuning.ensure_tuned). "every pair": the skinny launch the executor issues — W of
ops.skinny_waves, default-policy loads — was the faster in every alternating round.

    python benchmarks/bench_skinny.py [--rounds 3] [--only llama|gpt2] [--m 1,2,4,8,16] [--out DIR]

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
# (model, name, N, K, kind): kind in rope / res / swiglu / ln / ln_gelu / lmhead / ln_lmhead
SHAPES = [
    ("llama3-8b-1l", "qkv+rope", 6144, 4096, "rope"), ("llama3-8b-1l", "wo+res", 4096, 4096, "res"),
    ("llama3-8b-1l", "gate/up", 28672, 4096, "swiglu"), ("llama3-8b-1l", "down+res", 4096, 14336, "res"),
    ("llama3-8b-1l", "lm head", 128256, 4096, "lmhead"),
    ("gpt2", "qkv ln", 2304, 768, "ln"), ("gpt2", "proj+res", 768, 768, "bias_res"),
    ("gpt2", "fc1 ln gelu", 3072, 768, "ln_gelu"), ("gpt2", "fc2+res", 768, 3072, "bias_res"),
    ("gpt2", "lm head ln", 50257, 768, "ln_lmhead"),
]
VARIANTS = [(W, nt) for W in ops.SKINNY_WAVES for nt in (False, True)]


def operands(N, K, M, kind):
    g = torch.Generator(device=DEV).manual_seed(N + K + M)
    n = max(1, -(-int(PASS_BYTES) // (N * K * 2)))
    ws = [torch.empty(N, K, dtype=BF, device=DEV).normal_(0, 0.02, generator=g) for _ in range(n)]
    x = (torch.randn(M, K, device=DEV, generator=g) + 0.3).to(BF)
    n_out = N // 2 if kind == "swiglu" else N
    ld = -(-n_out // 64) * 64  # the executor's rows are padded (50257 -> 50304)
    kw = {}
    if kind in ("res", "bias_res"):
        kw["residual"] = torch.randn(M, n_out, device=DEV, generator=g).to(BF)
    if kind.startswith("ln") or kind == "bias_res":
        kw["bias"] = (0.1 * torch.randn(N, device=DEV, generator=g)).to(BF)
    if kind == "swiglu":
        kw["act"] = "swiglu"
    if kind == "ln_gelu":
        kw["act"] = "gelu"
    if kind == "rope":
        D, cols = 128, 40 * 128
        pos = torch.arange(M, device=DEV)[:, None].double() + 500
        inv = 1.0 / (500000.0 ** (torch.arange(0, D, 2, device=DEV).double() / D))
        kw["rope"] = ((pos * inv).cos().float().contiguous(), (pos * inv).sin().float().contiguous(), M, D, cols)
    norm = None
    if kind.startswith("ln"):
        norm = ((ws[0].float().sum(1)).contiguous(), "layernorm", 1e-5)  # colsum of copy 0: timing only needs [N] floats
    outs = [torch.empty(M, ld, dtype=BF, device=DEV)[:, :n_out] for _ in range(2)]
    return ws, x, kw, norm, outs


def reference(x, w, kw, norm):
    return ops._ref_linear_skinny(x.cpu(), w.cpu(), kw["bias"].cpu() if "bias" in kw else None, ops.ACT[kw.get("act")],
                                  kw["residual"].cpu() if "residual" in kw else None, 1.0,
                                  tuple(t.cpu() if torch.is_tensor(t) else t for t in kw["rope"]) if "rope" in kw else None,
                                  (norm[0].cpu(),) + norm[1:] if norm else None).float()


def bench_shape(model, name, N, K, kind, Ms, rounds):
    tuning.set_model(model)
    stream_exec = False  # the executor's policy (DLS_SKINNY_STREAM): default loads, nt measured slower
    lines, wins = [], {}
    for M in Ms:
        ws, x, kw, norm, outs = operands(N, K, M, kind)
        n = len(ws)

        def old(i, o=outs[0]):
            w = ws[i % n]
            if norm is not None:
                ops.linear_norm(x, w, norm[0], kw.get("bias"), norm[1], norm[2], act=kw.get("act"), out=o)
            else:
                ops.linear(x, w, kw.get("bias"), act=kw.get("act"), residual=kw.get("residual"), out=o, rope=kw.get("rope"))

        def new(W, nt, o=outs[1]):
            def f(i):
                ops.linear_skinny(x, ws[i % n], norm=norm, out=o, waves=W, stream=nt, **kw)
            return f

        # the tiles with the config the parent's executor would run: it tunes a shape its table lacks at setup
        tuning.ensure_tuned([(M, N, K, tuning.tag(ops.ACT[kw.get("act")]))], torch.device("cuda:0"))
        ref = reference(x, ws[0], kw, norm)
        scale = ref.abs().max().item()
        old(0)
        assert (outs[0].float().cpu() - ref).abs().max().item() < 2e-2 * scale, (name, M, "tiles")
        for W, nt in VARIANTS:
            outs[1].fill_(float("nan"))
            new(W, nt)(0)
            assert (outs[1].float().cpu() - ref).abs().max().item() < 2e-2 * scale, (name, M, W, nt)
        reps = max(4, min(n, 512))
        t = {"old": []}
        t.update({v: [] for v in VARIANTS})
        for _ in range(rounds):  # same-device, alternating
            t["old"].append(tuning._graph_time(old, reps=reps))
            for v in VARIANTS:
                t[v].append(tuning._graph_time(new(*v), reps=reps))
        med = {k: statistics.median(v) for k, v in t.items()}
        auto = (ops.skinny_waves(N, K, kw.get("act")), stream_exec)
        every = all(a < b for a, b in zip(t[auto], t["old"]))
        wins[M] = every
        best = min(VARIANTS, key=lambda v: med[v])
        wb = N * K * 2
        cells = " ".join(f"{med[v]:7.1f}" for v in VARIANTS)
        lines.append(f"{model:13s} {name:12s} {M:3d} {med['old']:8.1f} {cells}  W{auto[0]:<2d}{'nt' if auto[1] else '  '} "
                     f"{med[auto]:7.1f} {med['old'] / med[auto]:6.2f} {'yes' if every else 'NO':>5s} "
                     f"{wb / med['old'] / 1e6:6.2f} {wb / med[auto] / 1e6:6.2f}  W{best[0]:<2d}{'nt' if best[1] else '  '} "
                     f"{wb / 1e6:8.1f}")
        print(lines[-1], flush=True)
        del ws, x, kw, norm, outs
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
        sys.exit("bench_skinny.py needs a GPU")
    Ms = [int(v) for v in a.m.split(",")]
    head = (f"{'model':13s} {'gemm':12s} {'M':>3s} {'tiles us':>8s} " + " ".join(
        f"{'W' + str(W) + ('nt' if nt else ''):>7s}" for W, nt in VARIANTS) +
        f"  {'auto':5s} {'us':>7s} {'x':>6s} {'every':>5s} {'TB/s t':>6s} {'TB/s s':>6s}  {'best':5s} {'MB':>8s}")
    print(head, flush=True)
    lines, lm = [head], {}
    for model, name, N, K, kind in SHAPES:
        if a.only and not model.startswith(a.only):
            continue
        ls, wins = bench_shape(model, name, N, K, kind, Ms, a.rounds)
        lines += ls
        if "lmhead" in kind:
            lm[model] = wins
    tail = ["tiles: ops.linear / ops.linear_norm with the tuned config; W4 .. W16nt: ops.linear_skinny with that many waves "
            "and default / streaming weight loads, us per call (medians of alternating rounds); auto: the launch the "
            "executor issues (W of ops.skinny_waves, default-policy loads), x = tiles / auto, every: "
            "auto was the faster in every round; TB/s: weight bytes over the time (t tiles, s auto); best: the fastest "
            "variant's W and policy",
            "LM-head rows, auto faster in every pair: " + "; ".join(
                f"{m}: " + ", ".join(f"M {k} {'yes' if v else 'NO'}" for k, v in w.items()) for m, w in lm.items())]
    for x in tail:
        print(x, flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "kernels.txt"), "w") as f:
            f.write("\n".join(lines + tail) + "\n")


if __name__ == "__main__":
    main()
