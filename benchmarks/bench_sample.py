#!/usr/bin/env python3
"""The sampling kernel (ops.sample_tokens, csrc/kernels/sample.hip) against a sort-based sampler
composed of torch ops on the same logits and the same draw u: ``torch.sort``, top-k by position,
softmax, ``cumsum``, the top-p mask, ``searchsorted``, ``gather`` (greedy: ``argmax``). Shapes:
V = 128 256 (Llama-3) and 50 257 (GPT-2), B in {1, 8}; greedy, and (temperature 0.8, top_k 50,
top_p 0.9).

Protocol (that of bench_decode.py): the two samplers alternate on one device, --rounds times; every
figure is the median device time per call of a hipGraph of calls (ops.tuning._graph_time), and every
call of a graph reads another of 16 copies of the logits. The kernel is checked first: greedy
tokens against ``argmax``, sampled ones against the CPU path of ops.sample_tokens (same threshold;
Z, the weight before the token and the token's weight to 1e-5 of Z).

    python benchmarks/bench_sample.py [--rounds 3] [--out FILE]

Exit status 2 unless the kernel is the faster in every pair at V = 128 256, B = 1 and B = 8.
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
SETS = 16
MODES = {"greedy": (0.0, 0, 1.0), "t0.8 k50 p0.9": (0.8, 50, 0.9)}
C, POS, SEED = 64, 9, 1234


def torch_sampler(logits, V, tau, k, p, u, out):
    """The composition: one row per sequence, [B][ld] bf16 -> token ids [B]."""
    x = logits[:, :V].float()
    if not tau > 0:
        out.copy_(torch.argmax(x, dim=-1))
        return out
    s, idx = torch.sort(x, dim=-1, descending=True)
    if 0 < k < V:
        s = s[:, :k]
    pr = torch.softmax(s / tau, dim=-1)
    cum = pr.cumsum(-1)
    if p < 1:
        pr = pr * ((cum - pr) < p)
        cum = pr.cumsum(-1)
    j = torch.searchsorted(cum, u[:, None] * cum[:, -1:], right=True).clamp_(max=cum.shape[1] - 1)
    out.copy_(idx.gather(1, j)[:, 0])
    return out


def bench_shape(V, B, mode, rounds):
    tau, k, p = MODES[mode]
    ld = -(-V // 64) * 64
    g = torch.Generator(device=DEV).manual_seed(V + B)
    sets = [(torch.randn(B, ld, device=DEV, generator=g) * 3).bfloat16() for _ in range(SETS)]
    pos = torch.full((B,), POS, dtype=torch.int32, device=DEV)
    stream = torch.zeros(B, C, dtype=torch.int32, device=DEV)
    par = (torch.full((B,), tau, device=DEV), torch.full((B,), k, dtype=torch.int32, device=DEV),
           torch.full((B,), p, device=DEV))
    seed = torch.tensor([SEED], dtype=torch.int64, device=DEV)
    eos = torch.tensor([-1], dtype=torch.int32, device=DEV)
    nxt = torch.zeros(B, dtype=torch.int32, device=DEV)
    stats = torch.zeros(B, 4, device=DEV)
    ws = ops.sample_workspace(B, V, DEV)
    u = torch.tensor([ops.sample_uniform(SEED, 0, b, POS + 1) for b in range(B)], device=DEV)
    tok = torch.zeros(B, dtype=torch.int64, device=DEV)

    def kern(i):
        return ops.sample_tokens(sets[i % SETS], V, 1, pos, stream, C, *par, seed, eos=eos, next_out=nxt, stats=stats,
                                 workspace=ws)

    def comp(i):
        return torch_sampler(sets[i % SETS], V, tau, k, p, u, tok)

    kern(0)
    comp(0)
    torch.cuda.synchronize()
    if not tau > 0:
        assert nxt.tolist() == tok.tolist(), (V, B, nxt.tolist(), tok.tolist())
    else:
        cn, cs = ops.sample_tokens(sets[0].cpu(), V, 1, pos.cpu(), stream.cpu(), C, *(x.cpu() for x in par), SEED)
        gs = stats.cpu()
        assert torch.equal(gs[:, 0], cs[:, 0]), (V, B, gs[:, 0], cs[:, 0])
        same = nxt.cpu() == cn
        scale = cs[:, 1:2]
        assert bool(((gs[:, 1:2] - cs[:, 1:2]).abs() <= 1e-5 * scale).all()) and \
            bool((((gs[:, 2:] - cs[:, 2:]).abs() <= 1e-5 * scale).all(dim=1) | ~same).all()), (V, B, gs, cs)
    t = {"k": [], "t": []}
    for _ in range(rounds):  # same-device pairs, alternating
        t["k"].append(tuning._graph_time(kern, reps=SETS))
        t["t"].append(tuning._graph_time(comp, reps=SETS))
    med = {x: statistics.median(v) for x, v in t.items()}
    faster = all(a < b for a, b in zip(t["k"], t["t"]))
    n_slices = ops.sample_slices(B, V)[0]
    return (f"{V:7d} {B:2d} {mode:14s} {n_slices:6d} {med['k']:9.1f} {med['t']:9.1f} {med['t'] / med['k']:7.2f} "
            f"{'yes' if faster else 'NO':>10s} {B * V * 2 / med['k'] / 1e6:9.3f}"), faster


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_sample.py needs a GPU")
    head = (f"{'V':>7s} {'B':>2s} {'mode':14s} {'slices':>6s} {'kernel us':>9s} {'torch us':>9s} {'speedup':>7s} "
            f"{'every pair':>10s} {'TB/s':>9s}")
    lines = [head]
    print(head, flush=True)
    gate = True
    for V in (128256, 50257):
        for B in (1, 8):
            for mode in MODES:
                line, faster = bench_shape(V, B, mode, a.rounds)
                if V == 128256:
                    gate = gate and faster
                print(line, flush=True)
                lines.append(line)
                torch.cuda.empty_cache()
    tail = ["speedup: the torch composition over the kernel (medians); every pair: the kernel was the faster in every "
            "alternating round; TB/s: the logits bytes of the B rows over the kernel's time (one pass)",
            f"pass condition (V 128256, B 1 and B 8, kernel faster in every pair): {'met' if gate else 'NOT met'}"]
    for x in tail:
        print(x, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("sample_tokens against a sort-based torch sampler, us per call, median of alternating same-device "
                    "rounds\n" + "\n".join(lines + tail) + "\n")
    if not gate:
        sys.exit(2)


if __name__ == "__main__":
    main()
