#!/usr/bin/env python3
"""The skinny grouped expert GEMM (ops.gemm_grouped_skinny, csrc/kernels/gemm_grouped_skinny.hip)
against the path the tree had for a decode step's experts: ``ops.gemm_grouped`` on the same inputs
(the executor's call: rows_hint = R // E). Shapes: Mixtral-8x7B's expert MLP (E 8, top-2, H 4096,
F 14336), M in {1, 4, 8, 16} token rows with uniform random routing, the gate/up launch (SwiGLU,
rows gathered by a_rows) and the down launch (compact outputs) separately.

Protocol (that of bench_decode.py): the two kernels alternate on one device, --rounds times; every
figure is the median device time per call of a hipGraph of calls (ops.tuning._graph_time), and
call i of a graph runs routing i % --sets of as many random routings, so successive calls touch
other experts' weights (one expert's gate/up weight alone is 235 MB, the Infinity Cache 256 MB).
Both outputs are checked against an fp32 product of the routed rows first. The table gives the
routed experts' weight bytes over the skinny kernel's time, next to the 4.07 TB/s attn_decode
reaches on K/V bytes. Exit status 2 if the skinny kernel is not the faster in every pair at an M
where the executor takes it (M <= ops.MOE_SKINNY_MAX_ROWS).

    python benchmarks/bench_moe_decode.py [--rounds 3] [--sets 8] [--out DIR] [--step [--max-rows N]] [--skip-kernels]

--step: the decode step of mixtral-8x7b-1l (runtime.plan moe_decode=True, T 1; B 1 from a context
of 512 and of 8000 positions, B 2, 4, 8, 16 from 8000) as one captured hipGraph with the skinny
launches on and off (executor.MOE_SKINNY), the two graphs alternating. Needs a GPU: there is no fallback.
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

E, TOPK, H, F = 8, 2, 4096, 14336
DEV = "cuda"
ATTN_DECODE_TBS = 4.07


def routings(M, sets, seed):
    """``sets`` uniform random top-2 routings of M tokens: (a_rows, offsets, routed experts)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(sets):
        idx = torch.stack([torch.randperm(E, generator=g)[:TOPK] for _ in range(M)]).to(torch.int32)
        src, _, off = ops.moe_align(idx, E)
        out.append((src.to(DEV), off.to(DEV), int((off[1:] > off[:-1]).sum())))
    return out


def check(x, ws, route, got, act, compact):
    src, off, _ = route
    o = off.tolist()
    rows = x[src.long()] if act else x
    for e in range(E):
        n = o[e + 1] - o[e]
        if not n:
            continue
        ref = ops.ref_linear(rows[o[e]:o[e + 1]], ws[e], act="swiglu" if act else None).float()
        have = (got[e][:n] if compact else got[o[e]:o[e + 1]]).float()
        err = ((have - ref).abs().max() / ref.abs().max().clamp_min(1e-6)).item()
        assert err < 2e-2, (act, e, err)


def bench_m(M, w13, w2, p13, p2, rounds, sets):
    R = M * TOPK
    g = torch.Generator(device=DEV).manual_seed(M)
    x = torch.randn(M, H, device=DEV, generator=g).bfloat16()
    hb = (0.5 * torch.randn(R, F, device=DEV, generator=g)).bfloat16()
    hout = torch.empty(R, F, dtype=torch.bfloat16, device=DEV)
    outs = [torch.empty(M, H, dtype=torch.bfloat16, device=DEV) for _ in range(E)]
    optr = torch.tensor([o.data_ptr() for o in outs], dtype=torch.int64, device=DEV)
    rts = routings(M, sets, 100 + M)
    hint = max(1, R // E)

    def gu(fn, **kw):
        def f(i):
            src, off, _ = rts[i % sets]
            fn(x, w13, off, act="swiglu", out=hout, w_ptrs=p13, a_rows=src, **kw)
        return f

    def dn(fn, **kw):
        def f(i):
            _, off, _ = rts[i % sets]
            fn(hb, w2, off, outs=outs, w_ptrs=p2, out_ptrs=optr, **kw)
        return f

    pairs = {"gate/up": (gu(ops.gemm_grouped_skinny), gu(ops.gemm_grouped, rows_hint=hint), 2 * F * H * 2),
             "down": (dn(ops.gemm_grouped_skinny), dn(ops.gemm_grouped, rows_hint=hint), H * F * 2)}
    for f in pairs["gate/up"][:2]:
        f(0)
        check(x, w13, rts[0], hout, True, False)
    for f in pairs["down"][:2]:
        f(0)
        check(hb, w2, rts[0], outs, False, True)
    lines, ok = [], True
    reps = max(4, sets)
    for what, (new, old, wbytes) in pairs.items():
        t = {"new": [], "old": []}
        for _ in range(rounds):  # same-device pairs, alternating
            t["new"].append(tuning._graph_time(new, reps=reps))
            t["old"].append(tuning._graph_time(old, reps=reps))
        med = {k: statistics.median(v) for k, v in t.items()}
        faster = all(a < b for a, b in zip(t["new"], t["old"]))
        if M <= ops.MOE_SKINNY_MAX_ROWS:
            ok &= faster  # (beyond the bound the executor does not take the skinny kernel)
        routed = statistics.mean(rts[i % sets][2] for i in range(reps)) * wbytes
        lines.append(f"{what:8s} {M:3d} {med['new']:10.1f} {med['old']:10.1f} {med['old'] / med['new']:8.2f} "
                     f"{'yes' if faster else 'NO':>10s} {routed / 1e6:10.1f} {routed / med['new'] / 1e6:10.2f} "
                     f"{routed / med['old'] / 1e6:10.2f}")
    return lines, ok


def kernels(a):
    w13 = [torch.empty(2 * F, H, dtype=torch.bfloat16, device=DEV).normal_(0, 0.02) for _ in range(E)]
    w2 = [torch.empty(H, F, dtype=torch.bfloat16, device=DEV).normal_(0, 0.02) for _ in range(E)]
    mk = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)  # noqa: E731
    p13, p2 = mk(w13), mk(w2)
    head = (f"{'launch':8s} {'M':>3s} {'skinny us':>10s} {'grouped us':>10s} {'speedup':>8s} {'every pair':>10s} "
            f"{'routed MB':>10s} {'skinny TB/s':>10s} {'grouped TB/s':>10s}")
    lines, ok = [head], True
    print(head, flush=True)
    for M in (1, 4, 8, 16):
        ls, good = bench_m(M, w13, w2, p13, p2, a.rounds, a.sets)
        ok &= good
        for ln in ls:
            print(ln, flush=True)
        lines += ls
    tail = ["speedup: ops.gemm_grouped over ops.gemm_grouped_skinny (medians); every pair: the skinny kernel was the "
            "faster in every alternating round; routed MB: weight bytes of the experts with rows, mean over the "
            f"graph's calls; TB/s: those bytes over the kernel's time (attn_decode reaches {ATTN_DECODE_TBS} TB/s on K/V bytes)",
            f"pass condition (skinny faster in every pair where the executor takes it, M <= ops.MOE_SKINNY_MAX_ROWS = "
            f"{ops.MOE_SKINNY_MAX_ROWS}): {'met' if ok else 'NOT met'}"]
    for x in tail:
        print(x, flush=True)
    return lines + tail, ok


def step_ab(model="mixtral-8x7b-1l", C=8192, cases=((1, 1, 512), (1, 1, 8000), (2, 1, 8000), (4, 1, 8000), (8, 1, 8000), (16, 1, 8000)), steps=10, rounds=5):
    from distributed_llm_scheduler_amd.parallel import executor as exm
    from distributed_llm_scheduler_amd.parallel import runtime

    dev = torch.device("cuda:0")
    lines = []
    for B, T, past in cases:
        if B * T > ops.MOE_SKINNY_MAX_ROWS:
            lines.append(f"{model}  B {B}  T {T}: more than ops.MOE_SKINNY_MAX_ROWS = {ops.MOE_SKINNY_MAX_ROWS} token rows, "
                         "the grouped kernels either way")
            print(lines[-1], flush=True)
            continue
        p = runtime.plan(model, world=1, seq=T, batch=B, kv_cache=C, moe_decode=True)
        store = runtime.make_store(p, device_init=runtime.device_init_ok(p, 0))
        exs = {}
        for what, flag in (("off", False), ("on", True)):
            exm.MOE_SKINNY = flag
            ex = runtime.make_executor(p, 0, dev, store)
            ex.kv_randomize(past)
            ex.step()
            ex.kv_reset(past)
            if not ex.capture():
                raise RuntimeError("the decode step was not captured")
            assert len(ex._moe_skinny) == (p.cfg.n_layer if flag else 0)
            exs[what] = ex
        exm.MOE_SKINNY = True

        def timed(ex):
            ex.kv_reset(past)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(steps):
                ex.step()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / steps * 1e3

        t = {"off": [], "on": []}
        for _ in range(rounds):
            for what in ("off", "on"):
                t[what].append(timed(exs[what]))
        med = {k: statistics.median(v) for k, v in t.items()}
        lines.append(f"{model}  B {B}  T {T}  past {past}  cache {C}: {med['off']:.1f} us per step with DLS_MOE_SKINNY=0 "
                     f"(min {min(t['off']):.1f}, max {max(t['off']):.1f}), {med['on']:.1f} us with the skinny "
                     f"{' + '.join(next(iter(exs['on']._moe_skinny.values())))} "
                     f"(min {min(t['on']):.1f}, max {max(t['on']):.1f}): {med['off'] / med['on']:.2f}x, faster in "
                     f"{sum(a < b for a, b in zip(t['on'], t['off']))} of {rounds} rounds; one hipGraph of "
                     f"{exs['on'].launches} launches each, medians of {rounds} alternating rounds of {steps} steps")
        print(lines[-1], flush=True)
        del exs, store
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--out", default=None, help="directory for kernels.txt / step.txt")
    ap.add_argument("--step", action="store_true", help="also the mixtral-8x7b-1l decode step, skinny launches off and on")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--max-rows", type=int, default=None,
                    help="with --step: run it with ops.MOE_SKINNY_MAX_ROWS set to this (a bound search: the default "
                         "measures what the executor does)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_moe_decode.py needs a GPU")
    ok = True
    if a.out:
        os.makedirs(a.out, exist_ok=True)
    if not a.skip_kernels:
        lines, ok = kernels(a)
        if a.out:
            with open(os.path.join(a.out, "kernels.txt"), "w") as f:
                f.write("skinny against grouped expert GEMM, Mixtral-8x7B shapes, us per call, median of alternating "
                        "same-device rounds\n" + "\n".join(lines) + "\n")
        torch.cuda.empty_cache()
    if a.step:
        if a.max_rows is not None:
            ops.MOE_SKINNY_MAX_ROWS = a.max_rows  # (read by the executor at every step)
        lines = step_ab()
        if a.out:
            with open(os.path.join(a.out, "step.txt"), "w") as f:
                f.write("\n".join(lines) + "\n")
    if not ok:
        sys.exit(2)


if __name__ == "__main__":
    main()
