#!/usr/bin/env python3
"""Flagship benchmark: GPT-2 operator DAG placed by the scheduler onto N MI355X GPUs and
executed by the native executor (HIP kernels, RCCL p2p for cross-GPU edges).

Metric (BASELINE.json): "DAG makespan (ms) + tasks completed under mem cap, GPT-2 DAG at
1/2/4/8 MI355X". One step = executing the whole placed DAG once: N request replicas of
the reference's GPT-2-small DAG (99 tasks each, batch 1 x 512 tokens — test_gpt2.py:53),
random-init bf16 weights, synthetic token ids. Weak scaling: one 512-token request per GPU.
``value`` is the step makespan in ms (max over ranks); lower is better.

A plain run does only what that figure needs: it sets up, warms up, times the steps, writes the
step's outputs if ``--dump-outputs DIR`` is given, and prints the line. With ``--full`` the
same JSON line also carries:
  * ``capped``: the reference's experiment (simulation.py:161-192, 375-376: regime 0.8, its
    0.5 GB-per-parameter cost model, schedulers.py:404-442 eviction) EXECUTED — ONE GPT-2 DAG
    spread over the N GPUs with the reference's node memory split, for MRU_spec, EFT and DFS:
    tasks completed (reference at N = 1/2/4/8: MRU_spec 99, DFS 81/79/74/66), cross-GPU edges
    and bytes, parameter bytes re-filled per step, measured ms per step; at N > 1 also
    ``capped_replica`` (one request per GPU, each capped at 80 % of one DAG's need);
  * ``strong``: strong scaling with real cross-GPU DAG edges — a fixed batch of 8 GPT-2
    micro-batches pipeline-placed over the N GPUs (contiguous layer blocks; every block
    boundary an RCCL p2p send/recv): ms per step, cross-GPU edges and bytes.
Every line carries ``rccl_world`` and ``per_rank_ms`` of the headline run.

    python bench.py --gpus N --steps K --warmup W      # N > 1: starts its own N rank processes
    python bench.py --full                              # ... plus the capped / strong sub-results
    python bench.py --dump-outputs DIR                  # the last timed step's outputs as DIR/<name>.npy
    python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...
    python bench.py --model gpt2-medium --gpus 2 --cap-gb 8 --replicas 1          # one DAG across 2 GPUs
    python bench.py --model mixtral-8x7b --gpus 8 --placement expert               # DP attention + experts over 8 GPUs
    DLS_P2P=device python bench.py --gpus N ...   # cross-GPU edges moved by kernels (parallel/devp2p.py)
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import sys
import threading
import time

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402

METRIC = "DAG makespan (ms) + tasks completed under mem cap, GPT-2 DAG at 1/2/4/8 MI355X"


def log(*a):
    print(*a, file=sys.stderr, flush=True)


class Ctx:
    def __init__(self, world, rank, device, gpu, pg):
        self.world, self.rank, self.device, self.gpu, self.pg = world, rank, device, gpu, pg

    def sync(self):
        if self.gpu:
            torch.cuda.synchronize(self.device)
        if self.world > 1:
            dist.barrier()

    def gather_list(self, v: float):
        return self.gather(v)[1]

    def gather(self, v: float):
        """(max over ranks, per-rank list) of a host float."""
        if self.world == 1:
            return v, [v]
        t = torch.tensor([v], dtype=torch.float64, device=self.device if self.gpu else "cpu")
        outs = [torch.zeros_like(t) for _ in range(self.world)]
        dist.all_gather(outs, t)
        vals = [float(o.item()) for o in outs]
        return max(vals), vals


def regime_cap_gb(model, regime, batch, seq, cost_model) -> float:
    """Per-GPU cap = regime x the reference's total need of ONE request DAG
    (simulation.py:194-214 under the reference cost model; real bytes otherwise)."""
    from distributed_llm_scheduler_amd.eval.simulation import ImprovedSchedulerEvaluator
    from distributed_llm_scheduler_amd.models import registry
    from distributed_llm_scheduler_amd.models.params import group_layout

    tasks1, groups1, _ = registry.build(model, batch=batch, seq=seq, cost_model=cost_model)
    if cost_model == "reference":
        need = ImprovedSchedulerEvaluator({}).calculate_total_memory_needed(tasks1)
    else:
        gb = {pid: group_layout(g)[0] / 1e9 for pid, g in groups1.items()}
        need = max(t.memory_required + sum(gb[q] for q in t.params_needed) for t in tasks1) + sum(gb.values())
    return round(need * regime, 6)


def _cache_policy() -> dict:
    """The cache policies the step's kernels ran with (ops: DLS_LMHEAD_POL / DLS_ACT_POL /
    DLS_ATTN_FLAGS): stream_pol bits 1 weight DMA nt, 2 output stores nt, 4 write-through;
    attention flags bit 0 write-through stores, bit 1 XCD-grouped blocks."""
    from distributed_llm_scheduler_amd import ops
    return {"lm_head": ops.LMHEAD_POL, "gemm": ops.ACT_POL, "attention_flags": ops.ATTN_FLAGS}


DUMP_BUDGET_BYTES = 48 << 20  # all files of one --dump-outputs run, over all ranks (limit: 64 MB)
DUMP_SEED = 20240229


def dump_outputs(plan, ex, out_dir: str) -> list:
    """``--dump-outputs``: what the step just run hands its caller — the output of every task of
    the DAG that no other task consumes (each request's logits), as this rank holds it — written
    as ``out_dir/<task id, "/" as ".">.npy`` in float32. An output larger than its share of the
    byte budget is written as a fixed sample of its elements (flat indices drawn once from a
    seeded generator, sorted), the same from run to run and from build to build."""
    import numpy as np

    consumed = {d for t in plan.tasks for d in t.dependencies}
    names = [t.id for t in plan.tasks if t.id not in consumed]
    if not names:
        return []
    os.makedirs(out_dir, exist_ok=True)
    share = max(1, DUMP_BUDGET_BYTES // 4 // len(names))  # float32 elements per output
    written = []
    for name in names:
        if not ex.owns_output(name):
            continue  # another rank's output (or a task the memory cap left unplaced)
        v = ex.output(name).detach().reshape(-1)
        if v.numel() > share:
            g = torch.Generator().manual_seed(DUMP_SEED)
            idx = torch.randint(0, v.numel(), (share,), generator=g).sort().values
            v = v[idx.to(v.device)]
        path = os.path.join(out_dir, name.replace("/", ".") + ".npy")
        np.save(path, v.float().cpu().numpy())
        written.append(path)
    return written


def launch_ranks(n: int) -> int:
    """``python bench.py --gpus N`` without a launcher: start N rank processes of this script
    (fresh children — nothing here has touched the GPU), one per GPU, rendezvous on 127.0.0.1;
    rank 0 prints the JSON line. Any rank failing ends the job with its exit code."""
    import socket
    import subprocess

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env))
    rc = 0
    live = list(procs)
    while live:
        for p in list(live):
            code = p.poll()
            if code is None:
                continue
            live.remove(p)
            if code != 0 and rc == 0:
                rc = code
                log(f"[bench] rank {procs.index(p)} exited with {code}; stopping the other ranks")
                for q in live:
                    q.terminate()
        time.sleep(0.05)
    return rc


def run(ctx: Ctx, steps: int, warmup: int, *, model, scheduler, cap_gb, replicas, batch, seq, cost_model,
        placement, tp=1, sp=1, fuse=True, use_graph=True, init="auto", refine=False, roctx=False,
        profile=False, trace_out=None, tag="", node_speeds=None, merge_mb=1, transport=None,
        dump_dir=None) -> dict:
    """Plan, build the rank's executor, warm up, time ``steps`` steps bracketed by a barrier +
    device synchronize on both sides; the step time is the MAX over ranks."""
    t0 = time.time()
    plan = runtime.plan(model, world=ctx.world, scheduler=scheduler, cap_gb=cap_gb, replicas=replicas, batch=batch,
                        seq=seq, cost_model=cost_model, fuse=fuse, placement=placement, tp=tp, sp=sp,
                        node_speeds=node_speeds, merge_mb=merge_mb)
    log(f"[bench{tag}] rank {ctx.rank}: planned {plan.stats['tasks_completed']}/{plan.stats['tasks_total']} tasks in "
        f"{(time.time() - t0) * 1e3:.1f} ms; {plan.stats}")
    dev_init = init == "device" or (init == "auto" and ctx.gpu and runtime.device_init_ok(plan, ctx.rank))
    store = runtime.make_store(plan, device_init=dev_init)
    t0 = time.time()
    # DLS_P2P=device (or transport="device"): cross-GPU edges moved by kernels, IPC-mapped peers
    pg = runtime.p2p_group(plan, ctx.rank, ctx.device, ctx.pg, transport) if ctx.gpu else ctx.pg
    ex = runtime.make_executor(plan, ctx.rank, ctx.device, store, pg=pg, use_graph=use_graph, trace=roctx)
    log(f"[bench{tag}] rank {ctx.rank}: executor ready in {(time.time() - t0):.1f} s (device_init={dev_init})")
    # one eager step first (lazy initialisation, first-step weight transforms; what the capture
    # records), then the W warmup steps run the step exactly as it is timed — the captured
    # hipGraph when there is one — so the GPU enters the timed window in its steady state
    # (W eager steps left it idle behind the Python issue loop: 20 timed steps after them
    # measured 0.620-0.628 ms against 0.605 ms for 200, profiles/r6_status/short_window.txt)
    ex.step()
    ctx.sync()
    # expert-parallel capacity edges whose routing overflowed: widened on both of their ranks,
    # then the step runs again (repeat: a corrected layer can change a later layer's routing)
    ep_widened = 0
    while runtime.ep_widen_on_overflow(ex, ctx.pg):
        ep_widened += 1
        ex.step()
    ctx.sync()
    captured = ex.capture() if use_graph else False
    if captured and refine:
        log(f"[bench{tag}] rank {ctx.rank}: in-DAG GEMM refinement: {ex.refine_tuning()}")
    for _ in range(warmup):
        ex.step()
    ctx.sync()
    ex.reset_transport_errors()  # device transport: a cold first step may outlast a peer's wait
    log(f"[bench{tag}] rank {ctx.rank}: warmup done ({warmup} steps, hipGraph={captured})")

    ctx.sync()
    t_start = time.perf_counter()
    for _ in range(steps):
        ex.step()
    ctx.sync()
    elapsed = time.perf_counter() - t_start
    mine = elapsed / steps * 1e3
    ms, per_rank = ctx.gather(mine)
    launches = ctx.gather_list(ex.launches if ex.launches is not None else -1)
    p2p_err = ctx.gather_list(ex.transport_errors())  # a timed-out device-transport wait: numbers invalid
    ep_over = ctx.gather_list(len(ex.ep_overflow()))  # capacity overflow inside the timed steps
    st = plan.stats
    res = {
        "ms_per_step": round(ms, 5),
        "per_rank_ms": [round(v, 5) for v in per_rank],
        "tasks_completed": st["tasks_completed"],
        "tasks_total": st["tasks_total"],
        "scheduler": plan.scheduler_name,
        "cross_gpu_edges": st["cross_gpu_edges"],
        "cross_gpu_bytes": st["cross_gpu_bytes"],
        "cross_gpu_bytes_routed": st.get("cross_gpu_bytes_routed", st["cross_gpu_bytes"]),
        "cross_gpu_transfers": st.get("cross_gpu_transfers"),
        "modelled_period_ms": st.get("modelled_period_ms"),
        "tasks_per_rank": st.get("tasks_per_rank"),
        "kernel_groups_per_rank": st["kernels_per_rank"],
        # kernel launches of one step on this rank (counted in the captured hipGraphs; None if eager)
        "launches_per_rank": [None if v < 0 else int(v) for v in launches],
        "refill_gb_per_step": round(sum(st["refill_gb_per_step_per_rank"]), 6),
        "peer_fill_gb_per_step": round(sum(st.get("peer_fill_gb_per_step_per_rank", [0.0])), 6),
        "param_loads_per_step": sum(1 for i in plan.programs[ctx.rank].instrs if i.op == "load"),
        "param_evictions_per_step": sum(1 for i in plan.programs[ctx.rank].instrs if i.op == "evict"),
        "hip_graph": bool(captured),
        # segment-replayed programs (p2p or copy-stream refills): native runner or Python loop
        "issue_mode": ex.issue_mode or ("graph" if captured else "python"),
        "p2p": getattr(getattr(ex, "comm", None), "kind", None),
        "p2p_errors": [int(v) for v in p2p_err],
        # expert-parallel capacity edges (program.plan_ep_capacity): widening rounds after warm-up,
        # and groups that overflowed inside the timed steps (non-zero: those outputs were wrong)
        "ep_widened_rounds": ep_widened,
        "ep_overflow": [int(v) for v in ep_over],
        "cross_gpu_bytes_rccl": st.get("cross_gpu_bytes_rccl"),
    }
    if dump_dir:
        log(f"[bench{tag}] rank {ctx.rank}: outputs of the last timed step: {dump_outputs(plan, ex, dump_dir)}")
    if profile or trace_out:
        s = ex.step(profile=True)
        if trace_out:
            from distributed_llm_scheduler_amd.utils.tracing import chrome_trace
            evs = [None] * ctx.world
            if ctx.world > 1:
                dist.all_gather_object(evs, s.events)
            else:
                evs = [s.events]
            if ctx.rank == 0:
                chrome_trace(dict(enumerate(evs)), trace_out,
                             meta={"model": model, "scheduler": plan.scheduler_name, "world": ctx.world})
        if profile:
            res["timeline_ms"] = [(tid, round(a, 4), round(b, 4)) for tid, a, b in s.timeline]
    del ex, store, plan
    gc.collect()
    if ctx.gpu:
        torch.cuda.synchronize(ctx.device)
        torch.cuda.empty_cache()
    ctx.sync()
    return res


DEVICE_P2P_KEYS = ("ms_per_step", "per_rank_ms", "hip_graph", "launches_per_rank", "p2p_errors", "cross_gpu_bytes")


def device_p2p_child(ctx: Ctx, args) -> None:
    """``--device-p2p-child``: one rank of the isolated strong device-p2p sub-run (started by
    :func:`run_device_p2p_children`); rank 0 prints the sub-result as one JSON line."""
    merge = args.strong_mb if args.strong_merge else 1
    if os.environ.get("DLS_TEST_CHILD_ABORT") == str(ctx.rank):
        os.abort()  # (tests: a child that dies as a GPU fault would end it)
    try:
        r = run(ctx, args.extra_steps, min(args.warmup, 2), model=args.model, batch=args.batch, seq=args.seq,
                fuse=not args.no_fuse, use_graph=not args.no_graph, scheduler="EFT", cap_gb=288.0,
                replicas=args.strong_mb, cost_model="bytes", placement="pipeline", tag=":strong-devp2p",
                merge_mb=merge, transport="device" if ctx.gpu else None)
        out = {k: r[k] for k in DEVICE_P2P_KEYS}
    except Exception as e:  # noqa: BLE001 — reported to the parent, which records it
        log(f"[bench] rank {ctx.rank}: device-p2p child failed: {e!r}")
        out = {"error": repr(e)[:300]}
    if ctx.rank == 0:
        print(json.dumps(out), flush=True)
    if ctx.world > 1:
        dist.destroy_process_group()


def run_device_p2p_children(ctx: Ctx, budget_s: float):
    """Every rank starts one child process of this script in ``--device-p2p-child`` mode — the
    children form a job of their own (a fresh rendezvous port from rank 0) — and waits for it
    at most ``budget_s`` seconds. Returns rank 0's child's sub-result (None on other ranks); a
    child that crashes, or a job that does not finish in time, becomes an ``error`` entry."""
    import socket
    import subprocess

    if budget_s < 30:
        raise RuntimeError(f"no time left for the isolated sub-run ({budget_s:.0f} s)")
    port = [0]
    if ctx.rank == 0:
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port[0] = s.getsockname()[1]
        s.close()
    dist.broadcast_object_list(port, src=0)
    if ctx.gpu:
        torch.cuda.synchronize(ctx.device)
        gc.collect()
        torch.cuda.empty_cache()  # the parent's cached blocks: HBM the child may need
    # (torchrun's agent-store variables would make the children's rank 0 a CLIENT of a store
    # that does not exist on the new port)
    env = {k: v for k, v in os.environ.items() if not k.startswith("TORCHELASTIC_")}
    env.update(RANK=str(ctx.rank), WORLD_SIZE=str(ctx.world), MASTER_PORT=str(port[0]),
               MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"))
    argv = [a for a in sys.argv[1:] if a != "--device-p2p-child"]
    err, out = None, ""
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *argv, "--device-p2p-child"], env=env,
                           stdout=subprocess.PIPE, text=True, timeout=budget_s)
        out = r.stdout or ""
        if r.returncode != 0:
            err = f"child exited {r.returncode}"
    except subprocess.TimeoutExpired:
        err = f"child unfinished after {budget_s:.0f} s"
    bad = ctx.gather_list(1.0 if err else 0.0)
    ctx.sync()
    if ctx.rank != 0:
        return None
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    res = json.loads(lines[-1]) if lines else {}
    if err or any(bad):
        res.setdefault("error", err or f"child failed on rank(s) {[i for i, b in enumerate(bad) if b]}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--model", default="gpt2")
    ap.add_argument("--scheduler", default="EFT")
    ap.add_argument("--replicas", type=int, default=None,
                    help="request DAGs in the step, any R >= 1 (default: one per GPU x --replicas-per-gpu); "
                         "R < N places ONE request's DAG across several GPUs")
    ap.add_argument("--replicas-per-gpu", type=int, default=1)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--cap-gb", type=float, default=288.0, help="per-GPU HBM budget for parameters")
    ap.add_argument("--regime", type=float, default=None,
                    help="memory regime instead of --cap-gb: each GPU's cap is regime x the reference's total "
                         "need of one request DAG (simulation.py:194-214), e.g. 0.8 = the paper's 80%% experiments")
    ap.add_argument("--cost-model", default="bytes", choices=["bytes", "reference"],
                    help="planning cost model: real tensor bytes, or the reference's 0.5 GB per parameter "
                         "(memory-regime experiments: e.g. gpt2-medium under an 8 GB cap forces evict/reload)")
    ap.add_argument("--placement", default="scheduler",
                    choices=["scheduler", "replica", "pipeline", "tensor", "sequence", "expert"])
    ap.add_argument("--tp", type=int, default=1, help="tensor-parallel shards per layer (DAG transform)")
    ap.add_argument("--sp", type=int, default=1, help="sequence chunks per request (context-parallel DAG transform)")
    ap.add_argument("--init", default="auto", choices=["auto", "host", "device"],
                    help="weight init: device RNG straight into HBM, or host master copy (auto: device "
                         "unless the program re-fills groups in the steady state, whose cost must be a real copy)")
    ap.add_argument("--refine-tuning", action="store_true",
                    help="before timing, pick GEMM configs by whole-step hipGraph time (persists ops/gemm_tuning.json)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--no-fuse", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the capped / strong sub-results (off by default: a "
                         "plain run measures the headline only)")
    ap.add_argument("--no-extras", action="store_true",
                    help="headline only: the default, kept for older command lines (overrides --full)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the outputs of the last one (every request's logits; "
                         "a fixed seeded sample of an output too large for the 64 MB limit) as DIR/<name>.npy")
    ap.add_argument("--extra-steps", type=int, default=10, help="timed steps of each capped / strong sub-run")
    ap.add_argument("--strong-mb", type=int, default=8, help="micro-batches of the strong-scaling pipeline run")
    ap.add_argument("--no-strong-merge", dest="strong_merge", action="store_false",
                    help="run the strong sub-result's micro-batches as separate M = 512 chains (not merged)")
    ap.add_argument("--no-device-p2p-extra", dest="device_p2p_extra", action="store_false",
                    help="N > 1: skip the strong sub-result repeated over the device p2p transport")
    ap.add_argument("--device-p2p-extra-cpu", action="store_true",
                    help="(tests) run the isolated device-p2p sub-run's plumbing on CPU ranks too (gloo, the "
                         "strong pipeline over the host transport)")
    ap.add_argument("--device-p2p-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--merge-mb", type=int, default=1,
                    help="headline: merge this many request replicas into one batched request (plan merge_mb)")
    ap.add_argument("--extras-timeout", type=float, default=180.0,
                    help="seconds the capped / strong sub-results may take before the headline is printed without them")
    ap.add_argument("--profile", action="store_true", help="also print a measured per-kernel timeline")
    ap.add_argument("--trace-out", default=None, help="write a measured Chrome trace (all ranks) to this path")
    ap.add_argument("--roctx", action="store_true", help="roctx range per DAG instruction (rocprofv3 --marker-trace)")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        visible = torch.cuda.device_count()  # (counting devices does not initialise the GPU)
        if 0 < visible < args.gpus:
            log(f"[bench] --gpus {args.gpus} but only {visible} GPU(s) are visible")
            sys.exit(2)
        sys.exit(launch_ranks(args.gpus))  # one rank process per GPU, before any GPU call
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log(f"[bench] --gpus {args.gpus} but the job has WORLD_SIZE={world} ranks; refusing to report n_gpus={world}")
        sys.exit(2)
    gpu = torch.cuda.is_available()
    device = torch.device(f"cuda:{local}") if gpu else torch.device("cpu")
    if gpu:
        torch.cuda.set_device(device)
    pg = None
    if world > 1:
        from distributed_llm_scheduler_amd.parallel.comm import init_world

        init_world(rank, world, device if gpu else None)  # RCCL bound to this GPU + one barrier
        pg = dist.group.WORLD
    ctx = Ctx(world, rank, device, gpu, pg)
    if args.device_p2p_child:
        device_p2p_child(ctx, args)
        return

    replicas = args.replicas if args.replicas is not None else world * args.replicas_per_gpu
    if replicas < 1:
        raise SystemExit("--replicas must be >= 1")
    if args.regime is not None:
        args.cap_gb = regime_cap_gb(args.model, args.regime, args.batch, args.seq, args.cost_model)
        log(f"[bench] regime {args.regime}: per-GPU cap {args.cap_gb} GB ({args.cost_model} cost model)")
    common = dict(model=args.model, batch=args.batch, seq=args.seq, fuse=not args.no_fuse,
                  use_graph=not args.no_graph)
    head = run(ctx, args.steps, args.warmup, scheduler=args.scheduler, cap_gb=args.cap_gb, replicas=replicas,
               cost_model=args.cost_model, placement=args.placement, tp=args.tp, sp=args.sp, init=args.init,
               merge_mb=args.merge_mb, dump_dir=args.dump_outputs,
               refine=args.refine_tuning, roctx=args.roctx, profile=args.profile, trace_out=args.trace_out, **common)

    emitted = threading.Lock()  # ONE line per job: whichever of the main thread / watchdog gets it

    def emit(extras):
        if not emitted.acquire(blocking=False):
            return False
        if rank == 0:
            try:
                line = json.dumps(result(head, extras))
            except (RuntimeError, TypeError, ValueError):  # sub-results mutating under the watchdog
                line = json.dumps(result(head, {"extras_error": extras.get("extras_error", "sub-results unreadable")}))
            print(line, flush=True)
        return True

    def result(head, extras):
        ms = head["ms_per_step"]
        tokens = replicas * args.batch * args.seq
        pname = head["scheduler"] if args.placement == "scheduler" else args.placement
        out = {
            "metric": METRIC,
            "value": ms,
            "unit": "ms",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms,
            "higher_is_better": False,
            "scaling": "weak" if args.replicas is None else "strong",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic tokens, random-init weights",
            "config": {"model": {"gpt2": "gpt2-small"}.get(args.model, args.model),
                       "global_batch": replicas * args.batch, "seq_len": args.seq,
                       "parallelism": f"dag-placement x{world} ({pname}"
                                      f"{f', tp{args.tp}' if args.tp > 1 else ''}{f', sp{args.sp}' if args.sp > 1 else ''}"
                                      f", {replicas} request DAGs)"},
            "tasks_completed": head["tasks_completed"],
            "tasks_total": head["tasks_total"],
            "mem_cap_gb_per_gpu": args.cap_gb,
            "memory_regime": args.regime,
            "refill_gb_per_step": head["refill_gb_per_step"],
            "cost_model": args.cost_model,
            "param_loads_per_step": head["param_loads_per_step"],  # 0 re-fills when all resident
            "param_evictions_per_step": head["param_evictions_per_step"],
            "scheduler": head["scheduler"],
            "tokens_per_s": round(tokens / (ms / 1e3), 1),
            "kernel_groups_per_rank": head["kernel_groups_per_rank"],
            "launches_per_rank": head["launches_per_rank"],
            "cross_gpu_edges": head["cross_gpu_edges"],
            "cross_gpu_bytes": head["cross_gpu_bytes"],
            "cross_gpu_bytes_routed": head["cross_gpu_bytes_routed"],
            "p2p_transport": head["p2p"] or "none",
            # device transport: every rank's error word after the timed steps (non-zero: a wait
            # gave up, the step's numbers are wrong and ``valid`` is false)
            "p2p_errors": head["p2p_errors"],
            "valid": not any(head["p2p_errors"]) and not any(head["ep_overflow"]),
            "cross_gpu_bytes_rccl": head["cross_gpu_bytes_rccl"],
            "rccl_world": dist.get_world_size() if dist.is_initialized() else 1,
            "per_rank_ms": head["per_rank_ms"],
            "hip_graph": head["hip_graph"],
            "issue_mode": head["issue_mode"],
            "cache_policy": _cache_policy(),
            "weights": "random-init",
            "baseline_note": "vs_baseline is null: the reference only simulates (abstract seconds from per-task "
                             "constants, dependency-free makespan; BASELINE.md), so it has no wall-clock number in "
                             "these units. Its comparable outputs are tasks completed under a memory regime "
                             "(GPT-2, N=1, 80%: MRU_spec 99/99, DFS/Greedy/Critical 81/99) — see capped.",
            "scheduler_note": "headline placement by EFT (this framework's transfer- and memory-aware policy); at "
                              "288 GB per GPU every policy places each request on its own GPU identically. "
                              "capped.MRU_spec is the reference's policy under its own 80% regime.",
            **extras,
        }
        if "timeline_ms" in head:
            out["timeline_ms"] = head["timeline_ms"]
        return out

    extras = {}
    # The sub-results must never cost the headline: if they have not finished within
    # --extras-timeout seconds (a multi-GPU sub-run stuck in a collective, say), every rank's
    # watchdog fires — rank 0 prints the headline line with the extras marked unfinished and
    # each rank exits (os._exit: no collective teardown that could block on a stuck peer).
    done = threading.Event()

    def watchdog():
        if not done.wait(args.extras_timeout):
            log(f"[bench] rank {rank}: sub-results unfinished after {args.extras_timeout} s; exiting")
            if emit({**extras, "extras_error": f"sub-results unfinished after {args.extras_timeout} s"}):
                sys.stdout.flush()
                sys.stderr.flush()
                os._exit(0)

    t_extras = time.time()
    full = args.full and not args.no_extras
    if full:
        threading.Thread(target=watchdog, daemon=True).start()
    if full:
        ew = min(args.warmup, 2)
        # the reference's experiment (simulation.py:161-192, 375-376), executed: ONE request DAG
        # spread over the N GPUs under its 80 % memory regime — the regime's memory split over the
        # nodes as the reference splits it (60/40 at 2, 35/25/25/15 at 4, equal at 8), its
        # 0.5 GB-per-parameter cost model; cross-GPU DAG edges are RCCL p2p transfers
        from distributed_llm_scheduler_amd.eval.execute import regime_node_spec
        nodes = regime_node_spec(args.model, 0.8, world, args.batch, args.seq)
        capped = {"memory_regime": 0.8, "cost_model": "reference", "replicas": 1,
                  "mem_cap_gb_per_gpu": [round(m, 6) for m, _ in nodes], "node_speeds": [round(v, 4) for _, v in nodes]}
        extras["capped"] = capped
        keys = ("tasks_completed", "tasks_total", "ms_per_step", "refill_gb_per_step", "peer_fill_gb_per_step",
                "param_loads_per_step", "param_evictions_per_step", "cross_gpu_edges", "cross_gpu_bytes",
                "cross_gpu_transfers", "tasks_per_rank", "modelled_period_ms", "issue_mode")
        for sched in ("MRU_spec", "EFT", "DFS"):
            try:
                r = run(ctx, args.extra_steps, ew, scheduler=sched, cap_gb=[m for m, _ in nodes], replicas=1,
                        node_speeds=[v for _, v in nodes], cost_model="reference", placement="scheduler",
                        tag=f":capped-{sched}", **common)
            except Exception as e:  # noqa: BLE001 — recorded in the JSON line, the headline stands
                log(f"[bench] capped {sched} failed: {e!r}")
                capped[sched] = {"error": repr(e)[:300]}
                continue
            capped[sched] = {k: r[k] for k in keys}
        if world > 1:
            # one request per GPU, each GPU capped at 80 % of one request DAG's need
            cap80 = regime_cap_gb(args.model, 0.8, args.batch, args.seq, "reference")
            cr = {"memory_regime": 0.8, "cost_model": "reference", "replicas": world, "mem_cap_gb_per_gpu": cap80}
            extras["capped_replica"] = cr
            for sched in ("MRU_spec", "EFT", "DFS"):
                try:
                    r = run(ctx, args.extra_steps, ew, scheduler=sched, cap_gb=cap80, replicas=world,
                            cost_model="reference", placement="scheduler", tag=f":capped_replica-{sched}", **common)
                except Exception as e:  # noqa: BLE001
                    log(f"[bench] capped_replica {sched} failed: {e!r}")
                    cr[sched] = {"error": repr(e)[:300]}
                    continue
                cr[sched] = {k: r[k] for k in keys}
        # strong scaling with real cross-GPU edges: a fixed batch of micro-batches, pipeline
        # placement over the N GPUs (at N = 1: the same batch on one GPU)
        # the micro-batches are merged into one batch before placement (plan merge_mb): every
        # stage runs each op ONCE over all 8 x 512 rows, and consecutive steps overlap through
        # the stages; stages are balanced by measured kernel time (runtime.pipeline_stages)
        merge = args.strong_mb if args.strong_merge else 1
        strong = {"micro_batches": args.strong_mb, "placement": f"pipeline over {world} GPU(s)", "scaling": "strong",
                  "tokens_per_step": args.strong_mb * args.batch * args.seq, "micro_batches_merged": merge}
        extras["strong"] = strong
        try:
            r = run(ctx, args.extra_steps, ew, scheduler="EFT", cap_gb=288.0, replicas=args.strong_mb,
                    cost_model="bytes", placement="pipeline", tag=":strong", merge_mb=merge, **common)
            strong.update({k: r[k] for k in ("ms_per_step", "per_rank_ms", "tasks_completed", "tasks_total",
                                             "cross_gpu_edges", "cross_gpu_bytes", "hip_graph",
                                             "kernel_groups_per_rank", "launches_per_rank")})
        except Exception as e:  # noqa: BLE001
            log(f"[bench] strong sub-run failed: {e!r}")
            strong["error"] = repr(e)[:300]
        if world > 1 and (gpu or args.device_p2p_extra_cpu) and args.device_p2p_extra:
            # the same strong pipeline with its edges moved by kernels (parallel/devp2p.py): each
            # rank's whole step ONE hipGraph; peers' arenas mapped over xGMI through IPC handles.
            # Never yet run across GPUs: it runs in CHILD processes (one per rank, a job of their
            # own), so a fault there costs this sub-result, not the headline line
            sd = {"transport": "device", "micro_batches": args.strong_mb, "micro_batches_merged": merge,
                  "isolated": True}
            extras["strong_device_p2p"] = sd
            budget = args.extras_timeout - (time.time() - t_extras) - 20.0
            try:
                r = run_device_p2p_children(ctx, budget)
                if r is not None:  # rank 0
                    sd.update(r)
                    if "p2p_errors" in r:
                        sd["valid"] = not any(r["p2p_errors"])
            except Exception as e:  # noqa: BLE001
                log(f"[bench] strong device-p2p sub-run failed: {e!r}")
                sd["error"] = repr(e)[:300]

    if world > 1:
        dist.barrier()
    done.set()
    emit(extras)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
