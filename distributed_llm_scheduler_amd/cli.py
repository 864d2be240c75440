"""Command-line interface: ``python -m distributed_llm_scheduler_amd <command> ...``

Commands (defaults reproduce the reference's settings where one exists, SURVEY §5 "Config"):

  plan      build a model DAG, place it with a policy, lower to per-GPU programs; print the
            placement statistics, optionally save the plan (``--save``) for ``run --resume``
  run       execute a plan on this machine: one process per GPU under torchrun
            (RANK/WORLD_SIZE from the environment), or one CPU/GPU process; prints the
            measured step makespan; ``--trace`` writes a Chrome trace, ``--gantt`` a PNG;
            ``--loopback N`` runs an N-rank plan in one process (``--transport hub|device``).
            A device-transport wait that timed out makes the run invalid: exit code 3
  simulate  the reference evaluation sweep (raw_results.csv + 2x2 figure); --execute runs each
            policy's placement of a model DAG on the devices (measured makespan column)
  extract   the reference GPT-2 DAG (test_gpt2.py semantics) to JSON (test_gpt2.py also pickles it)
  elastic   run with device-loss injection: a worker dies, the DAG is re-planned onto the
            surviving devices and the step is re-executed
  models    list the model presets
  generate  generate tokens from synthetic prompts on one device: a decode plan whose step ends in
            the sampling launch (``runtime.plan(generate=True)``); prints one JSON line with the
            token ids, the steps and the tokens per second. ``--prefill-chunk Tc``: the prompts are
            consumed in chunk steps of Tc tokens per sequence (``runtime.plan(prefill_chunk=Tc)``); the
            line then also gives the chunk-step count and the time to the first generated token

Common options: --model, --devices (ignored under torchrun: WORLD_SIZE wins), --scheduler,
--hbm-cap-gb, --cost-model {bytes,reference}, --seq, --batch, --replicas, --placement,
--tp, --sp, --seed, --dtype (bf16: the kernels compute in bf16 with fp32 accumulation),
--weight-dtype {bf16,fp8,fp8-experts,mxfp4,mxfp4-experts} (how GEMM weights are STORED: fp8 = e4m3 + one
fp32 scale per output channel, dense models; fp8-experts = the same for the expert weights of an MoE model
only; mxfp4 = OCP MXFP4, e2m1 + one e8m0 scale per 32 elements, dense models, needs --act-dtype fp8;
mxfp4-experts = MXFP4 for the expert weights of an MoE model only, needs --act-dtype fp8),
--act-dtype {bf16,fp8} (fp8, with --weight-dtype fp8, mxfp4 or mxfp4-experts: GEMM inputs quantised per row,
multiplied on the block-scaled MFMA against the fp8 or fp4 weight), --kv-cache C (decode steps: --seq is
the number of new tokens per step and every attention node keeps a KV cache of C positions),
--kv-dtype {bf16,fp8} (with --kv-cache: fp8 = e4m3 cache bytes + one fp32 scale per position and KV head),
--moe-decode (with --kv-cache and an MoE model: decode steps of a Mixtral plan, the expert GEMMs of a step of a
few token rows on the skinny grouped kernel), --skinny-gemm (with --kv-cache and bf16 weights: the dense GEMMs of
a step of a few token rows on the weight-streaming skinny kernel) and, for
``run``, --past P (the caches are filled with random rows to length P before the timed steps).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from typing import List, Optional


def _common(ap: argparse.ArgumentParser) -> None:
    ap.add_argument("--model", default="gpt2")
    ap.add_argument("--devices", type=int, default=1, help="number of GPUs (overridden by WORLD_SIZE)")
    ap.add_argument("--scheduler", default="EFT",
                    help="DFS | Greedy | Critical | MRU_spec | EFT | Greedy_chain | MRU_paper")
    ap.add_argument("--hbm-cap-gb", type=float, default=288.0, help="per-GPU parameter budget (GB)")
    ap.add_argument("--cost-model", choices=["bytes", "reference"], default="bytes",
                    help="bytes: real tensor sizes; reference: 0.5 GB per parameter, constant compute times")
    ap.add_argument("--seq", type=int, default=512)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--replicas", type=int, default=1, help="independent request DAGs (data parallelism)")
    ap.add_argument("--placement", default="scheduler",
                    choices=["scheduler", "replica", "pipeline", "tensor", "sequence"])
    ap.add_argument("--tp", type=int, default=1, help="tensor-parallel shards per layer (DAG transform)")
    ap.add_argument("--sp", type=int, default=1, help="sequence chunks per request (context-parallel DAG transform)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--dtype", default="bf16", choices=["bf16"],
                    help="compute dtype of activations and MFMA operands (bf16, fp32 accumulation); the storage of "
                         "the GEMM weights is selectable with --weight-dtype")
    ap.add_argument("--weight-dtype", default="bf16", choices=["bf16", "fp8", "fp8-experts", "mxfp4", "mxfp4-experts"],
                    help="GEMM weight storage: bf16, or fp8 (OCP e4m3 + one fp32 scale per output channel; dense "
                         "models, no --tp / --sp): about half the parameter bytes under the same --hbm-cap-gb; "
                         "fp8-experts: the same storage for the expert weights of an MoE model (router, attention "
                         "and LM head stay bf16; no --tp / --sp); mxfp4: OCP MXFP4 for the tensors fp8 marks (e2m1 + one "
                         "e8m0 scale per 32 elements, 0.53 bytes per element; dense models, no --tp / --sp, needs "
                         "--act-dtype fp8); mxfp4-experts: MXFP4 for the expert weights of an MoE model (router, "
                         "attention and LM head stay bf16; no --tp / --sp, needs --act-dtype fp8)")
    ap.add_argument("--act-dtype", default="bf16", choices=["bf16", "fp8"],
                    help="GEMM input dtype over quantised weights: bf16 (the W8A16 kernel), or fp8 (needs --weight-dtype "
                         "fp8, mxfp4 or mxfp4-experts: rows quantised to e4m3 with one power-of-two scale each, multiplied on the "
                         "block-scaled MFMA: W8A8 or W4A8)")
    ap.add_argument("--kv-cache", type=int, default=None, metavar="C",
                    help="decode steps: --seq becomes the number of new tokens per step (1 .. 16) and every attention "
                         "node keeps K/V caches of C positions per sequence on its GPU; the caches count against "
                         "--hbm-cap-gb (dense gpt2 / llama models, MoE models with --moe-decode; no --tp / --sp)")
    ap.add_argument("--moe-decode", action="store_true",
                    help="with --kv-cache and an MoE model (bf16 weights): decode steps of the MoE DAG; a step of at "
                         "most ops.MOE_SKINNY_MAX_ROWS token rows (1: one sequence, one token) runs both grouped expert "
                         "launches of every MoE layer on the weight-streaming skinny kernel")
    ap.add_argument("--skinny-gemm", action="store_true",
                    help="with --kv-cache (bf16 weights): the dense GEMMs of a step of at most ops.SKINNY_MAX_ROWS "
                         "token rows run on the weight-streaming skinny kernel (ops.linear_skinny) instead of the "
                         "prefill tiles")
    ap.add_argument("--kv-dtype", default="bf16", choices=["bf16", "fp8"],
                    help="with --kv-cache: how the caches are stored: bf16, or fp8 (OCP e4m3 + one fp32 power-of-two "
                         "scale per position and KV head: (head_dim + 4) / (2 head_dim) of the bf16 bytes)")
    ap.add_argument("--past", type=int, default=0, metavar="P",
                    help="run, with --kv-cache: every sequence starts from a context of P positions of random cache "
                         "rows (the timed steps then run at that length without P / seq steps before them)")
    ap.add_argument("--no-fuse", action="store_true")


def _plan(a, world: int, resume: Optional[str] = None):
    from .parallel import runtime

    return runtime.plan(a.model, world=world, scheduler=a.scheduler, cap_gb=a.hbm_cap_gb, replicas=a.replicas,
                        batch=a.batch, seq=a.seq, cost_model=a.cost_model, fuse=not a.no_fuse,
                        placement=a.placement, tp=a.tp, resume=resume, sp=a.sp, weight_dtype=a.weight_dtype,
                        act_dtype=a.act_dtype, kv_cache=getattr(a, "kv_cache", None),
                        kv_dtype=getattr(a, "kv_dtype", "bf16"), moe_decode=getattr(a, "moe_decode", False),
                        skinny_gemm=getattr(a, "skinny_gemm", False))


def _has_kv(p) -> bool:
    """The plan has KV caches: asked of the plan's arguments, the same answer on every rank."""
    return p.args.get("kv_cache") is not None


def _kv_fields(a, p) -> dict:
    """JSON fields of a plan with KV caches: the capacity, the context the run starts from, the cache bytes."""
    if not _has_kv(p):
        return {}
    return {"kv_cache": a.kv_cache, "past": a.past, "kv_cache_gb": sum(p.kv_cache_bytes) / 1e9,
            "kv_dtype": p.args.get("kv_dtype", "bf16")}


def _kv_check(a, n_steps: int, what: str) -> None:
    """--past P plus the longest run of steps between two resets must fit the cache."""
    if a.past < 0 or a.past + n_steps * a.seq > a.kv_cache:
        raise SystemExit(f"--past {a.past} + {n_steps} steps ({what}) x --seq {a.seq} exceeds --kv-cache {a.kv_cache}")


def _param_gb(p) -> float:
    return round(sum(p.param_bytes.values()) / 1e9, 6)


def cmd_plan(a) -> int:
    from .parallel import runtime

    t0 = time.time()
    p = _plan(a, a.devices)
    out = {"model": a.model, "scheduler": p.scheduler_name, "world": p.world, "plan_ms": round((time.time() - t0) * 1e3, 2),
           "weight_dtype": a.weight_dtype, "act_dtype": a.act_dtype, "param_gb": _param_gb(p)}
    out.update(p.stats)
    out.update(_kv_fields(a, p))
    print(json.dumps(out))
    if a.save:
        runtime.save_plan(p, a.save)
        print(f"saved plan to {a.save}", file=sys.stderr)
    return 0


def _transport_failure(e: BaseException) -> Optional[str]:
    """The TransportError message in ``e`` or its cause chain (a rank thread's error is re-raised
    by the single-GPU harness as the cause of its RuntimeError), else None."""
    from .parallel.executor import TransportError

    while e is not None:
        if isinstance(e, TransportError):
            return str(e)
        e = e.__cause__
    return None


def cmd_run_loopback(a) -> int:
    """``run --loopback N``: the N-rank plan in THIS process on one device (the single-GPU
    multi-rank harness, parallel/loopback.py): every rank its own executor and thread, edges over
    the loopback hub (``--transport hub``, RCCL's p2p semantics) or moved by kernels (``--transport
    device``, parallel/devp2p.py; on the CPU the same protocol with host waits). A device-transport
    wait that gave up makes the run INVALID: the JSON line says so and the exit code is 3."""
    import torch

    from .parallel.loopback import run_loopback

    gpu = a.device != "cpu" and torch.cuda.is_available()
    dev = torch.device("cuda:0") if gpu else torch.device("cpu")
    p = _plan(a, a.loopback, resume=a.resume)
    out = {"model": a.model, "world": a.loopback, "scheduler": p.scheduler_name, "harness": "loopback",
           "transport": a.transport, "tasks_completed": p.stats["tasks_completed"],
           "tasks_total": p.stats["tasks_total"], "device": str(dev), **_kv_fields(a, p)}
    before = None
    if _has_kv(p):
        # the harness never resets: its warm-up steps (and the device transport's dry step on the
        # GPU) extend the context of --past before the timed steps do
        dry = 1 if gpu and a.transport == "device" else 0
        _kv_check(a, dry + a.warmup + a.steps, "dry + warm-up + timed" if dry else "warm-up + timed")

        def before(exs):
            for ex in exs:
                ex.kv_randomize(a.past, seed=a.seed)
    try:
        from .parallel.devp2p import TIMEOUT_S

        run = run_loopback(p, dev, steps=a.steps, warmup=a.warmup, capture=gpu and not a.no_graph,
                           transport=a.transport, delay_us=0.0, poison=False, p2p_timeout_s=TIMEOUT_S,
                           before_steps=before)
        errs = [ex.transport_errors() for ex in run.executors]
        for ex in run.executors:
            ex.check_transport()
    except Exception as e:  # noqa: BLE001
        msg = _transport_failure(e)
        if msg is None:
            raise
        print(json.dumps({**out, "valid": False, "error": msg}))
        print(f"run: INVALID — {msg}", file=sys.stderr)
        return 3
    print(json.dumps({**out, "ms_per_step": round(max(run.step_ms), 4), "p2p_errors": errs, "valid": True}))
    return 0


def cmd_run(a) -> int:
    import torch
    import torch.distributed as dist

    from .parallel import runtime

    if a.loopback:
        return cmd_run_loopback(a)
    world = int(os.environ.get("WORLD_SIZE", a.devices if a.device == "cpu" else 1))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    gpu = a.device != "cpu" and torch.cuda.is_available()
    dev = torch.device(f"cuda:{local}") if gpu else torch.device("cpu")
    if gpu:
        torch.cuda.set_device(dev)
    pg = None
    if world > 1:
        if "MASTER_ADDR" not in os.environ:
            raise SystemExit("world > 1 needs torchrun (or MASTER_ADDR/MASTER_PORT/RANK/WORLD_SIZE)")
        from .parallel.comm import init_world

        init_world(rank, world, dev if gpu else None)
        pg = dist.group.WORLD
    p = _plan(a, world, resume=a.resume)
    store = runtime.make_store(p, seed=a.seed, device_init=gpu and a.init == "device" and runtime.device_init_ok(p, rank))
    if gpu and pg is not None:  # DLS_P2P=device: cross-GPU edges moved by kernels (parallel/devp2p.py)
        pg = runtime.p2p_group(p, rank, dev, pg)
    ex = runtime.make_executor(p, rank, dev, store, pg=pg, use_graph=gpu and not a.no_graph, trace=a.roctx)

    def sync():
        if gpu:
            torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()

    kv = _has_kv(p)  # (every rank takes part, also one that holds no cache)
    if kv:
        # warm-up steps and the profiled step start from --past again, like the timed ones
        _kv_check(a, max(a.steps, 1 if (a.warmup or a.trace or a.gantt) else 0), "timed")
        ex.kv_randomize(a.past, seed=a.seed)
    failed: Optional[str] = None  # a device-transport wait gave up on this rank (TransportError)
    try:
        for _ in range(a.warmup):
            ex.step()
            if kv:
                ex.kv_reset(a.past)  # every warm-up step and the timed ones start from the same context
    except Exception as e:  # noqa: BLE001
        failed = _transport_failure(e)
        if failed is None:
            raise
    sync()
    while failed is None and runtime.ep_widen_on_overflow(ex, dist.group.WORLD if world > 1 else None):
        ex.step()  # expert capacity edges that overflowed: widened, the step runs again
    sync()
    if gpu and not a.no_graph and failed is None:
        ex.capture()
    sync()
    ex.reset_transport_errors()  # a cold first step may outlast a peer's wait (warm-up only)
    t0 = time.perf_counter()
    try:
        for _ in range(a.steps if failed is None else 0):
            ex.step()
    except Exception as e:  # noqa: BLE001
        failed = _transport_failure(e)
        if failed is None:
            raise
    sync()
    ms = (time.perf_counter() - t0) / max(a.steps, 1) * 1e3
    err = ex.transport_errors()
    if err and failed is None:
        failed = ex._transport_msg(err)
    if failed:
        print(f"run: rank {rank}: INVALID — {failed}", file=sys.stderr)
    t = torch.tensor([ms, 1.0 if failed else 0.0], dtype=torch.float64, device=dev if (gpu and world > 1) else "cpu")
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    invalid = bool(t[1].item())
    events = None
    if (a.trace or a.gantt) and not invalid:
        if kv:
            ex.kv_reset(a.past)  # the profiled step sees the context the timed steps started from
        st = ex.step(profile=True)
        events = [None] * world
        if world > 1:
            dist.all_gather_object(events, st.events)
        else:
            events = [st.events]
    if rank == 0:
        print(json.dumps({"model": a.model, "world": world, "scheduler": p.scheduler_name,
                          "tasks_completed": p.stats["tasks_completed"], "tasks_total": p.stats["tasks_total"],
                          "ms_per_step": round(float(t[0].item()), 4), "device": str(dev),
                          "p2p": getattr(ex.comm, "kind", None), "valid": not invalid,
                          "weight_dtype": a.weight_dtype, "act_dtype": a.act_dtype, "param_gb": _param_gb(p),
                          **_kv_fields(a, p)}))
        if events is not None:
            from .utils.tracing import chrome_trace, kernel_timeline

            if a.trace:
                chrome_trace(dict(enumerate(events)), a.trace, meta={"model": a.model, "world": world})
            if a.gantt:
                from .viz.plots import measured_gantt

                measured_gantt({r: kernel_timeline(e) for r, e in enumerate(events)}, path=a.gantt)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return 3 if invalid else 0


def cmd_simulate(a) -> int:
    if a.execute:  # same policies and regimes, the model DAG RUN on this job's devices
        import torch
        import torch.distributed as dist

        from .eval import execute

        world = int(os.environ.get("WORLD_SIZE", "1"))
        gpu = torch.cuda.is_available()
        dev = torch.device(f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}") if gpu else None
        if gpu:
            torch.cuda.set_device(dev)
        if world > 1:
            from .parallel.comm import init_world

            init_world(int(os.environ.get("RANK", "0")), world, dev)
        try:
            execute.main(a.model, a.schedulers.split(",") if a.schedulers else None,
                         tuple(float(x) for x in a.regimes.split(",")), a.steps, a.warmup, a.seq,
                         cost_model=a.cost_model, seed=a.seed, out_dir=a.out, nodes=a.nodes)
        finally:
            if world > 1:
                dist.destroy_process_group()
        return 0
    from .eval.simulation import main as sim_main

    sim_main(num_runs=a.runs, seed=a.seed, out_dir=a.out, engine=a.engine,
             schedulers=a.schedulers.split(",") if a.schedulers else None)
    return 0


def cmd_extract(a) -> int:
    from .models.tracer import LLMDAGExtractor
    from .utils.serialization import save_dag_json

    if not a.model.startswith("gpt2"):
        raise SystemExit("extract supports the GPT-2 family (reference test_gpt2.py semantics)")
    ex = LLMDAGExtractor(a.model)
    tasks = ex.extract_gpt2_dag(batch=a.batch, seq=a.seq, cost_model=a.cost_model)
    ex.analyze_dag(tasks)
    save_dag_json(tasks, a.out)
    print(f"wrote {len(tasks)} tasks to {a.out}")
    return 0


def cmd_elastic(a) -> int:
    from .parallel.elastic import run_elastic

    out = run_elastic(world=a.devices, steps=a.steps, fail_rank=a.fail_rank, fail_step=a.fail_step,
                      device=a.device, model=a.model, scheduler=a.scheduler, cap_gb=a.hbm_cap_gb,
                      replicas=a.replicas, batch=a.batch, seq=a.seq, cost_model=a.cost_model, placement=a.placement,
                      tp=a.tp, sp=a.sp, weight_dtype=a.weight_dtype, act_dtype=a.act_dtype)
    print(json.dumps(out))
    return 0


def cmd_models(a) -> int:
    from .models.config import PRESETS

    for name, c in sorted(PRESETS.items()):
        print(f"{name:14s} family={c.family:8s} layers={c.n_layer:3d} hidden={c.n_embd:5d} heads={c.n_head:3d} "
              f"kv={c.kv_heads:3d} ffn={c.ffn:6d} vocab={c.vocab_size:6d} experts={c.n_experts}")
    return 0


def cmd_generate(a) -> int:
    import torch

    from .parallel import runtime
    from .parallel.executor import synthetic_tokens

    gpu = a.device != "cpu" and torch.cuda.is_available()
    dev = torch.device("cuda:0") if gpu else torch.device("cpu")
    if a.kv_cache is None:
        raise SystemExit("generate needs --kv-cache C")
    if a.prompt_len < 1 or a.new < 1 or a.prompt_len + a.new > a.kv_cache:
        raise SystemExit(f"--prompt-len {a.prompt_len} + --new {a.new} must be positive and fit --kv-cache {a.kv_cache}")
    p = runtime.plan(a.model, world=1, scheduler=a.scheduler, cap_gb=a.hbm_cap_gb, batch=a.batch, seq=1,
                     kv_cache=a.kv_cache, kv_dtype=a.kv_dtype, generate=True, prefill_chunk=a.prefill_chunk,
                     moe_decode=a.moe_decode, skinny_gemm=a.skinny_gemm)
    store = runtime.make_store(p, seed=a.seed, device_init=gpu and runtime.device_init_ok(p, 0))
    ex = runtime.make_executor(p, 0, dev, store, use_graph=gpu and not a.no_graph)
    prompts = synthetic_tokens("@tokens", a.batch * a.prompt_len, p.cfg.vocab_size, a.seed).view(a.batch, -1).tolist()
    ex.set_sampling(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, seed=a.seed)
    ex.set_prompts("@tokens", prompts)
    ex.step()  # (derives weights, tunes nothing new afterwards)
    captured = ex.capture() if gpu and not a.no_graph else False
    first = {}
    if a.prefill_chunk is not None:
        # time to the first generated token: the chunk steps of the prompt plus one token step
        ex.set_prompts("@tokens", prompts)
        if gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        ex.generate(1)
        first = {"prefill_chunk": a.prefill_chunk, "chunk_steps": ex.prefill_steps,
                 "first_token_ms": round((time.perf_counter() - t0) * 1e3, 4)}
    ex.set_prompts("@tokens", prompts)
    if gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    tokens = ex.generate(a.new)
    dt = time.perf_counter() - t0
    steps = a.prompt_len - 1 + a.new if a.prefill_chunk is None else ex.prefill_steps + a.new
    print(json.dumps({"model": a.model, "device": str(dev), "batch": a.batch, "kv_cache": a.kv_cache,
                      "kv_dtype": a.kv_dtype, "prompt_len": a.prompt_len, "new": a.new, "temperature": a.temperature,
                      "top_k": a.top_k, "top_p": a.top_p, "seed": a.seed, "graph": bool(captured), "steps": steps,
                      "step_ms": round(dt / steps * 1e3, 4),
                      "tokens_per_s": round(a.batch * (a.prompt_len - 1 + a.new) / dt, 2), **first,
                      "prompts": prompts, "tokens": tokens}))
    return 0


def main(argv: Optional[List[str]] = None) -> int:
    ap = argparse.ArgumentParser(prog="python -m distributed_llm_scheduler_amd",
                                 description="MI355X-native memory-constrained DAG scheduler + executor")
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("plan", help="place a model DAG and print statistics")
    _common(p)
    p.add_argument("--save", default=None, help="write the plan (placement checkpoint) as JSON")
    p.set_defaults(fn=cmd_plan)
    r = sub.add_parser("run", help="execute a placed DAG (torchrun for several GPUs)")
    _common(r)
    r.add_argument("--device", default="auto", choices=["auto", "cpu"])
    r.add_argument("--steps", type=int, default=10)
    r.add_argument("--warmup", type=int, default=2)
    r.add_argument("--resume", default=None, help="use a plan saved by `plan --save` instead of re-scheduling")
    r.add_argument("--init", default="device", choices=["device", "host"])
    r.add_argument("--no-graph", action="store_true")
    r.add_argument("--roctx", action="store_true")
    r.add_argument("--trace", default=None, help="Chrome trace JSON path")
    r.add_argument("--gantt", default=None, help="measured Gantt PNG path")
    r.add_argument("--loopback", type=int, default=0,
                   help="run an N-rank plan in THIS process on one device (single-GPU multi-rank harness)")
    r.add_argument("--transport", default="hub", choices=["hub", "device"],
                   help="--loopback edges: the loopback hub (RCCL semantics) or kernels (device transport)")
    r.set_defaults(fn=cmd_run)
    s = sub.add_parser("simulate", help="reference evaluation sweep")
    s.add_argument("--runs", type=int, default=3)
    s.add_argument("--seed", type=int, default=0)
    s.add_argument("--out", default="evaluation_results")
    s.add_argument("--engine", choices=["native", "python"], default=None)
    s.add_argument("--schedulers", default=None)
    s.add_argument("--execute", action="store_true",
                   help="run each policy's placement of --model on this job's devices (measured makespan column)")
    s.add_argument("--model", default="gpt2")
    s.add_argument("--steps", type=int, default=10)
    s.add_argument("--warmup", type=int, default=3)
    s.add_argument("--seq", type=int, default=512)
    s.add_argument("--cost-model", choices=["bytes", "reference"], default="reference")
    s.add_argument("--regimes", default="1.0,0.9,0.8")
    s.add_argument("--nodes", choices=["equal", "reference", "laptops"], default="equal")
    s.set_defaults(fn=cmd_simulate)
    e = sub.add_parser("extract", help="reference GPT-2 DAG to JSON")
    e.add_argument("--model", default="gpt2")
    e.add_argument("--out", default="gpt2_dag.json")
    e.add_argument("--batch", type=int, default=1)
    e.add_argument("--seq", type=int, default=512)
    e.add_argument("--cost-model", choices=["bytes", "reference"], default="reference")
    e.set_defaults(fn=cmd_extract)
    el = sub.add_parser("elastic", help="run with device-loss injection and re-planning (one process per device)")
    _common(el)
    el.add_argument("--device", default="cpu", choices=["cpu", "cuda"])
    el.add_argument("--steps", type=int, default=2)
    el.add_argument("--fail-rank", type=int, default=None)
    el.add_argument("--fail-step", type=int, default=1)
    el.set_defaults(fn=cmd_elastic)
    m = sub.add_parser("models", help="list model presets")
    m.set_defaults(fn=cmd_models)
    g = sub.add_parser("generate", help="generate tokens on one device with on-device sampling")
    g.add_argument("--model", default="gpt2")
    g.add_argument("--kv-cache", type=int, default=None, metavar="C", help="positions per sequence (required)")
    g.add_argument("--kv-dtype", default="bf16", choices=["bf16", "fp8"])
    g.add_argument("--prompt-len", type=int, default=8, metavar="L", help="synthetic prompt tokens per sequence")
    g.add_argument("--new", type=int, default=16, metavar="N", help="tokens to generate per sequence")
    g.add_argument("--batch", type=int, default=1)
    g.add_argument("--temperature", type=float, default=0.0, help="0 = greedy")
    g.add_argument("--top-k", type=int, default=0, help="0 = off")
    g.add_argument("--top-p", type=float, default=1.0, help=">= 1 = off")
    g.add_argument("--seed", type=int, default=0)
    g.add_argument("--scheduler", default="EFT")
    g.add_argument("--hbm-cap-gb", type=float, default=288.0)
    g.add_argument("--device", default="auto", choices=["auto", "cpu"])
    g.add_argument("--no-graph", action="store_true")
    g.add_argument("--prefill-chunk", type=int, default=None, metavar="Tc",
                   help="consume the prompts in chunk steps of Tc tokens per sequence (2 .. min(C, 1024))")
    g.add_argument("--moe-decode", action="store_true", help="an MoE model's decode steps (see run --moe-decode)")
    g.add_argument("--skinny-gemm", action="store_true",
                   help="the dense GEMMs of the token step on the skinny kernel (see run --skinny-gemm)")
    g.set_defaults(fn=cmd_generate)
    a = ap.parse_args(argv)
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
