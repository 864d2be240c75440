"""Glue: model DAG -> scheduler placement -> per-rank programs -> executors.

``plan(...)`` is deterministic and runs identically on every rank (no communication is
needed to agree on the placement): the DAG builder, the native scheduler and the program
lowering are pure functions of their arguments.
"""
from __future__ import annotations

import json
import math
import os
from collections import defaultdict
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

from ..core import Node, get_scheduler
from ..core.task import Task
from ..models import registry
from ..models.params import ParamStore, group_layout
from .program import (Program, build_programs, build_steady_programs, plan_peer_fills, plan_prefill,
                      steady_fill_bytes)


@dataclass
class Plan:
    model: str
    tasks: List[Task]
    groups: Dict
    cfg: object
    scheduler_name: str
    scheduler: object
    schedule: Dict[str, List[str]]
    placement: Dict[str, int]
    order: List[str]
    node_rank: Dict[str, int]
    programs: List[Program]
    param_bytes: Dict[str, int]
    world: int
    cap_gb: float
    stats: Dict = field(default_factory=dict)
    args: Dict = field(default_factory=dict)  # plan() arguments (checkpoint / replan)
    # merged micro-batches (merge_mb > 1): request prefix "r{k}/" -> (merged prefix, batch
    # rows lo, hi) and merged token input -> the requests' token inputs, in row order
    requests: Dict = field(default_factory=dict)
    input_parts: Dict = field(default_factory=dict)
    # plan(kv_cache=C): bytes of the KV caches of the attention tasks each rank runs (they persist
    # across steps, next to the parameter and activation arenas); [] without a cache
    kv_cache_bytes: List[int] = field(default_factory=list)
    # plan(generate=True): bytes of the sampler's state per rank; [] without it
    sampler_bytes: List[int] = field(default_factory=list)
    # plan(prefill_chunk=Tc): bytes the chunk step adds per rank (its activation arena, workspace
    # beyond the token step's, gathered rows, row statistics, the fp8 dequantisation workspace)
    prefill_bytes: List[int] = field(default_factory=list)

    def owner(self, tid: str) -> Optional[int]:
        """Rank holding task ``tid``'s output (a merged request resolves to its group)."""
        if tid in self.placement:
            return self.placement[tid]
        if "/" in tid and self.requests:
            rid, base = tid.split("/", 1)
            m = self.requests.get(rid + "/")
            return self.placement.get(m[0] + base) if m else None
        return None

    @property
    def completed(self) -> int:
        return len(self.scheduler.completed_tasks)

    @property
    def total(self) -> int:
        return len(self.tasks)


def plan(model: str = "gpt2", world: int = 1, scheduler: str = "EFT", cap_gb: float = 288.0, replicas: int = 1,
         batch: int = 1, seq: int = 512, cost_model: str = "bytes", fuse: bool = True,
         node_speeds: Optional[Sequence[float]] = None, link_bw_gbps: float = 153.0,
         placement: str = "scheduler", tp: int = 1, resume: Optional[str] = None, sp: int = 1,
         residency: Optional[str] = None, merge_mb: int = 1, weight_dtype: str = "bf16",
         act_dtype: str = "bf16", kv_cache: Optional[int] = None, kv_dtype: str = "bf16",
         generate: bool = False, prefill_chunk: Optional[int] = None, moe_decode: bool = False,
         skinny_gemm: bool = False) -> Plan:
    """Build the DAG of ``replicas`` requests of ``model``, place it on ``world`` GPUs with
    ``scheduler`` under a per-GPU cap of ``cap_gb`` (one value, or one per GPU — the
    reference's heterogeneous node splits) and lower it to per-rank programs.

    ``placement``:
      * ``"scheduler"`` — the policy decides (default),
      * ``"replica"``   — request r on GPU r % world (plain data parallelism, a baseline),
      * ``"pipeline"``  — contiguous layer blocks per GPU, requests act as micro-batches
        (pipeline parallelism: each block boundary is a cross-GPU p2p edge),
      * ``"tensor"``    — with ``tp > 1``: shard k of every layer on GPU k % world, the
        shard-sum / residual / embedding / head nodes on GPU 0 (tensor parallelism).
      * ``"sequence"``  — with ``sp > 1``: sequence chunk c of every node on GPU c % world
        (context parallelism; the K/V edges between chunks are the cross-GPU transfers).
      * ``"expert"``    — MoE models: expert e of every layer on GPU e % world, everything
        else of request r on its home GPU r % world (expert parallelism: the router ->
        expert edges carry each expert's routed token rows, the expert -> combine edges its
        compact outputs).
    The fixed placements still go through the scheduler's memory accounting (tasks that
    do not fit fail exactly as in the policies).

    ``residency`` (default ``$DLS_RESIDENCY`` or ``"auto"``): how parameter residency of the
    repeating step is lowered — ``"trace"`` replays the policy's LOAD/EVICT trace (cold or
    warm-started, program.build_steady_programs); ``"auto"`` additionally offers a policy
    whose memory model is the repeating step (EFT) the planned keep set
    (program.plan_keep_sets) and keeps whichever re-fills fewer bytes per step.

    ``merge_mb`` = k > 1: the ``replicas`` requests are micro-batches of one batch, merged k at
    a time into one request of batch k x ``batch`` BEFORE placement (a DAG transform: every
    node of k co-located micro-batches becomes ONE node over k x the rows — one M = k x 512
    GEMM instead of k M = 512 launches, one p2p edge of k x the bytes instead of k). Every
    request keeps its own token ids and its own rows of the merged outputs
    (``Plan.requests``, ``DAGExecutor.output("r{k}/...")``).

    ``weight_dtype="fp8"``: the GEMM weights of a dense model are stored (and budgeted, filled
    and multiplied) as e4m3 bytes with one fp32 scale per output channel (registry.mark_fp8):
    about half the parameter bytes under the same cap. Raises ``ValueError`` with an MoE model,
    ``tp > 1`` or ``sp > 1``. ``weight_dtype="fp8-experts"``: the same storage for the expert
    weights of an MoE model only (router, attention and LM head stay bf16); raises ``ValueError``
    with a model without experts, ``tp > 1`` or ``sp > 1``. ``weight_dtype="mxfp4"``: the tensors
    ``"fp8"`` marks, stored as OCP MXFP4 (e2m1 pairs and one e8m0 scale per 32 elements of K:
    0.53 bytes per element); raises ``ValueError`` with an MoE model, ``tp > 1``, ``sp > 1``, a
    marked K that is no multiple of 32, or ``act_dtype != "fp8"`` (the one kernel is W4A8).
    ``weight_dtype="mxfp4-experts"``: MXFP4 storage for the tensors ``"fp8-experts"`` marks (router,
    attention and LM head stay bf16); raises ``ValueError`` with a model without experts,
    ``tp > 1``, ``sp > 1``, a marked K that is no multiple of 32, or ``act_dtype != "fp8"`` (the
    grouped kernel is W4A8).

    ``act_dtype="fp8"`` (with ``weight_dtype="fp8"``, ``"mxfp4"`` or ``"mxfp4-experts"`` only;
    anything else raises ``ValueError``): the input rows of every GEMM on a quantised weight are
    quantised to e4m3 with one power-of-two scale per row and multiplied on the block-scaled MFMA
    (``ops.linear_w8a8`` / ``ops.linear_w4a8`` / ``ops.gemm_grouped_w4a8``); the DAG, the bytes and
    the placement are those of the ``weight_dtype``.

    ``kv_cache=C``: decode steps. ``seq`` becomes the number of new tokens per step, T (a prefill
    chunk at T = 16, decode at T = 1); every attention node keeps K/V caches of C positions per
    sequence on the GPU it runs on (``attrs["kv_cache"]``), appends the step's T rows and attends
    them against the cache (``ops.kv_append`` / ``ops.attention_decode``). The cache bytes,
    ``2 * batch * C * n_kv_head * head_dim * 2`` per attention node, are part of the node's
    ``memory_required``, and after placement parameter arena + activation arena + caches are
    checked against every GPU's cap. A policy budgets parameters against the whole cap and sees a
    cache only while its attention task runs, so where the check fails the DAG is placed once more
    with every GPU's caches and activation arena set aside (a capped plan then evicts and
    re-fills parameters around its caches); if that does not fit either — the caches alone pass
    the cap — ``ValueError`` names the GPU and the three figures. ``Plan.kv_cache_bytes`` reports
    the caches per rank. gpt2 and llama families, placements ``scheduler`` / ``replica`` / ``pipeline``, any
    ``world``. Raises ``ValueError`` with an MoE model, ``tp``, ``sp`` or ``merge_mb`` above 1,
    C above the model's positions, T above 16, ``(n_head / n_kv_head) * T`` above 64, and with
    ``DLS_ATTN_BLOCK=1`` (the one-launch attention block has no cache).

    ``kv_dtype="fp8"`` (with ``kv_cache`` only, independent of ``weight_dtype`` / ``act_dtype``;
    anything else but ``"bf16"`` raises ``ValueError``): the caches hold e4m3 bytes and one fp32
    power-of-two scale per (position, KV head), ``2 * batch * C * n_kv_head * (head_dim + 4)`` bytes
    per attention node — what ``memory_required``, the cap check, its second placement and
    ``Plan.kv_cache_bytes`` then count. The step appends quantised rows and attends on the bytes
    (attn_decode_fp8.hip).

    ``generate=True`` (with ``kv_cache`` and ``seq == 1`` only; anything else raises ``ValueError``
    that says why): the decode step ends in a sampling launch (``ops.sample_tokens``) that writes
    the next token of every sequence into the token stream the next step embeds, so the captured
    step generates text (``DAGExecutor.set_prompts`` / ``set_sampling`` / ``generate``). Every
    request's ``lm_head`` op carries ``attrs["sample"]``; after placement its ``lm_head`` and
    ``embedding`` tasks must sit on one GPU (``world=1``, ``replica``, a ``scheduler`` placement
    that co-locates them) — ``ValueError`` names the two GPUs otherwise (``pipeline`` over more than
    one GPU): a token fed back across ranks is not supported. The sampler's state
    (``registry.sampler_state_bytes``, ``Plan.sampler_bytes``) counts towards the cap check next to
    the caches. The key enters ``Plan.args`` only when set.

    ``prefill_chunk=Tc`` (with ``kv_cache`` and ``seq == 1``, an int in 2 .. min(C, 1024); with or
    without ``generate``, either ``kv_dtype``): the plan's executor also runs its program as a CHUNK
    step in which every sequence consumes up to Tc tokens of its stream (``DAGExecutor.prefill`` /
    ``step_chunk``; ``generate`` then prefills each prompt in chunk steps). The DAG, the placement,
    the programs, the costs and the token step are those of the plan without the option. A chunk
    step runs the kernel groups up to the last attention only; what it adds to a GPU is
    ``Plan.prefill_bytes`` (``prefill_gb_per_rank``), counted against the cap next to the caches.
    Refused with ``ValueError``: a plan in which a rank's program sends or receives, and one whose
    programs re-fill parameters in the steady state. The key enters ``Plan.args`` only when set.

    ``moe_decode=True`` (with ``kv_cache``, an MoE model and ``weight_dtype="bf16"``; with or
    without ``generate``, either ``kv_dtype``): decode steps of an MoE model. Without the option an
    MoE model with ``kv_cache`` is refused as before. The step is the model's own DAG over
    ``batch * seq`` token rows — router, fused routing, grouped expert GEMMs, combine — around the
    cached attention; with at most ``ops.MOE_SKINNY_MAX_ROWS`` token rows (1: measured, see its
    comment) the executor issues both grouped expert launches of every layer through
    ``ops.gemm_grouped_skinny`` (``DLS_MOE_SKINNY=0``, and any larger step: the grouped kernels of
    full steps).
    Every other cache restriction holds. Refused with ``ValueError``: no ``kv_cache``, a model
    without experts, a ``weight_dtype`` other than ``"bf16"``, and ``prefill_chunk``. A capped plan (its programs evict and
    re-fill parameters), a plan with ``DLS_MOE_BATCH=0`` and a step of more than 16 token rows run
    the expert kernels of full steps. The key enters ``Plan.args`` only when set.

    ``skinny_gemm=True`` (with ``kv_cache`` and ``weight_dtype="bf16"``; any model family, either
    ``kv_dtype``, with or without ``generate``, ``prefill_chunk`` and ``moe_decode``): the executor
    sends the dense bf16 GEMMs of a step of at most ``ops.SKINNY_MAX_ROWS`` token rows (QKV,
    out-projection, gate/up, down, and with ``ops.SKINNY_LMHEAD`` the LM head) to the
    weight-streaming kernel of ``ops.linear_skinny`` instead of the prefill tiles; norms folded
    today stay folded (the kernel takes the row statistics itself), a chunk step keeps the tiles.
    The DAG, the placement, the programs and the costs are those of the plan without the option.
    Refused with ``ValueError``: no ``kv_cache``, a ``weight_dtype`` other than ``"bf16"``. The key
    enters ``Plan.args`` only when set.

    ``resume``: path of a placement saved by :func:`save_plan` — the saved decision (task
    order per GPU and the LOAD/EVICT trace) is reused instead of re-running the policy; the
    DAG is rebuilt from the saved arguments, which must match this call's.
    """
    caps_gb = [float(c) for c in cap_gb] if isinstance(cap_gb, (list, tuple)) else [float(cap_gb)] * world
    if len(caps_gb) != world:
        raise ValueError(f"{len(caps_gb)} per-GPU caps for world {world}")
    if isinstance(cap_gb, (list, tuple)):
        cap_gb = list(caps_gb)
    args = dict(model=model, world=world, scheduler=scheduler, cap_gb=cap_gb, replicas=replicas, batch=batch,
                seq=seq, cost_model=cost_model, fuse=fuse, node_speeds=list(node_speeds) if node_speeds else None,
                link_bw_gbps=link_bw_gbps, placement=placement, tp=tp)
    if sp > 1:
        args["sp"] = sp
    if weight_dtype != "bf16":  # (only when not the default: plans saved before it still resume)
        args["weight_dtype"] = weight_dtype
    if act_dtype != "bf16":  # (validated by registry.build below)
        args["act_dtype"] = act_dtype
    if kv_cache is not None:  # (validated by registry.build below)
        args["kv_cache"] = kv_cache
        if merge_mb > 1:
            raise ValueError("kv_cache does not combine with merged micro-batches (merge_mb > 1): every request "
                             "keeps caches and a position of its own")
        if os.environ.get("DLS_ATTN_BLOCK", "0") == "1":
            raise ValueError("kv_cache does not combine with DLS_ATTN_BLOCK=1: the one-launch attention block "
                             "has no KV cache")
        if placement not in ("scheduler", "replica", "pipeline"):
            raise ValueError(f"kv_cache: placement must be 'scheduler', 'replica' or 'pipeline', got {placement!r}")
    registry.check_kv_dtype(kv_dtype, kv_cache)
    if kv_dtype != "bf16":  # (only when not the default, as kv_cache)
        args["kv_dtype"] = kv_dtype
    registry.check_generate(generate, seq, kv_cache)
    if generate:  # (only when set: plans saved without it still resume, and stay as they were)
        args["generate"] = True
    registry.check_prefill_chunk(prefill_chunk, seq, kv_cache)
    if prefill_chunk is not None:  # (only when set, as generate)
        args["prefill_chunk"] = prefill_chunk
    registry.check_moe_decode(moe_decode, registry.get_config(model), kv_cache, weight_dtype, prefill_chunk)
    if moe_decode:  # (only when set, as generate)
        args["moe_decode"] = True
    registry.check_skinny_gemm(skinny_gemm, kv_cache, weight_dtype)
    if skinny_gemm:  # (only when set, as generate: the executor's choice of kernel, nothing the DAG sees)
        args["skinny_gemm"] = True
    requests, input_parts = {}, {}
    n_req, mb_batch = replicas, batch
    if merge_mb > 1:
        if replicas % merge_mb:
            raise ValueError(f"merge_mb={merge_mb} must divide replicas={replicas}")
        args["merge_mb"] = merge_mb
        n_req, mb_batch = replicas // merge_mb, batch * merge_mb
        for g in range(n_req):
            pre = f"r{g}/" if n_req > 1 else ""
            members = list(range(g * merge_mb, (g + 1) * merge_mb))
            input_parts[f"{pre}@tokens"] = [f"r{k}/@tokens" if replicas > 1 else "@tokens" for k in members]
            for j, k in enumerate(members):
                requests[f"r{k}/"] = (pre, j * batch, (j + 1) * batch)
    tasks, groups, cfg = registry.build(model, batch=mb_batch, seq=seq, replicas=n_req, cost_model=cost_model, tp=tp,
                                        sp=sp, weight_dtype=weight_dtype, act_dtype=act_dtype, kv_cache=kv_cache,
                                        kv_dtype=kv_dtype, generate=generate, moe_decode=moe_decode)
    param_bytes = {pid: group_layout(g)[0] for pid, g in groups.items()}

    def place_under(caps_now: Sequence[float]) -> Plan:
        """Run the policy (or the fixed placement, or the saved decision) under these per-GPU caps and lower it."""
        nodes = [Node(f"gpu{r}", caps_now[r], (node_speeds[r] if node_speeds else 1.0), device=r) for r in range(world)]
        node_rank = {n.id: r for r, n in enumerate(nodes)}
        cls = get_scheduler(scheduler)
        kw = {}
        if cost_model == "bytes":
            kw["param_cost"] = {pid: b / 1e9 for pid, b in param_bytes.items()}
        if cls.__name__ == "EFTScheduler":
            kw["link_bw_gbps"] = link_bw_gbps
            kw["refill_gb"] = {pid: b / 1e9 for pid, b in param_bytes.items()}  # what a refill really moves
            # the steady-state model needs real seconds, not abstract constants: the per-task kernel
            # times measured on an MI355X (ops/task_times.json, as the pipeline balancer uses) where
            # the table has the model, the roofline estimate elsewhere
            measured = measured_task_times(task_times_key(cfg.name, seq, mb_batch))
            if measured or cost_model != "bytes":
                kw["real_time"] = {t.id: measured.get(_base_id(t.id), real_time_s(t, param_bytes)) for t in tasks}
        sched = cls([n.fresh() for n in nodes], **kw)
        for t in tasks:
            sched.add_task(t.clone())
        if resume is not None:
            sched, schedule = _resume(resume, args, sched)
        elif placement == "scheduler":
            schedule = sched.schedule()
        elif placement in ("replica", "pipeline", "tensor", "sequence", "expert"):
            stage_of = None
            if placement == "pipeline" and world > 1 and os.environ.get("DLS_PIPELINE_STAGES", "balanced") != "layers":
                stage_of = pipeline_stages(tasks, world, param_bytes, caps_now, node_speeds, n_req,
                                           task_times_key(cfg.name, seq, mb_batch))
            order_in = tasks
            if placement == "expert" and world > 1 and n_req > 1:
                order_in = _interleave_requests(tasks)  # every GPU steps through the layers together
            schedule = _fixed_schedule(order_in, world, sched, placement, cfg, stage_of)
        else:
            raise ValueError(f"unknown placement {placement!r}")
        place = {tid: node_rank[sched.tasks[tid].assigned_node] for tid in sched.completed_tasks}
        order = [item for _, act, _, item in sched.events if act == "RUN"]
        caps = {r: int(caps_now[r] * 1e9) for r in range(world)}
        mode = residency or os.environ.get("DLS_RESIDENCY", "auto")
        if mode not in ("auto", "trace"):
            raise ValueError(f"unknown residency {mode!r}")
        planned = None
        if mode == "auto" and getattr(sched, "cyclic", False):
            # EFT's memory model is the repeating step: its residency may be the planned keep set
            # (program.plan_keep_sets) under the same budget the policy accounted: the node cap
            # minus the largest activation requirement among the node's tasks
            tmem = {t.id: t.memory_required for t in tasks}
            budget = {r: caps_now[r] - max([tmem[tid] for tid, rr in place.items() if rr == r] or [0.0])
                      for r in range(world)}
            planned = (budget, {pid: sched.param_size(pid) for pid in param_bytes})
        prefetch = os.environ.get("DLS_PREFETCH", "auto")  # executor.PREFETCH
        programs = build_steady_programs(tasks, place, order, world, param_bytes, caps, events=sched.events,
                                         node_rank=node_rank, fuse=fuse, planned=planned,
                                         lookahead=0 if prefetch == "0" else 1, force_ahead=prefetch == "1")
        if world > 1 and os.environ.get("DLS_PEER_FILL", "1") != "0":
            plan_peer_fills(programs, tasks, param_bytes)  # refills from a peer's HBM over xGMI
        name = cls.name if placement == "scheduler" else placement
        return Plan(model, tasks, groups, cfg, name, sched, schedule, place, order, node_rank, programs, param_bytes,
                    world, cap_gb, args=args, requests=requests, input_parts=input_parts)

    p = place_under(caps_gb)
    if kv_cache is not None:
        over = _kv_over_cap(p, caps_gb, prefill_chunk)
        if over and resume is None:
            # A policy budgets parameters against the whole cap and sees a cache only while its
            # attention task runs, but the caches persist: place once more with what this placement
            # needs for caches and activations set aside on every GPU
            reserve = [(kv + pr.act_arena_bytes) / 1e9 for kv, pr in zip(p.kv_cache_bytes, p.programs)]
            if all(caps_gb[r] > reserve[r] for r in range(world)):
                p = place_under([caps_gb[r] - reserve[r] for r in range(world)])
                over = _kv_over_cap(p, caps_gb, prefill_chunk)
        if over:
            raise ValueError(over)
    if generate:
        _check_feedback_placement(p)
    if prefill_chunk is not None:
        _check_chunk_programs(p)
    p.stats = plan_stats(p)
    return p


def _check_chunk_programs(p: Plan) -> None:
    """plan(prefill_chunk=Tc): a chunk step runs on one GPU from resident weights."""
    for r, pr in enumerate(p.programs):
        n = sum(1 for i in pr.instrs if i.op in ("send", "recv"))
        if n:
            raise ValueError(f"prefill_chunk: the program of GPU {r} has {n} sends / receives; chunk steps across "
                             f"ranks are not supported (world=1, or placement='replica')")
        fill = steady_fill_bytes(pr, p.param_bytes)
        peer = sum(1 for i in pr.instrs if i.op in ("psend",) or (i.op == "load" and i.peer >= 0))
        if fill > 0 or peer:
            raise ValueError(f"prefill_chunk: the program of GPU {r} re-fills parameters in the steady state "
                             f"({fill / 1e9:.6f} GB per step, {peer} peer transfers); chunk steps need resident "
                             f"weights (a larger cap_gb)")


def _kv_over_cap(p: Plan, caps_gb: Sequence[float], prefill_chunk: Optional[int] = None) -> Optional[str]:
    """Sets ``p.kv_cache_bytes`` (per rank: the caches of the attention tasks placed there) and
    says which GPU, if any, cannot hold its parameter arena, activation arena and caches together:
    caches persist across tasks, unlike activations."""
    per_rank, sampler = [0] * p.world, [0] * p.world
    for t in p.tasks:
        if t.op is not None and t.op.kind == "attention" and t.id in p.placement:
            per_rank[p.placement[t.id]] += registry.kv_cache_bytes(t.op)
        if t.op is not None and t.op.kind == "lm_head" and "sample" in t.op.attrs and t.id in p.placement:
            sampler[p.placement[t.id]] += registry.sampler_state_bytes(t.op)
    p.kv_cache_bytes = per_rank
    p.sampler_bytes = sampler if any(sampler) else []
    prefill = [0] * p.world
    if prefill_chunk is not None:
        tmap = {t.id: t for t in p.tasks}
        prefill = [plan_prefill(tmap, pr, prefill_chunk).total for pr in p.programs]
        p.prefill_bytes = prefill
    for r, pr in enumerate(p.programs):
        cap = int(caps_gb[r] * 1e9)
        if pr.param_arena_bytes + pr.act_arena_bytes + per_rank[r] + sampler[r] + prefill[r] > cap:
            return (f"GPU {r}: parameter arena {pr.param_arena_bytes / 1e9:.6f} GB + activation arena "
                    f"{pr.act_arena_bytes / 1e9:.6f} GB + KV caches {per_rank[r] / 1e9:.6f} GB"
                    + (f" + sampler state {sampler[r] / 1e9:.6f} GB" if sampler[r] else "")
                    + (f" + chunk-step buffers {prefill[r] / 1e9:.6f} GB" if prefill[r] else "")
                    + f" exceed its cap of {cap / 1e9:.6f} GB")
    return None


def _check_feedback_placement(p: Plan) -> None:
    """plan(generate=True): the sampler writes the token stream its request's embedding reads, on
    one GPU; a token fed back across ranks is not supported."""
    emb = {t.id.rsplit("/", 1)[0] if "/" in t.id else "": t.id for t in p.tasks
           if t.op is not None and t.op.kind == "embedding"}
    for t in p.tasks:
        if t.op is None or t.op.kind != "lm_head" or "sample" not in t.op.attrs:
            continue
        e = emb.get(t.id.rsplit("/", 1)[0] if "/" in t.id else "")
        a, b = p.placement.get(t.id), p.placement.get(e)
        if a is None or b is None or a != b:
            raise ValueError(f"generate=True: {t.id} runs on GPU {a} and {e} on GPU {b}; the sampled token is fed "
                             f"back on one GPU only (world=1, placement='replica', or a placement that keeps a "
                             f"request's embedding and LM head together)")


def real_time_s(t: Task, param_bytes: Dict[str, int]) -> float:
    """Roofline seconds of one task on one MI355X (the ``bytes`` cost model's estimate:
    models/gpt2._roofline), whatever cost model the task's ``compute_time`` is in."""
    from ..models.gpt2 import _roofline

    moved = float(getattr(t, "out_bytes", 0) or 0) + sum(float(param_bytes.get(p, 0)) for p in t.params_needed)
    return _roofline(float(getattr(t, "flops", 0.0) or 0.0), moved)


_PLAN_FORMAT = "dlsched-plan/1"


def save_plan(p: Plan, path: str) -> None:
    """Checkpoint a placement: the plan() arguments, the per-GPU task order and the
    scheduler's action trace (RUN / LOAD / EVICT / FAIL). Resume with ``plan(resume=path)``."""
    s = p.scheduler
    doc = {"format": _PLAN_FORMAT, "args": p.args, "scheduler": p.scheduler_name, "schedule": p.schedule,
           "events": [list(e) for e in s.events], "failed": sorted(s.failed_tasks),
           "stats": {k: v for k, v in p.stats.items() if isinstance(v, (int, float, list))}}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


class _ResumedSchedule:
    """Scheduler-shaped view of a saved decision (what build_programs / Plan consume)."""

    def __init__(self, sched, doc):
        self.tasks = sched.tasks
        self.nodes = sched.nodes
        self.events = [tuple(e) for e in doc["events"]]
        self.failed_tasks = set(doc.get("failed", []))
        self.completed_tasks = set()
        self.orphaned_tasks = set()
        for _, act, node, item in self.events:
            if act == "RUN":
                if item not in self.tasks:
                    raise ValueError(f"saved placement runs unknown task {item!r}")
                self.tasks[item].assigned_node = node
                self.completed_tasks.add(item)
        self.orphaned_tasks = set(self.tasks) - self.completed_tasks - self.failed_tasks


def _resume(path: str, args: Dict, sched):
    with open(path) as f:
        doc = json.load(f)
    if doc.get("format") != _PLAN_FORMAT:
        raise ValueError(f"{path}: not a saved plan")
    saved = dict(doc["args"])
    mismatch = {k: (saved.get(k), v) for k, v in args.items() if k not in ("fuse",) and saved.get(k) != v}
    if saved.get("weight_dtype", "bf16") != args.get("weight_dtype", "bf16"):  # (absent: the default)
        mismatch["weight_dtype"] = (saved.get("weight_dtype", "bf16"), args.get("weight_dtype", "bf16"))
    if saved.get("act_dtype", "bf16") != args.get("act_dtype", "bf16"):
        mismatch["act_dtype"] = (saved.get("act_dtype", "bf16"), args.get("act_dtype", "bf16"))
    if saved.get("kv_cache") != args.get("kv_cache"):
        mismatch["kv_cache"] = (saved.get("kv_cache"), args.get("kv_cache"))
    if saved.get("kv_dtype", "bf16") != args.get("kv_dtype", "bf16"):
        mismatch["kv_dtype"] = (saved.get("kv_dtype", "bf16"), args.get("kv_dtype", "bf16"))
    if saved.get("generate", False) != args.get("generate", False):
        mismatch["generate"] = (saved.get("generate", False), args.get("generate", False))
    if saved.get("prefill_chunk") != args.get("prefill_chunk"):
        mismatch["prefill_chunk"] = (saved.get("prefill_chunk"), args.get("prefill_chunk"))
    if saved.get("moe_decode", False) != args.get("moe_decode", False):
        mismatch["moe_decode"] = (saved.get("moe_decode", False), args.get("moe_decode", False))
    if saved.get("skinny_gemm", False) != args.get("skinny_gemm", False):
        mismatch["skinny_gemm"] = (saved.get("skinny_gemm", False), args.get("skinny_gemm", False))
    if mismatch:
        raise ValueError(f"saved plan was made with different arguments: {mismatch}")
    return _ResumedSchedule(sched, doc), {k: list(v) for k, v in doc["schedule"].items()}


def replan(p: Plan, lost_ranks: Sequence[int], **overrides) -> Plan:
    """Device loss: re-place the whole DAG on the surviving GPUs (ranks renumbered densely,
    speeds kept). The SURVEY §5 "device-loss injection -> re-plan onto survivors" path; the
    executor side is :func:`make_executor` on the new plan's programs."""
    lost = set(lost_ranks)
    keep = [r for r in range(p.world) if r not in lost]
    if not keep:
        raise RuntimeError("no surviving devices")
    a = dict(p.args)
    a.update(world=len(keep))
    if a.get("node_speeds"):
        a["node_speeds"] = [a["node_speeds"][r] for r in keep]
    if isinstance(a.get("cap_gb"), list):
        a["cap_gb"] = [a["cap_gb"][r] for r in keep]
    a.update(overrides)
    return plan(**a)


def _layer_of(tid: str, n_layer: int) -> int:
    """Pipeline position of a task: embedding -> -1, layer_i_* -> i, head -> n_layer."""
    base = tid.split("/")[-1]
    if base.startswith("layer_"):
        return int(base.split("_")[1])
    return -1 if base in ("embedding",) else n_layer


def _base_id(tid: str) -> str:
    return tid.split("/", 1)[1] if "/" in tid and tid[0] == "r" and tid.split("/", 1)[0][1:].isdigit() else tid


def pipeline_stages(tasks: Sequence[Task], world: int, param_bytes: Dict[str, int], caps_gb: Sequence[float],
                    node_speeds: Optional[Sequence[float]], replicas: int, model: str) -> Optional[Dict[str, int]]:
    """Pipeline stages balanced by kernel time (the VERDICT r4 item: layer-count blocks left
    half the stages idle half the time): a min-max partition of ONE request's DAG over the GPUs
    (the native steady-state partition, csrc/core/partition.h), every micro-batch's task on
    its base task's GPU. A stage's cost per step = its tasks' kernel time x the micro-batches +
    the p2p edges it sends and receives; cut points are the DAG's clean boundaries (the residual
    stream alone: attention / MLP half-layers), so no fused kernel pair is split. Kernel times:
    the measured per-task table (``ops/task_times.json``, written by
    ``benchmarks/measure_task_times.py`` on an MI355X) when it has the model, else the roofline
    (:func:`real_time_s`). Returns base task id -> GPU, or None (no native core / infeasible:
    the caller keeps layer-count blocks)."""
    from ..core import native as _native

    try:
        core = _native.load()
    except Exception:  # noqa: BLE001 — the layer-count split still works
        return None
    base = [t for t in tasks if _base_id(t.id) == t.id or t.id.startswith("r0/")]
    ids = [_base_id(t.id) for t in base]
    index = {tid: i for i, tid in enumerate(ids)}
    measured = measured_task_times(model)
    R = max(int(replicas), 1)
    pn, pidx, prow = [], {}, []
    for t in base:
        row = []
        for p in sorted(t.params_needed):
            if p not in pidx:
                pidx[p] = len(pn)
                pn.append(p)
            row.append(pidx[p])
        prow.append(row)
    inst = core.Instance()
    inst.task_ids = ids
    inst.mem = [float(t.out_bytes) * R / 1e9 for t in base]
    times = [measured.get(i, real_time_s(t, param_bytes)) if measured else real_time_s(t, param_bytes)
             for i, t in zip(ids, base)]
    inst.compute = [v * R for v in times]
    inst.real_time = list(inst.compute)
    inst.deps = [[index.get(_base_id(d), -1) for d in t.dependencies] for t in base]
    inst.params = prow
    inst.param_names = pn
    inst.param_cost = [param_bytes.get(p, 0) / 1e9 for p in pn]
    inst.param_refill = list(inst.param_cost)
    inst.node_ids = [f"gpu{r}" for r in range(world)]
    inst.node_mem = [float(c) for c in caps_gb]
    inst.node_speed = [float(v) for v in node_speeds] if node_speeds else [1.0] * world
    inst.out_size = [float(t.out_bytes) * R / 1e9 for t in base]
    # fused kernel chains of the lowering (program._fusion): a stage cut never splits one
    from .program import _consumers, _fusion
    tmap = {t.id: t for t in base}
    one = {t.id: 0 for t in base}
    order = [t.id for t in base]
    fused_into, _ = _fusion(tmap, one, order, _consumers(tmap, one, order), {t: i for i, t in enumerate(order)}, True)
    inst.fuse_into = [index[_base_id(fused_into[t.id])] if t.id in fused_into else -1 for t in base]
    part = core.steady_partition(inst, world, world)
    if not part.feasible:
        return None
    return {ids[i]: int(n) for i, n in enumerate(part.node_of_task) if n >= 0}


_TASK_TIMES: Dict[str, Dict[str, float]] = {}


def task_times_key(model: str, seq: int, batch: int) -> str:
    return f"{model}/s{seq}b{batch}"


def measured_task_times(key: str) -> Dict[str, float]:
    """Per-task kernel seconds measured on an MI355X (base task ids; a fused kernel group's
    time split over its tasks) for ``key`` = :func:`task_times_key`, from
    ``ops/task_times.json``; a batch the table lacks is scaled from batch 1 (an upper bound:
    bigger GEMMs run closer to peak); {} if absent."""
    if not _TASK_TIMES:
        path = os.environ.get("DLS_TASK_TIMES") or os.path.join(os.path.dirname(__file__), "..", "ops",
                                                                  "task_times.json")
        try:
            with open(path) as f:
                _TASK_TIMES.update(json.load(f))
        except (OSError, ValueError):
            _TASK_TIMES["__none__"] = {}
    if key in _TASK_TIMES:
        return dict(_TASK_TIMES[key])
    head, _, b = key.rpartition("b")
    if b.isdigit() and int(b) > 1 and (head + "b1") in _TASK_TIMES:
        return {t: v * int(b) for t, v in _TASK_TIMES[head + "b1"].items()}
    return {}


def _interleave_requests(tasks: Sequence[Task]) -> List[Task]:
    """Layer-major order of replicated requests (identical DAGs, ids ``r{k}/...``): the i-th
    task of every request before the (i+1)-th of any. With data-parallel attention and expert
    parallelism each GPU is home to one request and hosts experts of all of them; request-major
    order would run the requests one after another across the whole job (each GPU's experts
    serve request 0's 32 layers before its own request starts), whereas here every GPU works on
    the same layer, and one layer's expert nodes of all requests sit next to each other in its
    program — the co-run span (program.plan_coruns) that streams each expert's weights once."""
    seen: Dict[str, int] = defaultdict(int)
    keyed = []
    for n, t in enumerate(tasks):
        rep = t.id.split("/", 1)[0] if "/" in t.id else ""
        keyed.append((seen[rep], n, t))
        seen[rep] += 1
    return [t for _, _, t in sorted(keyed, key=lambda x: (x[0], x[1]))]


def _fixed_schedule(tasks: Sequence[Task], world: int, sched, mode: str, cfg,
                    stage_of: Optional[Dict[str, int]] = None) -> Dict[str, List[str]]:
    """Place without the policy: by replica (DP) or by contiguous pipeline stages (PP:
    ``stage_of`` base task -> GPU from :func:`pipeline_stages`, else layer-count blocks).
    Tasks are committed in DAG order; memory is still accounted per node."""
    out: Dict[str, List[str]] = {}
    nodes = list(sched.nodes.values())
    L = cfg.n_layer
    for t in tasks:
        if mode in ("replica", "expert"):
            rep = int(t.id.split("/")[0][1:]) if "/" in t.id else 0
            r = rep % world
            if mode == "expert" and t.op is not None and t.op.kind == "moe_expert":
                r = t.op.attrs["expert"] % world
        elif mode in ("tensor", "sequence"):
            tag = "tp" if mode == "tensor" else "sp"
            sfx = t.id.rsplit(".", 1)[-1] if "." in t.id.split("/")[-1] else ""
            r = int(sfx[2:]) % world if sfx.startswith(tag) and sfx[2:].isdigit() else 0
        elif stage_of is not None and _base_id(t.id) in stage_of:
            r = stage_of[_base_id(t.id)]
        else:
            layer = min(max(_layer_of(t.id, L), 0), L - 1)
            r = min(layer * world // L, world - 1)
        node = nodes[r]
        if any(d in sched.failed_tasks or d not in sched.completed_tasks for d in t.dependencies) \
                or not sched.assign_task_to_node(sched.tasks[t.id], node):
            sched.fail_task(t.id)
            continue
        out.setdefault(node.id, []).append(t.id)
    return out


def plan_stats(p: Plan) -> Dict:
    cross = 0
    cross_bytes = 0
    tmap = {t.id: t for t in p.tasks}
    for tid, r in p.placement.items():
        for d in tmap[tid].dependencies:
            if d in p.placement and p.placement[d] != r:
                cross += 1
                cross_bytes += tmap[d].xfer_bytes
    return {
        "tasks_total": len(p.tasks),
        "tasks_completed": len(p.scheduler.completed_tasks),
        "tasks_failed": len(p.scheduler.failed_tasks),
        "tasks_orphaned": len(p.scheduler.orphaned_tasks),
        "cross_gpu_edges": cross,
        "cross_gpu_bytes": cross_bytes,
        "kernels_per_rank": [pr.n_kernels for pr in p.programs],
        "param_peak_gb_per_rank": [pr.param_peak_bytes / 1e9 for pr in p.programs],
        "act_arena_gb_per_rank": [pr.act_arena_bytes / 1e9 for pr in p.programs],
        **({"kv_cache_gb_per_rank": [b / 1e9 for b in p.kv_cache_bytes]} if p.kv_cache_bytes else {}),
        **({"sampler_gb_per_rank": [b / 1e9 for b in p.sampler_bytes]} if p.sampler_bytes else {}),
        **({"prefill_gb_per_rank": [b / 1e9 for b in p.prefill_bytes]} if p.prefill_bytes else {}),
        # parameter bytes re-filled per steady-state step (evict/reload traffic of the plan)
        "refill_gb_per_step_per_rank": [steady_fill_bytes(pr, p.param_bytes) / 1e9 for pr in p.programs],
        # of which received from a peer GPU's arena over xGMI (RCCL p2p) instead of the host
        "peer_fill_gb_per_step_per_rank": [sum(int(p.param_bytes.get(i.param, 0)) for i in pr.instrs
                                               if i.op == "load" and i.peer >= 0) / 1e9 for pr in p.programs],
        "tasks_per_rank": [sum(1 for r in p.placement.values() if r == k) for k in range(p.world)],
        # distinct (producer, consumer GPU) transfers: what the p2p edges really move
        "cross_gpu_transfers": len({(d, r) for tid, r in p.placement.items() for d in tmap[tid].dependencies
                                    if d in p.placement and p.placement[d] != r}),
        # what the same transfers move when expert-parallel edges carry routed rows only (the
        # device transport, DAGExecutor._plan_routed_edges): expected M*k/E rows per expert
        "cross_gpu_bytes_routed": _routed_cross_bytes(p, tmap),
        # what the programs' p2p sends move per step on the RCCL transport: whole buffers, except
        # expert-parallel capacity edges (program.plan_ep_capacity: EP_CAPACITY x the expected
        # routed rows, fixed-size messages)
        "cross_gpu_bytes_rccl": _rccl_send_bytes(p, tmap),
        **_steady_stats(p.scheduler),
    }


def _rccl_send_bytes(p: Plan, tmap) -> int:
    total = 0
    for pr in p.programs:
        for i in pr.instrs:
            if i.op != "send":
                continue
            t = tmap[i.task]
            if i.rows and t.op is not None and t.op.out_shape:
                total += int(t.xfer_bytes * i.rows / math.prod(t.op.out_shape[:-1]))
            else:
                total += t.xfer_bytes
    return total


def _routed_cross_bytes(p: Plan, tmap) -> int:
    """Cross-GPU bytes per step with routed-row expert edges: a hidden state sent to a GPU whose
    consumers there are experts moves the rows routed to those experts (expected M*k/E per
    expert), an expert's output its routed rows; every other transfer its whole buffer."""
    total = 0
    users_at: Dict[Tuple[str, int], List[Task]] = {}
    for tid, r in p.placement.items():
        for d in tmap[tid].dependencies:
            if d in p.placement and p.placement[d] != r:
                users_at.setdefault((d, r), []).append(tmap[tid])
    for (d, r), users in users_at.items():
        t = tmap[d]
        exp_users = [u for u in users if u.op is not None and u.op.kind == "moe_expert" and u.op.inputs[0] == d]
        if users and len(exp_users) == len(users):
            a = exp_users[0].op.attrs
            total += int(t.xfer_bytes * a["top_k"] * len(exp_users) / a["n_experts"])
        elif t.op is not None and t.op.kind == "moe_expert":
            total += int(t.xfer_bytes * t.op.attrs["top_k"] / t.op.attrs["n_experts"])
        else:
            total += t.xfer_bytes
    return total


def _steady_stats(s) -> Dict:
    """EFT's steady-state model (csrc/core/partition.h): modelled step period of its cold pass
    and of the placement it returned, and whether the pipeline partition replaced the cold pass."""
    if not hasattr(s, "steady_period") or not getattr(s, "cold_period", 0.0):
        return {}
    return {"eft_partitioned": bool(s.partitioned), "modelled_period_ms": round(s.steady_period * 1e3, 4),
            "modelled_cold_period_ms": round(s.cold_period * 1e3, 4),
            "stages": [{"node": st["node"], "busy_ms": round(st["busy_s"] * 1e3, 4),
                        "refill_gb": round(st["refill_gb"], 6)} for st in s.stages]}


def torch_device_type(device) -> str:
    import torch

    return torch.device(device).type


def ep_widen_on_overflow(ex, pg=None) -> bool:
    """After a step of an expert-parallel job (one process per rank): did any rank's capacity
    edge overflow? (one all-reduce; a host read of this rank's flags). If so every rank widens
    the groups IT saw overflow (both ranks of a group see the same routing counts) and the
    caller re-runs the step — and re-captures, if it captured — then calls this again: a
    corrected layer can change a later layer's routing, so repeat until it returns False."""
    import torch
    import torch.distributed as dist

    mine = ex.ep_overflow()
    flag = torch.tensor([1 if mine else 0], dtype=torch.int32,
                        device=ex.device if (ex.gpu and pg is not None and dist.get_backend(pg) == "nccl") else "cpu")
    if pg is not None:
        dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=pg)
    if not int(flag.item()):
        return False
    ex.widen_ep(mine)
    return True


def make_store(p: Plan, seed: int = 0, device_init: bool = False) -> ParamStore:
    return ParamStore(p.groups, seed=seed, device_init=device_init)


def device_init_ok(p: Plan, rank: int) -> bool:
    """Can rank's weights be random-initialised straight into HBM? Only when its program
    re-fills nothing in the steady state: every refill of an evicted/overwritten group must
    be a real host->HBM copy (a measured cost, and capturable in a hipGraph)."""
    return steady_fill_bytes(p.programs[rank], p.param_bytes) == 0


P2P = os.environ.get("DLS_P2P", "rccl")  # cross-GPU DAG edges: "rccl" (c10d p2p) or "device" (devp2p.py)


def p2p_group(p: Plan, rank: int, device, pg, transport: Optional[str] = None):
    """The ``pg`` to hand :func:`make_executor` for a process-per-GPU job: the process group
    itself (RCCL p2p, the default), or — ``transport="device"`` / ``DLS_P2P=device`` — the
    device-initiated transport (parallel/devp2p.py: edges moved by kernels, each rank's whole
    step one hipGraph), whose arenas and mailboxes the ranks exchange as IPC handles over ``pg``
    once, when the executors are built."""
    transport = transport or P2P
    if pg is None or p.world == 1 or transport == "rccl":
        return pg
    if transport != "device":
        raise ValueError(f"unknown p2p transport {transport!r}")
    from .devp2p import DeviceP2PGroup, DeviceP2PWorld

    return DeviceP2PGroup(DeviceP2PWorld(p, device, [rank]), rank, pg=pg)


def make_executor(p: Plan, rank: int, device, store: Optional[ParamStore] = None, pg=None, use_graph: bool = True,
                  trace: bool = False, debug: bool = False, autotune: bool = True):
    """``debug=True``: validate every rank's program first (parallel/validate.py) and run the
    executor with arena canaries and output finiteness checks. ``autotune=False``: GEMM shapes
    missing from the tuning table run the kernel's heuristic config instead of being tuned first."""
    from .executor import DAGExecutor

    if debug:
        from .validate import check_plan

        dev = torch_device_type(device) == "cuda"
        transport = getattr(pg, "world", None) is not None and type(pg).__name__ in ("DeviceP2PGroup", "HostP2PGroup")
        errs = check_plan(p, device=transport, gpu=dev)
        if errs:
            raise RuntimeError("invalid plan:\n  " + "\n  ".join(errs[:20]))
    # per-model GEMM choices by the canonical preset name (aliases such as "mixtral" resolve to it)
    return DAGExecutor(p.tasks, p.programs[rank], store or make_store(p), device, model_cfg=p.cfg,
                       use_graph=use_graph, pg=pg, trace=trace, debug=debug, model_name=p.cfg.name, autotune=autotune,
                       input_parts=p.input_parts, requests=p.requests, act_dtype=p.args.get("act_dtype", "bf16"),
                       prefill_chunk=p.args.get("prefill_chunk"), skinny_gemm=p.args.get("skinny_gemm", False))
