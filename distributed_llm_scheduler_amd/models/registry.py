"""Model registry: preset name -> (task DAG, parameter groups, config)."""
from __future__ import annotations

from typing import Dict, List, Tuple

from ..core.task import Task
from .config import ModelConfig, get_config
from .params import MX_BLOCK, ParamGroup


def param_groups(cfg: ModelConfig) -> Dict[str, ParamGroup]:
    if cfg.family == "gpt2":
        from .gpt2 import gpt2_param_groups
        return gpt2_param_groups(cfg)
    if cfg.family in ("llama", "mixtral"):
        from .llama import llama_param_groups
        return llama_param_groups(cfg)
    raise KeyError(cfg.family)


def build_dag(cfg: ModelConfig, batch: int = 1, seq: int = 512, cost_model: str = "bytes",
              prefix: str = "") -> List[Task]:
    if cfg.family == "gpt2":
        from .gpt2 import build_gpt2_dag
        return build_gpt2_dag(cfg, batch=batch, seq=seq, cost_model=cost_model, prefix=prefix)
    if cfg.family in ("llama", "mixtral"):
        from .llama import build_llama_dag
        return build_llama_dag(cfg, batch=batch, seq=seq, cost_model=cost_model, prefix=prefix)
    raise KeyError(cfg.family)


WEIGHT_DTYPES = ("bf16", "fp8", "fp8-experts")
# block-scaled (OCP MX) weight storage, accepted next to WEIGHT_DTYPES: "mxfp4" marks the tensors
# "fp8" marks (dense models) and needs act_dtype="fp8"
MX_WEIGHT_DTYPES = ("mxfp4",)
# the same storage for the expert weights of an MoE model only (what "fp8-experts" marks), also
# with act_dtype="fp8": the grouped W4A8 kernel
MX_EXPERT_WEIGHT_DTYPES = ("mxfp4-experts",)
ACT_DTYPES = ("bf16", "fp8")
# (op kind, weight key) pairs that read a tensor as a GEMM weight operand
_GEMM_OPERANDS = {("linear", "w"), ("lm_head", "w"), ("attention", "w_qkv"), ("attention", "w_o"),
                  ("swiglu_mlp", "w_gate_up"), ("swiglu_mlp", "w_down")}
# the expert GEMM weights of an MoE layer (weight_dtype="fp8-experts"); the router weight
# (moe.gate, read by a "linear" node) is not among them
_EXPERT_OPERANDS = {("moe_expert", "w_gate_up"), ("moe_expert", "w_down")}


def mark_fp8(tasks: List[Task], groups: Dict[str, ParamGroup], operands=_GEMM_OPERANDS,
             fmt: str = "fp8") -> List[str]:
    """Mark for quantised storage in format ``fmt`` ("fp8", or "mxfp4": ``TensorSpec.qfmt``) (``TensorSpec.quant``) every tensor that EVERY reader reads as one
    of ``operands`` — (op kind, weight key) pairs: by default the GEMM weight operands of a
    dense model, ``_EXPERT_OPERANDS`` for the experts of an MoE model. Embedding tables, norm
    gains, biases and a weight an embedding also gathers from (GPT-2's tied ``wte``) stay bf16.
    Returns the marked names."""
    gemm, other = set(), set()
    for t in tasks:
        if t.op is None:
            continue
        for key, name in t.op.weights.items():
            if isinstance(name, str):
                (gemm if (t.op.kind, key) in operands else other).add(name)
    marked = []
    for g in groups.values():
        for sp in g.tensors:
            if sp.name in gemm and sp.name not in other and len(sp.shape) == 2 and sp.parent is None:
                if fmt == "mxfp4" and sp.shape[1] % MX_BLOCK:
                    raise ValueError(f"weight_dtype='mxfp4': {sp.name} has K = {sp.shape[1]}, not a multiple of "
                                     f"{MX_BLOCK} (one e8m0 scale per {MX_BLOCK} elements)")
                sp.quant = True
                sp.qfmt = fmt
                marked.append(sp.name)
    return marked


def check_act_dtype(act_dtype: str, weight_dtype: str) -> None:
    """``act_dtype="fp8"`` (e4m3 GEMM inputs, one power-of-two scale per row) exists only over
    quantised GEMM weights of a dense model: ``weight_dtype="fp8"`` (the W8A8 kernel) or
    ``"mxfp4"`` (the W4A8 kernel, which is the only MXFP4 GEMM: ``"mxfp4"`` needs ``"fp8"``) —
    and over the MXFP4 expert weights of an MoE model, ``weight_dtype="mxfp4-experts"`` (the grouped
    W4A8 kernel; it needs ``"fp8"`` for the same reason)."""
    if act_dtype not in ACT_DTYPES:
        raise ValueError(f"act_dtype must be one of {ACT_DTYPES}, got {act_dtype!r}")
    if weight_dtype in MX_EXPERT_WEIGHT_DTYPES:
        if act_dtype != "fp8":
            raise ValueError(f"weight_dtype={weight_dtype!r} needs act_dtype='fp8': the one grouped MXFP4 kernel is "
                             f"W4A8 (e4m3 activation rows on the block-scaled MFMA), got act_dtype={act_dtype!r}")
        return
    if act_dtype == "fp8" and weight_dtype not in ("fp8", "mxfp4"):
        raise ValueError(f"act_dtype='fp8' needs weight_dtype='fp8' or 'mxfp4' (the fp8 x fp8 and MXFP4 x fp8 "
                         f"GEMMs of dense models), got weight_dtype={weight_dtype!r}")
    if weight_dtype == "mxfp4" and act_dtype != "fp8":
        raise ValueError(f"weight_dtype='mxfp4' needs act_dtype='fp8': there is one MXFP4 kernel, W4A8 (e4m3 "
                         f"activation rows on the block-scaled MFMA), got act_dtype={act_dtype!r}")


KV_MAX_STEP = 16  # new tokens per step the decode attention kernel takes
KV_MAX_COLS = 64  # (n_head / n_kv_head) * new tokens: its query columns per KV head


def check_kv_cache(cfg: ModelConfig, seq: int, kv_cache: int, tp: int = 1, sp: int = 1, moe_decode: bool = False) -> None:
    """What a KV cache of ``kv_cache`` positions with ``seq`` new tokens per step does not combine
    with. An MoE model takes decode steps only with ``moe_decode=True`` (see :func:`check_moe_decode`)."""
    if not isinstance(kv_cache, int) or isinstance(kv_cache, bool) or kv_cache < 1:
        raise ValueError(f"kv_cache must be a positive number of positions, got {kv_cache!r}")
    if cfg.n_experts and not moe_decode:
        raise ValueError(f"kv_cache: MoE models ({cfg.name}) take decode steps only with moe_decode=True "
                         "(--moe-decode); without it the cache covers dense gpt2 / llama models only")
    if tp > 1 or sp > 1:
        raise ValueError("kv_cache does not combine with tensor or sequence parallelism (tp, sp > 1): a cache "
                         "belongs to one attention node on one GPU")
    if kv_cache > cfg.n_positions:
        raise ValueError(f"kv_cache={kv_cache} exceeds {cfg.name}'s {cfg.n_positions} positions")
    if seq < 1 or seq > KV_MAX_STEP:
        raise ValueError(f"kv_cache: seq is the number of new tokens per step, 1 .. {KV_MAX_STEP}, got {seq}")
    if seq > kv_cache:
        raise ValueError(f"kv_cache={kv_cache} holds less than one step of {seq} tokens")
    rep = cfg.n_head // cfg.kv_heads
    if rep * seq > KV_MAX_COLS:
        raise ValueError(f"kv_cache: (n_head / n_kv_head) * seq = {rep} * {seq} exceeds the decode attention "
                         f"kernel's {KV_MAX_COLS} query rows per KV head")


def check_moe_decode(moe_decode: bool, cfg: ModelConfig, kv_cache: "int | None", weight_dtype: str = "bf16",
                     prefill_chunk=None) -> None:
    """What ``moe_decode=True`` (decode steps of an MoE model over the KV cache, the expert GEMMs
    of a step of a few token rows on the skinny grouped kernel: ops.MOE_SKINNY_MAX_ROWS) needs of a plan."""
    if not moe_decode:
        return
    if kv_cache is None:
        raise ValueError("moe_decode=True needs a KV cache (kv_cache=C): it is the decode step of an MoE model")
    if not cfg.n_experts:
        raise ValueError(f"moe_decode=True needs an MoE model; {cfg.name} has no experts (its decode steps need "
                         "no option)")
    if weight_dtype != "bf16":
        raise ValueError(f"moe_decode=True takes weight_dtype='bf16' only, got {weight_dtype!r}: quantised experts "
                         "keep their own grouped kernels, which have no skinny form yet")
    if prefill_chunk is not None:
        raise ValueError("moe_decode=True does not combine with prefill_chunk: a chunk step's bit-identical repeat "
                         "has not been shown for the routing and combine launches of an MoE layer")


def check_skinny_gemm(skinny_gemm: bool, kv_cache: "int | None", weight_dtype: str = "bf16") -> None:
    """What ``skinny_gemm=True`` (the dense GEMMs of a decode step of at most ops.SKINNY_MAX_ROWS
    token rows on the weight-streaming skinny kernel, ops.linear_skinny) needs of a plan. Every
    model family, both ``kv_dtype``s, ``generate``, ``prefill_chunk`` (the token step takes the
    kernel, the chunk step keeps the tiles), MoE models with ``moe_decode`` (their dense GEMMs)
    and capped plans are accepted."""
    if not skinny_gemm:
        return
    if kv_cache is None:
        raise ValueError("skinny_gemm=True needs a KV cache (kv_cache=C): the skinny kernel is for the at most 16 "
                         "token rows of a decode step")
    if weight_dtype != "bf16":
        raise ValueError(f"skinny_gemm=True takes weight_dtype='bf16' only, got {weight_dtype!r}: the quantised GEMMs "
                         "have no skinny form yet")


KV_DTYPES = ("bf16", "fp8")


def check_kv_dtype(kv_dtype: str, kv_cache: "int | None") -> None:
    if kv_dtype not in KV_DTYPES:
        raise ValueError(f"kv_dtype must be one of {KV_DTYPES}, got {kv_dtype!r}")
    if kv_dtype != "bf16" and kv_cache is None:
        raise ValueError(f"kv_dtype={kv_dtype!r} needs a KV cache (kv_cache=C)")


def check_generate(generate: bool, seq: int, kv_cache: "int | None") -> None:
    """What on-device token sampling (``generate=True``) needs of a plan."""
    if not generate:
        return
    if kv_cache is None:
        raise ValueError("generate=True needs a KV cache (kv_cache=C): the sampler feeds the token stream of "
                         "decode steps")
    if seq != 1:
        raise ValueError(f"generate=True needs seq=1, got {seq}: a step of T > 1 tokens would consume positions "
                         "whose tokens are not generated yet")


PREFILL_MAX_CHUNK = 1024  # widest query chunk of ops.attention_chunk


def check_prefill_chunk(prefill_chunk, seq: int, kv_cache: "int | None") -> None:
    """What chunked prompt prefill (``prefill_chunk=Tc``: a second step shape of Tc tokens per
    sequence next to the token step) needs of a plan; works with or without ``generate`` and with
    either ``kv_dtype``."""
    if prefill_chunk is None:
        return
    if kv_cache is None:
        raise ValueError("prefill_chunk needs a KV cache (kv_cache=C): a chunk step fills the caches of decode steps")
    if seq != 1:
        raise ValueError(f"prefill_chunk needs seq=1, got {seq}: the plan's own step is the token step, the chunk "
                         "step is its second shape")
    hi = min(kv_cache, PREFILL_MAX_CHUNK) if isinstance(kv_cache, int) else PREFILL_MAX_CHUNK  # (kv_cache: checked by build)
    if not isinstance(prefill_chunk, int) or isinstance(prefill_chunk, bool) or not 2 <= prefill_chunk <= hi:
        raise ValueError(f"prefill_chunk must be an int in 2 .. min(kv_cache, {PREFILL_MAX_CHUNK}) = {hi}, "
                         f"got {prefill_chunk!r}")


def sample_slices(B: int, V: int):
    """(workgroups per row, elements per workgroup) of the sampling kernel (csrc/kernels/sample.hip
    ``sample_slices``), for its workspace's bytes."""
    S = max(1, min(64, -(-V // 8192), 512 // max(B, 1)))
    length = -(-(-(-V // 8)) // S) * 8
    return -(-V // length), length


def sampler_state_bytes(op) -> int:
    """Bytes a marked LM head (``attrs["sample"]``) keeps next to the caches: temperature, top_k,
    top_p, prompt_len, done and next per sequence, stats [B][4], seed, eos, and the kernel's
    workspace (264 words per workgroup of a row, one ticket per row), each padded to 256."""
    B, V = op.out_shape[0], op.out_shape[-1]
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    return 6 * al(4 * B) + al(16 * B) + al(8) + al(4) + al(4 * B * sample_slices(B, V)[0] * 264) + al(4 * B)


def kv_cache_bytes(op, dtype_bytes: int = 2) -> int:
    """Bytes of an attention node's K and V caches: 2 * B * C * n_kv_head * head_dim * dtype_bytes;
    with ``attrs["kv_dtype"] == "fp8"`` 2 * B * C * n_kv_head * (head_dim + 4): one e4m3 byte per
    element and one fp32 scale per (position, KV head)."""
    a = op.attrs
    if a.get("kv_dtype", "bf16") == "fp8":
        return 2 * op.out_shape[0] * a["kv_cache"] * a["n_kv_head"] * (a["head_dim"] + 4)
    return 2 * op.out_shape[0] * a["kv_cache"] * a["n_kv_head"] * a["head_dim"] * dtype_bytes


def add_kv_cache(tasks: List[Task], batch: int, seq: int, kv_cache: int, cost_model: str = "bytes",
                 kv_dtype: str = "bf16") -> None:
    """In place: every attention node carries ``attrs["kv_cache"] = C`` (and ``attrs["kv_dtype"]``
    when that is not bf16); its ``memory_required``
    grows by its cache bytes (which persist across steps, unlike its activations, so every policy
    sees what the node needs on its GPU); its flops count the score terms over the cache length
    (T queries x C keys in place of the causal T x T), and under the ``bytes`` cost model its time
    the cache bytes it streams."""
    from .gpt2 import _roofline

    for t in tasks:
        if t.op is None or t.op.kind != "attention":
            continue
        t.op.attrs["kv_cache"] = int(kv_cache)
        if kv_dtype != "bf16":
            t.op.attrs["kv_dtype"] = kv_dtype
        a = t.op.attrs
        cache = kv_cache_bytes(t.op)
        core_old = 2.0 * batch * a["n_head"] * seq * seq * a["head_dim"]
        core_new = 4.0 * batch * a["n_head"] * seq * kv_cache * a["head_dim"]
        if cost_model == "bytes":
            # the builder's time (the roofline of the old flops and the node's other bytes) stays
            # as a floor; the new time is the larger of it and the roofline of the new flops
            # against the cache bytes alone, which the node streams once per step
            t.compute_time = max(t.compute_time, _roofline(t.flops - core_old + core_new, cache))
        t.flops = t.flops - core_old + core_new
        t.memory_required += cache / 1e9


def build(model: str, batch: int = 1, seq: int = 512, replicas: int = 1, cost_model: str = "bytes",
          tp: int = 1, sp: int = 1, weight_dtype: str = "bf16", act_dtype: str = "bf16",
          kv_cache: "int | None" = None,
          kv_dtype: str = "bf16", generate: bool = False,
          moe_decode: bool = False) -> Tuple[List[Task], Dict[str, ParamGroup], ModelConfig]:
    """``replicas`` independent requests (task ids prefixed ``r{k}/``) sharing weights;
    ``tp > 1`` splits every layer into tensor-parallel shards, ``sp > 1`` every token-wise
    node into sequence chunks (models/transforms.py). ``weight_dtype="fp8"``: the GEMM weights
    of a dense model are stored as e4m3 with one fp32 scale per output channel
    (:func:`mark_fp8`); not with MoE models, ``tp`` or ``sp``. ``weight_dtype="fp8-experts"``: the
    same storage for the expert weights (``w_gate_up``, ``w_down``) of an MoE model only — router,
    attention and LM head stay bf16; not with a model without experts, ``tp`` or ``sp``.
    ``act_dtype="fp8"`` (checked here, acted on by the executor: the DAG and the stored bytes do
    not depend on it) needs ``weight_dtype="fp8"`` or ``"mxfp4"``. ``weight_dtype="mxfp4"``: the
    tensors ``"fp8"`` marks, stored as OCP MXFP4 (e2m1 pairs + one e8m0 scale per 32 elements of K,
    0.53 bytes per element); dense models only, no ``tp`` / ``sp``, every marked K a multiple of
    32, and ``act_dtype="fp8"`` (the one kernel is W4A8). ``weight_dtype="mxfp4-experts"``: the
    tensors ``"fp8-experts"`` marks, stored as MXFP4 — router, attention and LM head stay bf16; not
    with a model without experts, ``tp`` or ``sp``; every marked K a multiple of 32, and
    ``act_dtype="fp8"`` (the grouped kernel is W4A8). ``kv_cache=C``: ``seq`` is the number of new
    tokens per step and every attention node keeps a KV cache of C positions (:func:`add_kv_cache`).
    ``kv_dtype="fp8"`` (needs ``kv_cache``; independent of ``weight_dtype`` / ``act_dtype``): the
    caches hold e4m3 bytes and one fp32 scale per (position, KV head) (:func:`kv_cache_bytes`).
    ``generate=True`` (needs ``kv_cache`` and ``seq == 1``): every request's ``lm_head`` op carries
    ``attrs["sample"]``, the request's ordinal, and the executor samples the next token after it.
    ``moe_decode=True`` (needs ``kv_cache``, an MoE model and ``weight_dtype="bf16"``): lifts the
    cache's refusal of MoE models (:func:`check_moe_decode`); the DAG is the model's own."""
    check_kv_dtype(kv_dtype, kv_cache)
    check_generate(generate, seq, kv_cache)
    known = WEIGHT_DTYPES + MX_WEIGHT_DTYPES + MX_EXPERT_WEIGHT_DTYPES
    if weight_dtype not in known:
        raise ValueError(f"weight_dtype must be one of {known}, got {weight_dtype!r}")
    check_act_dtype(act_dtype, weight_dtype)
    cfg = get_config(model)
    if weight_dtype == "fp8":
        if cfg.n_experts:
            raise ValueError("weight_dtype='fp8' does not cover MoE models: weight_dtype='fp8-experts' stores "
                             "their expert weights as fp8 (attention, router and LM head stay bf16)")
        if tp > 1 or sp > 1:
            raise ValueError("weight_dtype='fp8' does not combine with tensor or sequence parallelism (tp, sp > 1)")
    if weight_dtype == "mxfp4":
        if cfg.n_experts:
            raise ValueError("weight_dtype='mxfp4' does not cover MoE models (dense models only)")
        if tp > 1 or sp > 1:
            raise ValueError("weight_dtype='mxfp4' does not combine with tensor or sequence parallelism (tp, sp > 1)")
    if weight_dtype == "fp8-experts":
        if not cfg.n_experts:
            raise ValueError(f"weight_dtype='fp8-experts' needs an MoE model; {model} has no experts "
                             "(weight_dtype='fp8' covers dense models)")
        if tp > 1 or sp > 1:
            raise ValueError("weight_dtype='fp8-experts' does not combine with tensor or sequence parallelism "
                             "(tp, sp > 1)")
    if weight_dtype in MX_EXPERT_WEIGHT_DTYPES:
        if not cfg.n_experts:
            raise ValueError(f"weight_dtype={weight_dtype!r} needs an MoE model; {model} has no experts "
                             "(weight_dtype='mxfp4' covers dense models)")
        if tp > 1 or sp > 1:
            raise ValueError(f"weight_dtype={weight_dtype!r} does not combine with tensor or sequence parallelism "
                             "(tp, sp > 1)")
    check_moe_decode(moe_decode, cfg, kv_cache, weight_dtype)
    if kv_cache is not None:
        check_kv_cache(cfg, seq, kv_cache, tp, sp, moe_decode)
    tasks: List[Task] = []
    for r in range(replicas):
        tasks.extend(build_dag(cfg, batch, seq, cost_model, prefix=f"r{r}/" if replicas > 1 else ""))
    if kv_cache is not None:
        add_kv_cache(tasks, batch, seq, kv_cache, cost_model, kv_dtype)
    if generate:
        for t in tasks:
            if t.op is not None and t.op.kind == "lm_head":
                t.op.attrs["sample"] = int(t.id.split("/", 1)[0][1:]) if replicas > 1 else 0
    groups = param_groups(cfg)
    if tp > 1:
        from .transforms import tensor_parallel
        tasks, groups = tensor_parallel(tasks, groups, cfg, tp)
    if sp > 1:
        if tp > 1:
            raise ValueError("combine sequence and tensor parallelism through separate DAGs (not both)")
        from .transforms import sequence_parallel
        tasks, groups = sequence_parallel(tasks, groups, cfg, sp)
    if weight_dtype == "fp8":
        mark_fp8(tasks, groups)
    elif weight_dtype == "fp8-experts":
        mark_fp8(tasks, groups, _EXPERT_OPERANDS)
    elif weight_dtype == "mxfp4":
        mark_fp8(tasks, groups, fmt="mxfp4")
    elif weight_dtype in MX_EXPERT_WEIGHT_DTYPES:
        mark_fp8(tasks, groups, _EXPERT_OPERANDS, fmt="mxfp4")
    return tasks, groups, cfg
