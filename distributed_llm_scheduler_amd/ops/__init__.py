"""Operator layer: hand-written HIP/CDNA4 kernels with fp32 PyTorch references.

``ops.linear(x, w, ...)`` etc. dispatch on the tensor's device:

* GPU tensors run the HIP kernels in ``_dlsched_ops`` (csrc/kernels/*.hip, built for
  gfx950). If the extension cannot be loaded on a GPU box this raises — there is no
  silent eager fallback for GPU tensors.
* CPU tensors run the ``ref_*`` implementations (fp32 math, result cast back to the
  input dtype). They define the numerics the kernels are tested against and power the
  CPU "fake device" executor used by the multi-process tests.

Weight layout everywhere: GEMM weights are ``[N][K]`` (K contiguous); ``y = x @ W^T``.
"""
from __future__ import annotations

import math
import os
import threading
from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from . import tuning

ACT = {None: 0, "none": 0, "gelu": 1, "gelu_tanh": 1, "silu": 2, "relu": 3, "swiglu": 4}
SWIGLU = 4
SWIGLU_BLOCK = 16  # gate/up interleave granularity of a SwiGLU-epilogue weight (csrc common.h)
# cache policy of vocabulary-sized projections (the LM head: a weight read once per step and a
# write-once logits tensor; GemmArgs::stream_pol): bit 0 weight DMA nt, bit 1 output stores nt.
# Streaming both keeps GPT-2's 170 MB of layer weights resident in the 256 MB Infinity Cache
# from step to step (its 77 MB LM-head weight and 51 MB of logits otherwise push them out):
# step 0.639 vs 0.689 ms (profiles/r4_ab/lmhead_stream_policy.txt)
LMHEAD_POL = int(os.environ.get("DLS_LMHEAD_POL", "3"))
LMHEAD_MIN_N = 32000
# weights of at least this many MB DMA'd with the nt policy (0: off) — for models whose weights
# stream from HBM every step anyway (A/B knob)
WEIGHT_NT_MB = float(os.environ.get("DLS_WEIGHT_NT_MB", "0"))
# cache policy bits of every other GEMM launch: 2 output stores nt, 4 output stores
# write-through (sc1) — bf16 outputs, split-K partial slabs and their reduce kernels' outputs
# leave the XCD's L2 as they are written, so the kernel boundary has no dirty lines to write
# back: GPT-2 0.620 vs 0.640 ms, Llama-3-8B 9.46 vs 9.49 ms (profiles/r4_ab/write_through.txt);
# nt output stores cost GPT-2 5 %
ACT_POL = int(os.environ.get("DLS_ACT_POL", "4"))
# per-model default where the measurement disagrees (DLS_ACT_POL, when set, wins): Mixtral-8x7B's
# step is faster with default-policy output stores, 24.40 / 24.50 vs 24.68 / 24.75 ms
# (profiles/r5_ab/knob_recheck.txt)
ACT_POL_MODEL = {"mixtral-8x7b": 0}
_ACT_POL_SET = "DLS_ACT_POL" in os.environ
# attention flags: bit 0 output stores write-through (no measurable difference), bit 1 the
# blocks of one head grouped on one XCD (A/B knob)
ATTN_FLAGS = int(os.environ.get("DLS_ATTN_FLAGS", "0"))
# attention kernel variant (0: the launcher's choice by grid size; 1..13: attention.hip)
ATTN_VARIANT = int(os.environ.get("DLS_ATTN_VARIANT", "0"))


# the LM-head policy pays only while the model's layer weights can stay MALL-resident: a
# vocabulary projection whose own weight is this large belongs to a model whose weights stream
# from HBM every step anyway, and there nt weight DMA slows the LM head itself (Llama-3-8B's
# 1 GB LM head: 683 vs 432 us per step, profiles/r4_ab/lmhead_stream_policy.txt)
LMHEAD_POL_MAX_MB = 128


def _stream_pol(N: int, K: int) -> int:
    lm = N >= LMHEAD_MIN_N and N * K * 2 <= LMHEAD_POL_MAX_MB * 1e6
    pol = LMHEAD_POL if lm else (ACT_POL if _ACT_POL_SET else ACT_POL_MODEL.get(tuning._model, ACT_POL))
    if WEIGHT_NT_MB > 0 and N * K * 2 >= WEIGHT_NT_MB * 1e6:
        pol |= 1
    return pol

_lock = threading.Lock()
_ext = None
_ext_err: Optional[BaseException] = None


def _load_ext():
    global _ext, _ext_err
    if _ext is not None:
        return _ext
    with _lock:
        if _ext is None:
            try:
                from .. import _build
                if os.environ.get("DLS_SKIP_BUILD") != "1":
                    _build.build_ops()
                import importlib
                _ext = importlib.import_module("distributed_llm_scheduler_amd._dlsched_ops")
            except BaseException as e:  # noqa: BLE001 - re-raised with context in ext()
                _ext_err = e
    return _ext


def ext():
    """The compiled HIP op library; raises if it is unavailable (never falls back)."""
    m = _load_ext()
    if m is None:
        raise RuntimeError(f"HIP kernel library _dlsched_ops is not available: {_ext_err!r}")
    return m


def native_available() -> bool:
    return _load_ext() is not None


def _gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


# ----------------------------------------------------------------- references (fp32)

def _act_ref(y: torch.Tensor, act) -> torch.Tensor:
    a = ACT[act] if not isinstance(act, int) else act
    if a == 1:
        return F.gelu(y, approximate="tanh")
    if a == 2:
        return F.silu(y)
    if a == 3:
        return F.relu(y)
    return y


def interleave_gate_up(w: torch.Tensor) -> torch.Tensor:
    """[gate (F rows); up (F rows)] -> rows interleaved in blocks of 16 (gate 16c..16c+15, then
    up 16c..16c+15) — the layout the GEMM's SwiGLU epilogue pairs fragments in. Works for a
    weight [2F, K] or a per-row vector [2F] (bias, colsum)."""
    F2 = w.shape[0]
    assert F2 % (2 * SWIGLU_BLOCK) == 0, "SwiGLU width must be a multiple of 16"
    F = F2 // 2
    rest = tuple(w.shape[1:])
    g = w[:F].reshape((F // SWIGLU_BLOCK, SWIGLU_BLOCK) + rest)
    u = w[F:].reshape((F // SWIGLU_BLOCK, SWIGLU_BLOCK) + rest)
    return torch.stack([g, u], 1).reshape((F2,) + rest).contiguous()


def rope_pair_perm(n_q_heads: int, n_k_heads: int, head_dim: int, total_rows: int) -> torch.Tensor:
    """Row order making every RoPE pair adjacent within each q / k head: new row 2i of a head
    is its old row i, new 2i+1 is old i + D/2 (V rows untouched). q.k is invariant under a
    permutation applied to both, so attention needs nothing else."""
    half = head_dim // 2
    within = torch.stack([torch.arange(half), torch.arange(half) + half], 1).reshape(-1)
    idx = torch.arange(total_rows)
    for h in range(n_q_heads + n_k_heads):
        idx[h * head_dim:(h + 1) * head_dim] = h * head_dim + within
    return idx


def _rope_ref_pairs(y: torch.Tensor, rope) -> torch.Tensor:
    cos_t, sin_t, S, D, cols = rope
    M = y.shape[0]
    pos = torch.arange(M) % S
    c = cos_t.cpu()[pos].float()
    sn = sin_t.cpu()[pos].float()
    heads = cols // D
    v = y[:, :cols].reshape(M, heads, D // 2, 2)
    x0, x1 = v[..., 0], v[..., 1]
    cc, ss = c[:, None, :], sn[:, None, :]
    out = torch.stack([x0 * cc - x1 * ss, x1 * cc + x0 * ss], -1).reshape(M, cols)
    return torch.cat([out, y[:, cols:]], 1)


def _swiglu_interleaved(y: torch.Tensor) -> torch.Tensor:
    F2 = y.shape[-1]
    v = y.reshape(y.shape[:-1] + (F2 // (2 * SWIGLU_BLOCK), 2, SWIGLU_BLOCK))
    return (F.silu(v[..., 0, :]) * v[..., 1, :]).reshape(y.shape[:-1] + (F2 // 2,))


def ref_linear(x, w, bias=None, act=None, residual=None, alpha=1.0, rope=None):
    y = alpha * (x.float() @ w.float().t())
    if bias is not None:
        y = y + bias.float()
    if rope is not None:
        y = _rope_ref_pairs(y.reshape(-1, y.shape[-1]), rope).reshape(y.shape)
    if (ACT[act] if not isinstance(act, int) else act) == SWIGLU:
        y = _swiglu_interleaved(y)
        return (y if residual is None else y + residual.float()).to(x.dtype)
    y = _act_ref(y, act)
    if residual is not None:
        y = y + residual.float()
    return y.to(x.dtype)


def ref_layernorm(x, w, b, eps=1e-5):
    return F.layer_norm(x.float(), (x.shape[-1],), w.float(), None if b is None else b.float(), eps).to(x.dtype)


def ref_rmsnorm(x, w, eps=1e-5):
    xf = x.float()
    return (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps) * w.float()).to(x.dtype)


def ref_attention(q, k, v, B, S, n_head, n_kv_head, head_dim, causal=True, scale=None, Sq=None, q_off=0):
    """q [B*Sq][>=nh*D], k/v [B*S][>=nkv*D] (row views into a packed qkv buffer allowed).
    ``Sq``/``q_off``: the queries are the sequence chunk at positions q_off .. q_off+Sq-1
    attending keys 0 .. S-1 (causal: key <= query position)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(head_dim)
    Sq = S if Sq is None else Sq
    qh = q[:, :n_head * head_dim].float().reshape(B, Sq, n_head, head_dim).transpose(1, 2)
    kh = k[:, :n_kv_head * head_dim].float().reshape(B, S, n_kv_head, head_dim).transpose(1, 2)
    vh = v[:, :n_kv_head * head_dim].float().reshape(B, S, n_kv_head, head_dim).transpose(1, 2)
    rep = n_head // n_kv_head
    if rep > 1:
        kh = kh.repeat_interleave(rep, dim=1)
        vh = vh.repeat_interleave(rep, dim=1)
    s = (qh @ kh.transpose(-1, -2)) * scale
    if causal:
        qpos = torch.arange(Sq, device=q.device)[:, None] + q_off
        mask = torch.arange(S, device=q.device)[None, :] > qpos
        s = s.masked_fill(mask, float("-inf"))
    o = torch.softmax(s, dim=-1) @ vh
    return o.transpose(1, 2).reshape(B * Sq, n_head * head_dim).to(q.dtype)


def rope_tables(S: int, head_dim: int, theta: float, device="cpu") -> Tuple[torch.Tensor, torch.Tensor]:
    inv = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.float64) / head_dim))
    ang = torch.arange(S, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().float().contiguous().to(device), ang.sin().float().contiguous().to(device)


def ref_rope_(qkv, S, n_head, n_kv_head, head_dim, k_col, cos_t, sin_t):
    M = qkv.shape[0]
    pos = torch.arange(M, device=qkv.device) % S
    c, s = cos_t[pos].to(qkv.device), sin_t[pos].to(qkv.device)
    half = head_dim // 2

    def rot(view, heads):
        x = view.float().reshape(M, heads, head_dim)
        x1, x2 = x[..., :half], x[..., half:]
        cc, ss = c[:, None, :], s[:, None, :]
        out = torch.cat([x1 * cc - x2 * ss, x2 * cc + x1 * ss], dim=-1)
        view.copy_(out.reshape(M, heads * head_dim).to(view.dtype))

    rot(qkv[:, :n_head * head_dim], n_head)
    rot(qkv[:, k_col:k_col + n_kv_head * head_dim], n_kv_head)
    return qkv


# --------------------------------------------------------------------- dispatchers

def _post_norm_args(post_norm):
    """(out, w, b, kind, eps) -> kwargs of the native post-norm (kind "layernorm" / "rmsnorm")."""
    y, nw, nb, kind, eps = post_norm
    return dict(norm_out=y, norm_w=nw, norm_b=nb if kind == "layernorm" else None,
                norm_mode=1 if kind == "layernorm" else 2, norm_eps=float(eps))


def _post_norm_ref(src, post_norm):
    y, nw, nb, kind, eps = post_norm
    s2 = src.reshape(-1, src.shape[-1])
    r = ref_layernorm(s2, nw, nb, eps) if kind == "layernorm" else ref_rmsnorm(s2, nw, eps)
    y.view(r.shape).copy_(r)


def linear(x, w, bias=None, act=None, residual=None, alpha=1.0, out=None, rows=None, rows_hint=None,
           compact=False, rope=None, stats_out=None, post_norm=None):
    """``act(alpha * x @ w^T + bias) + residual`` — one MFMA GEMM kernel with the whole
    epilogue fused on GPU. ``act="swiglu"`` takes a gate/up-interleaved weight
    (:func:`interleave_gate_up`) and returns the N/2-wide ``silu(gate) * up``. ``rows``
    (int32[2] tensor on x's device) restricts the GEMM to rows [rows[0], rows[1]) of x and
    ``out`` without a host sync (MoE experts); ``rows_hint`` is the expected row count used
    to pick the tuned kernel config; ``compact`` writes the range to rows 0..r1-r0-1 of ``out``
    (at most ``out.shape[0]`` rows). ``rope=(cos, sin, S, D, cols)`` rotates output columns
    [0, cols) in the epilogue (q/k rows pair-interleaved, :func:`rope_pair_perm`). ``stats_out``
    (GPU, fp32 [M, 2], zeroed by the caller): accumulate each output row's (sum, sum of
    squares) for the next folded norm (:func:`linear_norm` ``ext_stats``). ``post_norm =
    (y, w, b, "rmsnorm" | "layernorm", eps)``: also write the NEXT norm of the output rows into
    ``y`` (a split-K launch does it in its row-owning reduce, saving the norm launch)."""
    a = ACT[act] if not isinstance(act, int) else act
    n_out = w.shape[0] // 2 if a == SWIGLU else w.shape[0]
    if _gpu(x):
        shp = x.shape[:-1] + (n_out,)
        M = x.numel() // x.shape[-1]
        cfg, sk = tuning.lookup(rows_hint or M, w.shape[0], w.shape[1], tuning.tag(a, rows is not None))
        if cfg == tuning.LIB:  # (only with DLS_ALLOW_VENDOR_GEMM=1: tuning.lookup)
            if tuning.VENDOR and a == 0 and residual is None and rows is None and rope is None \
                    and stats_out is None and post_norm is None:
                # opt-in: a PLAIN GEMM (no fused epilogue) whose tuned choice is the vendor
                # library (hipBLASLt via torch); every fused-epilogue GEMM stays on the HIP kernels
                x2 = x.reshape(M, x.shape[-1])
                o2 = out.view(M, n_out) if out is not None else torch.empty(M, n_out, dtype=x.dtype, device=x.device)
                if bias is not None:
                    torch.addmm(bias, x2, w.t(), beta=1.0, alpha=float(alpha), out=o2)
                else:
                    torch.mm(x2, w.t(), out=o2)
                    if alpha != 1.0:
                        o2.mul_(alpha)
                return o2.view(shp) if out is None else out
            cfg, sk = tuning.lookup_fused(rows_hint or M, w.shape[0], w.shape[1], tuning.tag(a, rows is not None))
        # (a wave-private choice the family refuses for this epilogue: the same tile's K-grouped config)
        cfg, sk = tuning.resolve_private((cfg, sk), w.shape[1], a, rows is not None, rope is not None)
        # (the 64-row family takes folded-norm launches only: what the table held before)
        cfg, sk = tuning.resolve_private_wide((cfg, sk), w.shape[1], a, rows is not None, rope is not None)
        rc, rs_, rS, rD, rcols = rope if rope is not None else (None, None, 1, 2, 0)
        y = ext().gemm(x, w, bias, residual, a, float(alpha), out, cfg, sk, None, 0, 1e-5, rows, bool(compact),
                       rc, rs_, int(rS), int(rD), int(rcols), stats_out, None,
                       stream_pol=_stream_pol(w.shape[0], w.shape[1]) if rows is None else 0,
                       **(_post_norm_args(post_norm) if post_norm is not None else {}))
        return y.view(shp) if out is None else out
    if rows is not None:
        r0, r1 = (int(v) for v in rows.tolist())
        if out is None:
            out = torch.zeros(x.shape[:-1] + (n_out,), dtype=x.dtype)
        res = residual[r0:r1] if residual is not None else None
        o2 = out.reshape(-1, out.shape[-1])
        if compact:
            n = min(r1 - r0, o2.shape[0])
            o2[:n] = ref_linear(x[r0:r0 + n], w, bias, act, None, alpha)
        else:
            o2[r0:r1] = ref_linear(x[r0:r1], w, bias, act, res, alpha)
        return out
    y = ref_linear(x, w, bias, act, residual, alpha, rope=rope)
    if out is not None:
        out.copy_(y)
        y = out
    if post_norm is not None:
        _post_norm_ref(y, post_norm)
    return y


def quantize_fp8(w):
    """bf16 GEMM weight [N, K] -> ``(q, scale)``: OCP e4m3 (``torch.float8_e4m3fn``, K
    contiguous) and one fp32 POWER-OF-TWO scale per output channel, the smallest 2^e with
    ``amax_n / 2^e <= 448`` (an all-zero row: 1); round-to-nearest, saturating at +-448, no NaN
    code. ``W[n][k] ~= q[n][k] * scale[n]``, and that product is exactly a bf16 value. Runs on
    ``w``'s device."""
    from ..models.params import quantize_fp8 as _q
    return _q(w)


def dequantize_fp8(q, scale, dtype=torch.bfloat16):
    """``q[n][k] * scale[n]`` as ``dtype`` (exact in bf16 for power-of-two scales)."""
    from ..models.params import dequantize_fp8 as _d
    return _d(q, scale, dtype)


W8_SPLITS = (1, 2, 4, 8)  # split-K factors of the fp8-weight GEMM (csrc/kernels/gemm_w8.hip)


def w8_configs() -> int:
    """Number of tile configurations of the fp8-weight GEMM (``linear_w8(config=...)``)."""
    return int(ext().gemm_w8_num_configs())


def w8_workspace_elems(M: int, N: int, K: int) -> int:
    """fp32 elements of split-K workspace the shape's automatic config needs (0: no K split)."""
    _, sk = ext().gemm_w8_pick(int(M), int(N), int(K))
    return int(sk) * int(M) * int(N) if sk > 1 else 0


def linear_w8(x, q, scale, bias=None, act=None, residual=None, alpha=1.0, out=None, config=None, workspace=None):
    """``act(alpha * scale[n] * sum_k x[m][k] * q[n][k] + bias[n]) + residual`` with an fp8
    weight: ``q`` e4m3 [N, K] (K contiguous, K % 16 == 0), ``scale`` fp32 [N] (any positive
    values), fp32 accumulation, bf16 output. GPU: one HIP kernel (gemm_w8.hip: the fp8 bytes go
    through LDS, are converted to bf16 in registers and multiplied on the bf16 MFMA; the scale
    is applied in the epilogue). ``act="swiglu"``: the rows of ``q`` and ``scale`` interleave
    gate and up in blocks of ``SWIGLU_BLOCK`` (:func:`interleave_gate_up`), N/2 outputs.
    ``config``: ``None`` picks by shape; ``c`` forces tile configuration c (< :func:`w8_configs`)
    without a K split; ``(c, s)`` also splits K s ways (partial sums in fp32, reduced in a fixed
    order: bitwise reproducible). ``workspace`` (fp32, GPU): the split-K partial slabs, for
    callers that must not allocate (hipGraph capture). CPU tensors run :func:`ref_linear` on
    the dequantised weight."""
    a = ACT[act] if not isinstance(act, int) else act
    if q.dtype != torch.float8_e4m3fn:
        raise TypeError(f"linear_w8: the weight must be float8_e4m3fn, got {q.dtype}")
    if _gpu(x):
        n_out = q.shape[0] // 2 if a == SWIGLU else q.shape[0]
        cfg, sk = (-1, 0) if config is None else (tuple(config) if isinstance(config, (tuple, list)) else (config, 1))
        y = ext().gemm_w8(x, q, scale, bias, residual, a, float(alpha), out, int(cfg), int(sk),
                          _stream_pol(q.shape[0], q.shape[1]) & 6, workspace)
        return y.view(x.shape[:-1] + (n_out,)) if out is None else out
    if x.shape[-1] % 16:
        raise ValueError(f"linear_w8: K must be a multiple of 16, got {x.shape[-1]}")
    y = ref_linear(x, dequantize_fp8(q, scale, torch.float32), bias, act, residual, alpha)
    if out is not None:
        out.copy_(y.reshape(out.shape))
        return out
    return y


W8A8_SPLITS = (1, 2, 4, 8)  # split-K factors of the fp8 x fp8 GEMM (csrc/kernels/gemm_w8a8.hip)


def w8a8_configs() -> int:
    """Number of tile configurations of the fp8 x fp8 GEMM (``linear_w8a8(config=...)``)."""
    return int(ext().gemm_w8a8_num_configs())


def w8a8_workspace_elems(M: int, N: int, K: int) -> int:
    """fp32 elements of split-K workspace the shape's automatic config needs (0: no K split)."""
    _, sk = ext().gemm_w8a8_pick(int(M), int(N), int(K))
    return int(sk) * int(M) * int(N) if sk > 1 else 0


def _as_e4m3(t):
    """A caller's 1-byte buffer (the executor's uint8 scratch) seen as e4m3."""
    return t if t is None or t.dtype == torch.float8_e4m3fn else t.view(torch.float8_e4m3fn)


def _q8_out(q, s, out_q, out_scale):
    if out_q is not None:
        _as_e4m3(out_q).view(torch.uint8).copy_(q.reshape(out_q.shape).view(torch.uint8))
        q = _as_e4m3(out_q)
    if out_scale is not None:
        out_scale.copy_(s)
        s = out_scale
    return q, s


def quantize_rows_fp8(x, out_q=None, out_scale=None):
    """bf16 activation rows ``x`` [M, K] (rows may be strided) -> ``(q, scale)``: e4m3 [M, K] and
    one fp32 power-of-two scale per ROW, exactly :func:`quantize_fp8` of ``x`` (byte for byte,
    up to the sign of a zero). GPU: one launch of quant_rows.hip, which allocates nothing when
    ``out_q`` (1-byte elements, contiguous) and ``out_scale`` are given. CPU tensors run
    :func:`quantize_fp8`."""
    if _gpu(x):
        q, s = ext().quantize_rows_fp8(x, _as_e4m3(out_q), out_scale)
        return q.view(x.shape), s
    q, s = quantize_fp8(x.reshape(-1, x.shape[-1]))
    q, s = _q8_out(q, s, out_q, out_scale)
    return q.view(x.shape), s


def _norm_q8(x, w, b, eps, residual, sum_out, out_q, out_scale, rms):
    if _gpu(x):
        q, s, sm = ext().norm_q8(x, w, b, float(eps), residual, rms, sum_out, _as_e4m3(out_q), out_scale)
        q = q.view(x.shape)
        return (q, s, sm.view(x.shape)) if residual is not None else (q, s)
    r = rmsnorm(x, w, eps, residual=residual, sum_out=sum_out) if rms \
        else layernorm(x, w, b, eps, residual=residual, sum_out=sum_out)
    y, sm = r if residual is not None else (r, None)
    q, s = quantize_rows_fp8(y, out_q, out_scale)
    return (q, s, sm) if residual is not None else (q, s)


def layernorm_q8(x, w, b, eps=1e-5, residual=None, sum_out=None, out_q=None, out_scale=None):
    """:func:`layernorm` emitting its output as quantised rows: ``(q, scale)`` bitwise what
    ``quantize_rows_fp8(layernorm(...))`` gives (the bf16-ROUNDED normalised value is what gets
    quantised), in ONE launch on GPU. With ``residual`` returns ``(q, scale, x + residual)``
    (``sum_out`` as in :func:`layernorm`). CPU tensors run the two-step composition."""
    return _norm_q8(x, w, b, eps, residual, sum_out, out_q, out_scale, False)


def rmsnorm_q8(x, w, eps=1e-5, residual=None, sum_out=None, out_q=None, out_scale=None):
    """:func:`rmsnorm` emitting quantised rows; see :func:`layernorm_q8`."""
    return _norm_q8(x, w, None, eps, residual, sum_out, out_q, out_scale, True)


def linear_w8a8(xq, xscale, q, scale, bias=None, act=None, residual=None, alpha=1.0, out=None, config=None,
                workspace=None):
    """``act(alpha * xscale[m] * scale[n] * sum_k xq[m][k] * q[n][k] + bias[n]) + residual`` with
    BOTH operands fp8: ``xq`` e4m3 [M, K] with fp32 row scales ``xscale`` [M]
    (:func:`quantize_rows_fp8`), ``q`` e4m3 [N, K] with fp32 channel scales ``scale`` [N]
    (any positive values), K contiguous, K % 16 == 0, fp32 accumulation, bf16 output. GPU: one
    HIP kernel on the block-scaled fp8 MFMA (gemm_w8a8.hip; neutral block scales, both scales in
    the epilogue). ``act="swiglu"``, ``config``, ``workspace`` and a strided ``out`` as
    :func:`linear_w8` (``config`` < :func:`w8a8_configs`, splits ``W8A8_SPLITS``). CPU tensors
    run :func:`ref_linear` on the two dequantised operands in fp32."""
    a = ACT[act] if not isinstance(act, int) else act
    if q.dtype != torch.float8_e4m3fn or xq.dtype != torch.float8_e4m3fn:
        raise TypeError(f"linear_w8a8: both operands must be float8_e4m3fn, got {xq.dtype} and {q.dtype}")
    if _gpu(xq):
        n_out = q.shape[0] // 2 if a == SWIGLU else q.shape[0]
        cfg, sk = (-1, 0) if config is None else (tuple(config) if isinstance(config, (tuple, list)) else (config, 1))
        y = ext().gemm_w8a8(xq, xscale, q, scale, bias, residual, a, float(alpha), out, int(cfg), int(sk),
                            _stream_pol(q.shape[0], q.shape[1]) & 6, workspace)
        return y.view(xq.shape[:-1] + (n_out,)) if out is None else out
    if xq.shape[-1] % 16:
        raise ValueError(f"linear_w8a8: K must be a multiple of 16, got {xq.shape[-1]}")
    xd = dequantize_fp8(xq.reshape(-1, xq.shape[-1]), xscale, torch.float32).reshape(xq.shape)
    y = ref_linear(xd, dequantize_fp8(q, scale, torch.float32), bias, act, residual, alpha).to(torch.bfloat16)
    if out is not None:
        out.copy_(y.reshape(out.shape))
        return out
    return y


def quantize_mxfp4(w):
    """bf16 GEMM weight [N, K] (K % 32 == 0) -> ``(q, s)`` in OCP MXFP4: ``q`` uint8 [N, K/2],
    element k of a row in the low (k even) / high (k odd) nibble of byte k/2 as e2m1 (bit 3 the
    sign, codes 0..7 = 0, 0.5, 1, 1.5, 2, 3, 4, 6), and ``s`` uint8 [N, K/32] e8m0, code c =
    2^(c - 127), the smallest power of two with ``amax_block / 2^e <= 6`` (an all-zero block:
    127); round-to-nearest-even, saturating at +-6. ``W[n][k] ~= e2m1(q[n][k]) * 2^(s[n][k/32] -
    127)``, exactly a bf16 value. Runs on ``w``'s device."""
    from ..models.params import quantize_mxfp4 as _q
    return _q(w)


def dequantize_mxfp4(q, s, dtype=torch.bfloat16):
    """``e2m1(q[n][k]) * 2^(s[n][k/32] - 127)`` as ``dtype`` [N, K] (exact in bf16)."""
    from ..models.params import dequantize_mxfp4 as _d
    return _d(q, s, dtype)


W4A8_SPLITS = (1, 2, 4, 8)  # split-K factors of the MXFP4 x fp8 GEMM (csrc/kernels/gemm_w4a8.hip)


def w4a8_configs() -> int:
    """Number of tile configurations of the MXFP4 x fp8 GEMM (``linear_w4a8(config=...)``)."""
    return int(ext().gemm_w4a8_num_configs())


def w4a8_workspace_elems(M: int, N: int, K: int) -> int:
    """fp32 elements of split-K workspace the shape's automatic config needs (0: no K split)."""
    _, sk = ext().gemm_w4a8_pick(int(M), int(N), int(K))
    return int(sk) * int(M) * int(N) if sk > 1 else 0


def linear_w4a8(xq, xscale, q, s, bias=None, act=None, residual=None, alpha=1.0, out=None, config=None,
                workspace=None):
    """``act(alpha * xscale[m] * sum_k xq[m][k] * W[n][k] + bias[n]) + residual`` with fp8
    activations and an MXFP4 weight: ``xq`` e4m3 [M, K] with fp32 row scales ``xscale`` [M]
    (:func:`quantize_rows_fp8`), ``W[n][k] = e2m1(q[n][k]) * 2^(s[n][k/32] - 127)`` in the layout
    of :func:`quantize_mxfp4` (``q`` uint8 [N, K/2], ``s`` uint8 [N, K/32], any code 0..254),
    K % 32 == 0, fp32 accumulation, bf16 output. GPU: one HIP kernel on the block-scaled MFMA
    with an fp4 and an fp8 operand (gemm_w4a8.hip; the hardware applies the block scales, the
    row scale is applied in the epilogue). ``act="swiglu"`` (rows of ``q`` and ``s`` interleaved
    together), ``config``, ``workspace`` and a strided ``out`` as :func:`linear_w8` (``config``
    < :func:`w4a8_configs`, splits ``W4A8_SPLITS``). CPU tensors run :func:`ref_linear` on the
    two dequantised operands in fp32."""
    a = ACT[act] if not isinstance(act, int) else act
    if xq.dtype != torch.float8_e4m3fn:
        raise TypeError(f"linear_w4a8: the activations must be float8_e4m3fn, got {xq.dtype}")
    if q.dtype != torch.uint8 or s.dtype != torch.uint8:
        raise TypeError(f"linear_w4a8: the MXFP4 weight and its block scales must be uint8, got {q.dtype} and {s.dtype}")
    K = xq.shape[-1]
    if K % 32:
        raise ValueError(f"linear_w4a8: K must be a multiple of 32, got {K}")
    if q.dim() != 2 or q.shape[1] != K // 2 or tuple(s.shape) != (q.shape[0], K // 32):
        raise ValueError(f"linear_w4a8: expected q [N, {K // 2}] and s [N, {K // 32}], got {tuple(q.shape)} and "
                         f"{tuple(s.shape)}")
    if _gpu(xq):
        n_out = q.shape[0] // 2 if a == SWIGLU else q.shape[0]
        cfg, sk = (-1, 0) if config is None else (tuple(config) if isinstance(config, (tuple, list)) else (config, 1))
        y = ext().gemm_w4a8(xq, xscale, q, s, bias, residual, a, float(alpha), out, int(cfg), int(sk),
                            _stream_pol(q.shape[0], K) & 6, workspace)
        return y.view(xq.shape[:-1] + (n_out,)) if out is None else out
    xd = dequantize_fp8(xq.reshape(-1, K), xscale, torch.float32).reshape(xq.shape)
    y = ref_linear(xd, dequantize_mxfp4(q, s, torch.float32), bias, act, residual, alpha).to(torch.bfloat16)
    if out is not None:
        out.copy_(y.reshape(out.shape))
        return out
    return y


def derive_norm_gemm(w, ln_w, ln_b=None, bias=None):
    """Fold a norm's affine into the following GEMM: returns (W' = W * ln_w, colsum(W') in
    fp32, bias' = bias + W @ ln_b). W' is rounded to bf16 BEFORE the column sums, so the
    epilogue's mean correction matches exactly what the MFMAs multiply."""
    wf = w.float()
    wd = (wf * ln_w.float()[None, :]).to(w.dtype)
    cs = wd.float().sum(1).contiguous()
    b = torch.zeros(w.shape[0], device=w.device) if bias is None else bias.float()
    if ln_b is not None:
        # an elementwise product + row sum, NOT ``wf @ ln_b``: that GEMV would run in the vendor
        # BLAS (hipBLASLt), which EXITS the process (status 1, "operation not permitted when
        # stream is capturing") when first used while another rank thread of the single-GPU
        # harness is capturing a graph — the round-5 driver GPU suite's silent death
        b = b + (wf * ln_b.float()[None, :]).sum(1)
    return wd, cs, b.to(w.dtype).contiguous()


def linear_norm(x, w_derived, colsum, bias_derived, mode, eps=1e-5, act=None, residual=None, out=None, rope=None,
                ext_stats=None):
    """``act(W . norm(x) + bias) + residual`` in ONE GEMM on the raw rows ``x`` (GPU), with
    ``(w_derived, colsum, bias_derived)`` from :func:`derive_norm_gemm`. ``mode`` is
    "layernorm" or "rmsnorm". Row statistics are accumulated in the GEMM's main loop, or —
    with ``ext_stats`` (fp32 [M, 2] sums emitted by x's producer) — read from there, which
    frees the tile config and split-K choice."""
    m = {"layernorm": 1, "rmsnorm": 2}[mode]
    a = ACT[act] if not isinstance(act, int) else act
    shp = x.shape[:-1] + (w_derived.shape[0] // 2 if a == SWIGLU else w_derived.shape[0],)
    M, N, K = x.numel() // x.shape[-1], w_derived.shape[0], w_derived.shape[1]
    split = tuning.col_split(M, N, K, tuning.tag(a)) if ext_stats is not None and rope is None and a != SWIGLU \
        else None
    if split:
        # one launch per column range (e.g. the LM head: a whole round of 256 x 256 tiles, then
        # the remaining columns as one round of 256 x 144 tiles) into column views of ``out``
        if out is None:
            out = torch.empty(shp, dtype=x.dtype, device=x.device)
        o2 = out.view(M, N)
        r2 = residual.reshape(M, N) if residual is not None else None
        pol = _stream_pol(N, K)
        for n0, n1, c, k in split:
            ext().gemm(x, w_derived[n0:n1], bias_derived[n0:n1] if bias_derived is not None else None,
                       r2[:, n0:n1] if r2 is not None else None, a, 1.0, o2[:, n0:n1], int(c), int(k),
                       colsum[n0:n1], m, float(eps), None, False, None, None, 1, 2, 0, None, ext_stats,
                       stream_pol=pol)
        return out
    cfg, sk = tuning.resolve_private(tuning.lookup_fused(M, N, K, tuning.tag(a)), K, a, folded=True)
    # a 64-row wave-private id goes through when that family takes the launch, else its fallback
    cfg, sk = tuning.resolve_private_wide((cfg, sk), K, a, rope=rope is not None, folded=True,
                                          ext_stats=ext_stats is not None, residual=residual is not None)
    if ext_stats is None:
        sk = 1
        if 0 <= cfg < tuning.REGSTAGE and tuning.kstep(cfg) != 64:
            # in-loop row statistics need one K group: the fastest such candidate of the shape
            # instead of the kernel's generic 64x64 fallback
            cfg = next((int(c) for c, _ in tuning.runner_ups(M, N, K, tuning.tag(a), 8)
                        if 0 <= c < tuning.REGSTAGE and tuning.kstep(c) == 64), -1)
    rc, rs_, rS, rD, rcols = rope if rope is not None else (None, None, 1, 2, 0)
    pol = _stream_pol(N, K)
    if cfg >= tuning.REGSTAGE and cfg not in tuning.PRIVATE_WIDE_CFGS:
        cfg = -1  # (register-staged choices have no folded norm: the kernel heuristic)
    y = ext().gemm(x, w_derived, bias_derived, residual, a, 1.0, out, cfg, sk, colsum,
                   m, float(eps), None, False, rc, rs_, int(rS), int(rD), int(rcols), None, ext_stats,
                   stream_pol=pol)
    return y.view(shp) if out is None else out


# ------------------------------------------------------------- dense skinny GEMM (M <= 16)

SKINNY_ROWS_LIMIT = 16  # rows the kernel of gemm_skinny.hip takes (one token fragment per wave)
SKINNY_WAVES = (4, 8, 16)  # its instances: waves per workgroup = ways K is split inside it
# Token rows of a decode step up to which the executor sends dense GEMMs to the skinny kernel, and
# whether vocabulary-sized projections (N >= LMHEAD_MIN_N) go there too: set by the measurements of
# profiles/skinny_gemm/ (README, "Dense skinny GEMM"). The captured llama3-8b-1l step with every
# dense GEMM skinny won every alternating round at 1 and 2 rows (1.08x), 4 of 5 at 4 rows, none at
# 8 and 16 (step_bound_search.txt): 2. The LM-head rows of the kernel table (kernels.txt) won every
# pair at M = 1, 2 and 4 on both models (Llama's 1.05 GB head: 162 against 197 us at M = 1), and the
# step without the skinny LM head is a tie with the tiles (step_lmhead_off.txt): True.
SKINNY_MAX_ROWS = 2
SKINNY_LMHEAD = True
_NORM_MODE = {"layernorm": 1, "rmsnorm": 2, 1: 1, 2: 2}


def skinny_waves(N: int, K: int, act=None) -> int:
    """Waves per workgroup ``linear_skinny`` launches with (the rule of gemm_skinny_waves in
    gemm_skinny.hip, mirrored here for the CPU back end), read off the kernel table of
    profiles/skinny_gemm/: 4 for SwiGLU, 16 for a vocabulary-sized N at K >= 2048, else 8."""
    a = ACT[act] if not isinstance(act, int) else act
    strips = N // 32 if a == SWIGLU else (N + 15) // 16
    nk = (K + 63) // 64
    if a == SWIGLU:
        return 4
    return 16 if strips >= 4096 and nk >= 32 else 8


def skinny_refusal(M, N, K, act=None, rope=None, norm=None, waves=None, lda=None, ldw=None) -> Optional[str]:
    """Why the skinny kernel does not take a launch (None: it does) — the rules of
    gemm_skinny_takes in gemm_skinny.hip."""
    try:
        a = ACT[act] if not isinstance(act, int) else act
    except KeyError:
        return f"unknown activation {act!r}"
    lda, ldw = (K if lda is None else lda), (K if ldw is None else ldw)
    if not 1 <= M <= SKINNY_ROWS_LIMIT:
        return f"M = {M}: the kernel takes 1..{SKINNY_ROWS_LIMIT} rows"
    if N < 1 or K < 32 or K % 32:
        return f"N = {N}, K = {K}: N >= 1 and K a positive multiple of 32"
    if lda % 8 or ldw % 8 or lda < K or ldw < K:
        return "row strides of x and w must be multiples of 8 elements"
    if a not in (0, 1, 2, 3, SWIGLU):
        return f"unknown activation {act!r}"
    if a == SWIGLU and N % 32:
        return f"SwiGLU needs N % 32 == 0, N = {N}"
    if rope is not None:
        _, _, S, D, cols = rope
        if a != 0 or cols <= 0 or cols % 4 or cols > N or D < 4 or D % 4 or cols % D or S < 1:
            return "RoPE needs no activation, cols % 4 == 0, whole heads (cols % D == 0) and D % 4 == 0"
    if norm is not None and norm[1] not in _NORM_MODE:
        return f"norm mode {norm[1]!r}: 'layernorm' or 'rmsnorm'"
    if waves is not None and waves not in SKINNY_WAVES:
        return f"waves = {waves}: one of {SKINNY_WAVES}"
    return None


def skinny_ok(M, N, K, act=None, rope=None, norm=None, waves=None, lda=None, ldw=None) -> bool:
    """Does the dense skinny kernel take an [M][K] x [N][K]^T launch with this epilogue?"""
    return skinny_refusal(M, N, K, act, rope, norm, waves, lda, ldw) is None


def _ref_linear_skinny(x, w, bias, act, residual, alpha, rope, norm):
    """fp32 reference of linear_skinny on the operands the kernel receives; a folded norm takes
    its row statistics from x."""
    a = ACT[act] if not isinstance(act, int) else act
    if norm is None:
        return ref_linear(x, w, bias, a, residual, alpha, rope=rope)
    colsum, mode, eps = norm
    xf = x.float()
    K = x.shape[-1]
    y = alpha * (xf @ w.float().t())
    ms = xf.pow(2).sum(-1, keepdim=True) / K
    if _NORM_MODE[mode] == 1:
        mu = xf.sum(-1, keepdim=True) / K
        y = torch.rsqrt((ms - mu * mu).clamp_min(0) + eps) * (y - mu * colsum.float())
    else:
        y = torch.rsqrt(ms + eps) * y
    if bias is not None:
        y = y + bias.float()
    if rope is not None:
        y = _rope_ref_pairs(y.reshape(-1, y.shape[-1]), rope).reshape(y.shape)
    y = _swiglu_interleaved(y) if a == SWIGLU else _act_ref(y, a)
    if residual is not None:
        y = y + residual.float()
    return y.to(x.dtype)


def linear_skinny(x, w, bias=None, act=None, residual=None, alpha=1.0, out=None, rope=None, norm=None, stream=False,
                  waves=None, **refused):
    """``act(alpha * x @ w^T + bias) + residual`` for the 1 <= M <= 16 rows of a decode step on the
    weight-streaming kernel of gemm_skinny.hip (GPU): a workgroup per 16-column strip, ``waves``
    waves (4, 8, 16; None: :func:`skinny_waves`) split K inside it and sum in a fixed order — no
    atomics, no workspace, two launches bit-identical, and a row's result does not depend on the
    other rows of the launch. Same operands as :func:`linear`: ``act="swiglu"`` takes the gate/up
    interleaved weight, ``rope=(cos, sin, S, D, cols)`` rotates pair-interleaved columns.
    ``norm=(colsum, mode, eps)`` folds a LayerNorm / RMSNorm of x's rows into the launch: ``w``,
    ``bias`` and ``colsum`` are the derived operands of :func:`derive_norm_gemm`, x holds the RAW
    rows and the kernel takes the row statistics itself. ``stream``: weight loads with the
    streaming (nt) cache policy — for weights that cannot stay in the Infinity Cache anyway.
    What the kernel does not take raises ``ValueError``: M > 16, K % 32 != 0, SwiGLU with
    N % 32 != 0, operands that are not bf16 or not 16-byte aligned rows, and the ``rows`` /
    ``compact`` / ``stats_out`` / ``ext_stats`` / ``post_norm`` arguments of :func:`linear`."""
    for k, v in refused.items():
        if k not in ("rows", "rows_hint", "compact", "stats_out", "ext_stats", "post_norm"):
            raise TypeError(f"linear_skinny() got an unexpected keyword argument {k!r}")
        if v is not None and v is not False and k != "rows_hint":
            raise ValueError(f"linear_skinny: `{k}` is not part of the skinny kernel's contract")
    if x.dim() < 2 or w.dim() != 2 or w.shape[1] != x.shape[-1]:
        raise ValueError("linear_skinny: x [..., K] and w [N][K]")
    a = ACT.get(act, -1) if not isinstance(act, int) else act
    K, N = x.shape[-1], w.shape[0]
    M = x.numel() // K
    x2 = x.reshape(M, K)
    if x.dtype != torch.bfloat16 or w.dtype != torch.bfloat16:
        raise ValueError("linear_skinny: bf16 operands only")
    if x2.stride(1) != 1 or w.stride(1) != 1 or x2.data_ptr() % 16 or w.data_ptr() % 16:
        raise ValueError("linear_skinny: rows of x and w must be contiguous and 16-byte aligned")
    why = skinny_refusal(M, N, K, a if a >= 0 else act, rope, norm, waves, x2.stride(0) if M > 1 else K, w.stride(0))
    if why is not None:
        raise ValueError(f"linear_skinny: {why}")
    n_out = N // 2 if a == SWIGLU else N
    for name, t, shp in (("bias", bias, (N,)), ("residual", residual, (M, n_out)), ("out", out, (M, n_out))):
        if t is not None and (t.dtype != torch.bfloat16 or t.numel() != math.prod(shp)):
            raise ValueError(f"linear_skinny: {name} must be bf16 {list(shp)}")
    if norm is not None and (norm[0].dtype != torch.float32 or norm[0].numel() != N):
        raise ValueError("linear_skinny: norm = (fp32 colsum [N], mode, eps)")
    r2 = residual if residual is None or residual.dim() == 2 else residual.reshape(M, n_out)
    o2 = out if out is None or out.dim() == 2 else out.view(M, n_out)
    if _gpu(x):
        rc, rs_, rS, rD, rcols = rope if rope is not None else (None, None, 1, 4, 0)
        cs, m, eps = (norm[0], _NORM_MODE[norm[1]], float(norm[2])) if norm is not None else (None, 0, 1e-5)
        y = ext().gemm_skinny(x2, w, bias, r2, a, float(alpha), o2, cs, m, eps, rc, rs_, int(rS), int(rD), int(rcols),
                              bool(stream), int(waves or 0))
        return y.view(x.shape[:-1] + (n_out,)) if out is None else out
    y = _ref_linear_skinny(x2, w, bias, a, r2, alpha, rope, norm).reshape(x.shape[:-1] + (n_out,))
    if out is not None:
        out.copy_(y.reshape(out.shape))
        return out
    return y


def mlp_fused_ok(M, H, F, Hout) -> bool:
    """Does the one-launch MLP block (gemm_fused.hip) take this shape on this GPU?"""
    return bool(ext().mlp_fused_ok(int(M), int(H), int(F), int(Hout)))


def mlp_fused(x, w1_derived, b1_derived, colsum1, ext_stats, mode, eps, h, w2, b2, residual, out, stats_out=None,
              sync=None, spin_limit=1 << 22):
    """A pre-norm transformer MLP block as ONE launch (GPU): ``h = GELU(W1'.norm(x) + b1')``
    (norm folded as in :func:`linear_norm`, row statistics handed over in ``ext_stats``) and
    ``out = h W2^T + b2 + residual`` (+ each output row's statistics into ``stats_out``), the two
    GEMMs linked inside the launch (fc1 tiles publish write-through, fc2 tiles start when their
    rows' fc1 tiles have arrived). ``sync``: zeroed int32 [2 * M / 64 + 1]; its last word is set
    if a wait gave up (never expected). ``h`` is written too (it is the DAG's activation)."""
    m = {"layernorm": 1, "rmsnorm": 2}[mode]
    if sync is None:
        sync = torch.zeros(2 * (x.numel() // x.shape[-1]) // 64 + 1, dtype=torch.int32, device=x.device)
    ext().mlp_fused(x, w1_derived, b1_derived, colsum1, ext_stats, m, float(eps), ACT["gelu"], h, w2, b2, residual,
                    out, stats_out, sync, int(spin_limit))
    return out


def attn_block_ok(M, H, B, S, n_head, n_kv_head, head_dim) -> bool:
    """Does the one-launch attention block (attn_block.hip) take this shape?"""
    return bool(ext().attn_block_ok(int(M), int(H), int(B), int(S), int(n_head), int(n_kv_head), int(head_dim)))


def attn_block_sync(M, S, B, n_head, device) -> torch.Tensor:
    """A zeroed counter buffer for :func:`attn_block` (the launch resets it; last word: error)."""
    return torch.zeros(int(ext().attn_block_sync_size(int(M), int(S), int(B), int(n_head))), dtype=torch.int32,
                       device=device)


def attn_block(x, w_qkv_derived, b_qkv_derived, colsum, ext_stats, mode, eps, qkv, o, w_o, b_o, residual, out,
               B, S, n_head, stats_out=None, sync=None, scale=None, spin_limit=1 << 22):
    """A pre-norm attention block as ONE launch (GPU, attn_block.hip): ``qkv = W'.norm(x) + b'``
    (norm folded as in :func:`linear_norm`, row statistics of x in ``ext_stats``), causal MHA
    over ``qkv`` into ``o``, ``out = o W_o^T + b_o + residual`` (+ each output row's statistics
    into ``stats_out``) — the three stages linked inside the launch by per-row-block arrival
    counters (a query tile starts once the q / k / v tiles of its rows and earlier ones exist;
    an out-proj tile once every head of its rows is done). ``qkv`` and ``o`` are written too."""
    m = {"layernorm": 1, "rmsnorm": 2}[mode]
    H = x.shape[-1]
    if sync is None:
        sync = attn_block_sync(x.numel() // H, S, B, n_head, x.device)
    scale = scale if scale is not None else 1.0 / math.sqrt(H // n_head)
    ext().attn_block(x, w_qkv_derived, b_qkv_derived, colsum, ext_stats, m, float(eps), qkv, o, w_o, b_o, residual,
                     out, stats_out, int(B), int(S), int(n_head), float(scale), sync, int(spin_limit))
    return out


def layernorm(x, w, b, eps=1e-5, residual=None, out=None, sum_out=None):
    """LayerNorm; with ``residual`` returns ``(LN(x + residual), x + residual)``."""
    if _gpu(x):
        y, s = ext().norm(x, w, b, float(eps), residual, False, out, sum_out)
        y = y.view(x.shape)
        return (y, s.view(x.shape)) if residual is not None else y
    if residual is not None:
        s = (x.float() + residual.float()).to(x.dtype)
        y = ref_layernorm(s, w, b, eps)
        if sum_out is not None:
            sum_out.copy_(s)
        if out is not None:
            out.copy_(y)
        return y, s
    y = ref_layernorm(x, w, b, eps)
    if out is not None:
        out.copy_(y)
    return y


def rmsnorm(x, w, eps=1e-5, residual=None, out=None, sum_out=None):
    if _gpu(x):
        y, s = ext().norm(x, w, None, float(eps), residual, True, out, sum_out)
        y = y.view(x.shape)
        return (y, s.view(x.shape)) if residual is not None else y
    if residual is not None:
        s = (x.float() + residual.float()).to(x.dtype)
        y = ref_rmsnorm(s, w, eps)
        if sum_out is not None:
            sum_out.copy_(s)
        if out is not None:
            out.copy_(y)
        return y, s
    y = ref_rmsnorm(x, w, eps)
    return out.copy_(y) if out is not None else y


def attention(q, k, v, B, S, n_head, n_kv_head, head_dim, causal=True, scale=None, out=None, Sq=None, q_off=0):
    """Flash attention (GPU) / fp32 reference (CPU). ``Sq``/``q_off``: a sequence chunk of
    queries at positions q_off.. against S keys (sequence-parallel attention nodes)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(head_dim)
    if _gpu(q):
        return ext().attention(q, k, v, B, S, n_head, n_kv_head, head_dim, causal, float(scale), out, ATTN_VARIANT,
                               int(Sq or 0), int(q_off), int(ATTN_FLAGS))
    y = ref_attention(q, k, v, B, S, n_head, n_kv_head, head_dim, causal, scale, Sq=Sq, q_off=q_off)
    if out is not None:
        out.copy_(y)
        return out
    return y


# ---------------------------------------------------------- KV cache and decode steps
# Caches are bf16 [B][C][n_kv_head*head_dim]; ``pos`` (int32 [B], on the caches' device) holds
# every sequence's length before the step, so a captured step follows a growing sequence.
# fp8 caches (``k_scale`` / ``v_scale`` given): uint8 e4m3 bytes of the same shape plus fp32
# power-of-two scales [B][n_kv_head][C], one per (position, KV head) by the rule of quantize_fp8.

DECODE_HEAD_DIMS = (64, 128)  # head_dim instances of the GPU decode attention kernel (the CPU path takes any)


def _kv_scales_ok(k_cache, v_cache, k_scale, v_scale, what):
    """Whether the caches are fp8; the checks the GPU binding makes, for the CPU path."""
    if (k_scale is None) != (v_scale is None):
        raise RuntimeError(f"{what}: k_scale and v_scale go together")
    fp8 = k_cache.dtype == torch.uint8
    if fp8 != (k_scale is not None):
        raise RuntimeError(f"{what}: uint8 (e4m3) caches need k_scale and v_scale" if fp8 else
                           f"{what}: k_scale / v_scale go with uint8 (e4m3) caches")
    if fp8:
        B, C, E = k_cache.shape
        for s_ in (k_scale, v_scale):
            if s_.dtype != torch.float32 or s_.dim() != 3 or s_.shape[0] != B or s_.shape[2] != C \
                    or s_.shape[1] < 1 or E % s_.shape[1] or s_.shape != k_scale.shape:
                raise RuntimeError(f"{what}: scales must be fp32 [B][n_kv_head][C]")
    return fp8


def kv_dequantize(cache, scale):
    """An fp8 cache (uint8 e4m3 [B][C][E]) and its scales (fp32 [B][n_kv_head][C]) as bf16
    [B][C][E]: exact, every e4m3 value times a power of two being a bf16 value."""
    B, C, E = cache.shape
    H = scale.shape[1]
    x = cache.view(torch.float8_e4m3fn).float().view(B, C, H, E // H)
    return (x * scale.transpose(1, 2)[..., None]).to(torch.bfloat16).view(B, C, E)


def kv_append(k_new, v_new, k_cache, v_cache, pos, T, k_scale=None, v_scale=None):
    """Rows ``pos[b] .. pos[b]+T-1`` of sequence b's caches <- rows ``b*T .. b*T+T-1`` of
    ``k_new`` / ``v_new`` ([B*T][>= n_kv_head*head_dim], column views of the packed qkv buffer
    allowed). Rows at or past the capacity C are dropped. With ``k_scale`` / ``v_scale`` the caches
    are fp8: every head's row is quantised by :func:`quantize_fp8` and its scale lands at
    ``[b][h][pos[b]+t]`` (GPU: attn_decode_fp8.hip)."""
    if _gpu(k_cache):
        ext().kv_append(k_new, v_new, k_cache, v_cache, pos, int(T), k_scale, v_scale)
        return
    fp8 = _kv_scales_ok(k_cache, v_cache, k_scale, v_scale, "kv_append")
    B, C, E = k_cache.shape
    for b, p in enumerate(pos.tolist()):
        n = max(0, min(T, C - p))
        if not fp8:
            k_cache[b, p:p + n] = k_new[b * T:b * T + n, :E]
            v_cache[b, p:p + n] = v_new[b * T:b * T + n, :E]
            continue
        if n == 0:
            continue
        H = k_scale.shape[1]
        for new, cache, sc in ((k_new, k_cache, k_scale), (v_new, v_cache, v_scale)):
            q, s_ = quantize_fp8(new[b * T:b * T + n, :E].to(torch.bfloat16).reshape(n * H, E // H))
            cache[b, p:p + n] = q.view(torch.uint8).view(n, E)
            sc[b, :, p:p + n] = s_.view(n, H).t()


def attention_decode_sizes(B, T, C, n_head, n_kv_head, head_dim, chunk=0):
    """(fp32 partial elements, int32 tickets) of ``attention_decode``'s workspace."""
    return ext().attention_decode_sizes(B, T, C, n_head, n_kv_head, head_dim, int(chunk))


def attention_decode_workspace(B, T, C, n_head, n_kv_head, head_dim, device, chunk=0):
    """The workspace of ``attention_decode``: (partials, tickets), allocated once by the caller
    (never inside a captured step); the tickets start at zero and reset themselves. The CPU path
    needs none."""
    if torch.device(device).type != "cuda":
        return None
    pf, nc = attention_decode_sizes(B, T, C, n_head, n_kv_head, head_dim, chunk)
    return (torch.empty(max(pf, 4), dtype=torch.float32, device=device),
            torch.zeros(max(nc, 1), dtype=torch.int32, device=device))


def ref_attention_decode(q, k_cache, v_cache, pos, T, n_head, n_kv_head, head_dim, scale=None):
    """fp32: query t of sequence b (row b*T + t of q) attends cache rows 0 .. pos[b]+t."""
    B, C, _E = k_cache.shape
    out = torch.zeros(B * T, n_head * head_dim, dtype=q.dtype, device=q.device)
    for b, p in enumerate(pos.tolist()):
        S = min(p + T, C)
        out[b * T:(b + 1) * T] = ref_attention(q[b * T:(b + 1) * T], k_cache[b, :S], v_cache[b, :S], 1, S, n_head,
                                               n_kv_head, head_dim, True, scale, Sq=T, q_off=p)
    return out


def attention_decode(q, k_cache, v_cache, pos, T, n_head, n_kv_head, head_dim, scale=None, out=None,
                     workspace=None, chunk=0, k_scale=None, v_scale=None):
    """Causal attention of the T new queries of every sequence (q [B*T][>= n_head*head_dim])
    against its cache rows ``0 .. pos[b]+t``; runs after ``kv_append``. GPU: attn_decode.hip with
    ``workspace`` from ``attention_decode_workspace`` (``chunk``: keys per workgroup, 0 = the
    launcher's choice; the workspace must be sized with the same value). CPU: fp32 torch. With
    ``k_scale`` / ``v_scale`` the caches are fp8 (attn_decode_fp8.hip; the workspace is the same);
    the CPU path dequantises them first."""
    scale = scale if scale is not None else 1.0 / math.sqrt(head_dim)
    if _gpu(q):
        if workspace is None:
            raise ValueError("attention_decode needs the workspace of attention_decode_workspace on the GPU")
        return ext().attention_decode(q, k_cache, v_cache, pos, int(T), n_head, n_kv_head, head_dim, float(scale),
                                      workspace[0], workspace[1], out, int(chunk), k_scale, v_scale)
    if _kv_scales_ok(k_cache, v_cache, k_scale, v_scale, "attention_decode"):
        if k_scale.shape[1] != n_kv_head:
            raise RuntimeError("attention_decode: scales must be fp32 [B][n_kv_head][C]")
        k_cache, v_cache = kv_dequantize(k_cache, k_scale), kv_dequantize(v_cache, v_scale)
    if not (1 <= T <= 16 and n_head % n_kv_head == 0 and n_head // n_kv_head * T <= 64):  # (any head_dim here)
        raise RuntimeError("attention_decode: needs 1 <= T <= 16 and (n_head / n_kv_head) * T <= 64 "
                           f"(T {T}, heads {n_head}/{n_kv_head})")
    y = ref_attention_decode(q, k_cache, v_cache, pos, T, n_head, n_kv_head, head_dim, scale)
    if out is not None:
        out[:, :n_head * head_dim].copy_(y)
        return out
    return y


# ---------------------------------------------------------- prompt chunks over the cache
CHUNK_MAX_T = 1024  # widest query chunk of attention_chunk
CHUNK_VARIANTS = (2, 8, 13)  # the (NW, ST, KS) configurations its launcher chooses among, by ops.attention's numbers


def kv_dequantize_rows(cache, scale, pos, T, out):
    """Rows ``0 .. min(pos[b]+T, C)-1`` of every sequence of an fp8 cache (uint8 e4m3 [B][C][E], scales
    fp32 [B][n_kv_head][C]) into ``out`` (bf16 [B][C][E]) as e4m3 x scale, each value exactly a bf16:
    :func:`kv_dequantize` on those rows, and no other row of ``out`` is touched. One launch on the
    GPU (attn_chunk.hip), ``pos`` read on the device."""
    if cache.dtype != torch.uint8 or cache.dim() != 3:
        raise RuntimeError("kv_dequantize_rows: the cache must be uint8 (e4m3) [B][C][n_kv_head*head_dim]")
    B, C, E = cache.shape
    if scale.dtype != torch.float32 or scale.dim() != 3 or scale.shape[0] != B or scale.shape[2] != C \
            or scale.shape[1] < 1 or E % scale.shape[1] or (E // scale.shape[1]) % 8:
        raise RuntimeError("kv_dequantize_rows: scales must be fp32 [B][n_kv_head][C], head_dim a multiple of 8")
    if out.dtype != torch.bfloat16 or out.shape != cache.shape or not out.is_contiguous() or T < 1:
        raise RuntimeError("kv_dequantize_rows: out must be contiguous bf16 of the cache's shape, T >= 1")
    if _gpu(cache):
        ext().kv_dequantize_rows(cache, scale, pos, int(T), out)
        return out
    for b, p in enumerate(pos.tolist()):
        n = min(max(min(p, C), 0) + T, C)
        out[b, :n] = kv_dequantize(cache[b:b + 1, :n], scale[b:b + 1, :, :n])[0]
    return out


def attention_chunk_variant(B, T, n_head, variant=0):
    """The configuration (one of ``CHUNK_VARIANTS``) the GPU launcher of ``attention_chunk`` takes."""
    return ext().attention_chunk_variant(int(B), int(T), int(n_head), int(variant))


def attention_chunk(q, k_cache, v_cache, pos, T, n_head, n_kv_head, head_dim, scale=None, out=None,
                    k_scale=None, v_scale=None, workspace=None, variant=0):
    """Causal attention of a prompt chunk: the ``T`` queries of every sequence (q [B*T][>=
    n_head*head_dim], 1 <= T <= 1024, any n_head / n_kv_head) against its cache rows; query row
    ``b*T + t`` attends rows ``0 .. min(pos[b]+t, C-1)``. Runs after ``kv_append``, as
    ``attention_decode`` does. ``pos`` (int32 [B]) is read on the device and the grid depends on
    (T, n_head, B) alone, so a captured launch follows a growing, ragged batch. Cache rows at or past
    ``pos[b]+T`` are never read; rows of query positions >= C are unspecified but finite.
    Cache rows below ``pos[b]+T`` must hold finite V values, also those a query does not see
    (``pos[b]+t < r < pos[b]+T``, written by the step's own append): a row of a loaded tile that the
    causal mask hides enters the product with V as ``0 x v`` on both paths, as in ``attention``.
    A hidden K row may hold anything: its score is replaced by the mask.
    GPU: attn_chunk.hip (``variant``: 0 = chosen by block count, or one of ``CHUNK_VARIANTS``).
    With ``k_scale`` / ``v_scale`` the caches are fp8: ``kv_dequantize_rows`` fills ``workspace`` —
    two bf16 [B][C][n_kv_head*head_dim] buffers (K, V) allocated by the caller — and the bf16 kernel
    runs on it. CPU: fp32 torch."""
    scale = scale if scale is not None else 1.0 / math.sqrt(head_dim)
    if k_cache.dim() != 3:
        raise RuntimeError("attention_chunk: caches must be [B][C][n_kv_head*head_dim]")
    if not (1 <= T <= CHUNK_MAX_T and n_kv_head >= 1 and n_head % n_kv_head == 0):
        raise RuntimeError("attention_chunk: needs 1 <= T <= 1024 and n_head a multiple of n_kv_head "
                           f"(T {T}, heads {n_head}/{n_kv_head})")
    if variant not in (0,) + CHUNK_VARIANTS:
        raise RuntimeError(f"attention_chunk: variant must be 0 or one of {CHUNK_VARIANTS}")
    fp8 = _kv_scales_ok(k_cache, v_cache, k_scale, v_scale, "attention_chunk")
    if fp8:
        if k_scale.shape[1] != n_kv_head:
            raise RuntimeError("attention_chunk: scales must be fp32 [B][n_kv_head][C]")
        if _gpu(q):
            if workspace is None or len(workspace) != 2:
                raise ValueError("attention_chunk with fp8 caches needs workspace=(k, v): two bf16 buffers of the "
                                 "caches' shape")
            k_cache = kv_dequantize_rows(k_cache, k_scale, pos, T, workspace[0])
            v_cache = kv_dequantize_rows(v_cache, v_scale, pos, T, workspace[1])
        else:
            k_cache, v_cache = kv_dequantize(k_cache, k_scale), kv_dequantize(v_cache, v_scale)
    if _gpu(q):
        return ext().attention_chunk(q, k_cache, v_cache, pos, int(T), n_head, n_kv_head, head_dim, float(scale), out,
                                     int(variant))
    y = ref_attention_decode(q, k_cache, v_cache, pos, T, n_head, n_kv_head, head_dim, scale)
    if out is not None:
        out[:, :n_head * head_dim].copy_(y)
        return out
    return y


def kv_advance(pos, limit, T, tmp=None):
    """``pos[b] = min(pos[b] + T, max(limit[b], pos[b]))`` in place (int32 [B] each): a chunk step's
    advance, which stops every sequence at its target and never moves one back. One tiny launch
    on the GPU. CPU: three in-place torch ops through ``tmp`` (int32 [B], the caller's), which
    allocate nothing; without ``tmp`` one such buffer is allocated."""
    if pos.dtype != torch.int32 or limit.dtype != torch.int32 or pos.shape != limit.shape or pos.dim() != 1 \
            or not 0 <= T < 1 << 30:
        raise RuntimeError("kv_advance: pos and limit must be int32 [B], 0 <= T < 2^30")
    if _gpu(pos):
        ext().kv_advance(pos, limit, int(T))
        return
    if tmp is None:
        tmp = torch.empty_like(pos)
    elif tmp.dtype != torch.int32 or tmp.shape != pos.shape:
        raise RuntimeError("kv_advance: tmp must be int32 [B]")
    torch.maximum(limit, pos, out=tmp)
    pos.add_(int(T))
    torch.minimum(pos, tmp, out=pos)


def decode_prologue(pos, T, C, tokens=None, tok_out=None, tables=(), outs=()):
    """One launch per step: ``tok_out[b*T + t] = tokens[b][p]`` and ``outs[i][b*T + t] =
    tables[i][p]`` at ``p = min(pos[b] + t, C - 1)``. ``tokens`` int32 [B][C]; ``tables`` up to
    two [>= C][W] tables (wpe; RoPE cos and sin). The gathered rows then serve ``embedding``,
    ``rope_`` and the GEMM's RoPE epilogue with ``S = B*T``, where ``row % S`` is the row."""
    if _gpu(pos):
        ext().decode_prologue(pos, tokens, tok_out, int(T), int(C), list(tables), list(outs))
        return
    p = (pos.long()[:, None] + torch.arange(T)[None, :]).clamp(0, C - 1)  # [B][T]
    if tokens is not None:
        tok_out.copy_(tokens.reshape(-1, C).gather(1, p).reshape(-1))
    for t, o in zip(tables, outs):
        o.copy_(t[p.reshape(-1)])


# ---------------------------------------------------------- token sampling
# The contract (README "Generating tokens"): greedy at temperature 0; otherwise weights
# exp((l - l_max)/tau), top-k and top-p by whole value classes, and a Philox4x32-10 draw against the
# cumulative weight in index order. Both paths write stats[b] = (theta, Z, weight before the token,
# the token's weight) and apply the stream rule to ``tokens[b][pos[b] + T]``.

SAMPLE_MAX_V = 1 << 20


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11): four 32-bit counter words, two key words -> four words."""
    c0, c1, c2, c3 = (int(c) & 0xFFFFFFFF for c in counter)
    k0, k1 = (int(k) & 0xFFFFFFFF for k in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def sample_uniform(seed: int, request: int, b: int, n: int) -> float:
    """The draw of sequence ``b`` of request ``request`` at position ``n``: 24 bits in [0, 1)."""
    seed &= (1 << 64) - 1
    return (philox4x32_10((n, b, request, 0), (seed & 0xFFFFFFFF, seed >> 32))[0] >> 8) * 2.0 ** -24


def sample_slices(B: int, V: int):
    """(workgroups per row, elements per workgroup) of the GPU kernel for B rows of V logits."""
    return tuple(ext().sample_sizes(int(B), int(V))[2:])


def sample_workspace_sizes(B: int, V: int):
    """(int32 partial words, int32 tickets) of ``sample_tokens``' workspace."""
    return tuple(ext().sample_sizes(int(B), int(V))[:2])


def sample_workspace(B, V, device):
    """The workspace of ``sample_tokens``: (partials, tickets), allocated once by the caller (never
    inside a captured step); the tickets start at zero and the launch resets them. The CPU path
    needs none."""
    if torch.device(device).type != "cuda":
        return None
    pw, nc = ext().sample_sizes(int(B), int(V))[:2]
    return (torch.empty(max(pw, 4), dtype=torch.int32, device=device),
            torch.zeros(max(nc, 1), dtype=torch.int32, device=device))


def _sample_check(logits, V, T, pos, tokens, C, temperature, top_k, top_p, seed, request, prompt_len, eos, done,
                  next_out, stats):
    """The argument checks both paths of ``sample_tokens`` go through; returns B."""
    def bad(msg):
        raise ValueError("sample_tokens: " + msg)

    dev = logits.device
    B = pos.numel()
    if not (1 <= V <= SAMPLE_MAX_V and T >= 1 and C >= 1 and B >= 1):
        bad(f"needs 1 <= V <= {SAMPLE_MAX_V}, T >= 1, C >= 1 and at least one sequence (V {V}, T {T}, C {C}, B {B})")
    if logits.dtype != torch.bfloat16 or logits.dim() != 2 or logits.shape[0] != B * T or logits.shape[1] < V \
            or logits.stride(1) != 1:
        bad(f"logits must be bf16 [B*T][>= V] with contiguous rows (B {B}, T {T}, V {V}, got {tuple(logits.shape)})")
    if logits.stride(0) % 8 or logits.stride(0) < (V + 7) // 8 * 8:
        bad("the logits' row stride must be a multiple of 8 that covers V rounded up to 8")
    if not 0 <= int(request) < 1 << 31:
        bad(f"request ordinal {request}")

    def vec(t, n, dtype, name):
        if t is None:
            return
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.numel() != n or not t.is_contiguous() \
                or t.device != dev:
            bad(f"{name} must be a contiguous {dtype} tensor of {n} elements on {dev}")

    vec(pos, B, torch.int32, "pos")
    vec(tokens, B * C, torch.int32, "tokens")
    vec(temperature, B, torch.float32, "temperature")
    vec(top_k, B, torch.int32, "top_k")
    vec(top_p, B, torch.float32, "top_p")
    vec(prompt_len, B, torch.int32, "prompt_len")
    vec(done, B, torch.int32, "done")
    vec(next_out, B, torch.int32, "next_out")
    vec(stats, B * 4, torch.float32, "stats")
    if isinstance(seed, torch.Tensor):
        vec(seed, 1, torch.int64, "seed")
    elif not isinstance(seed, int):
        bad("seed must be an int or an int64 tensor of one element")
    if isinstance(eos, torch.Tensor):
        vec(eos, 1, torch.int32, "eos")
    elif not isinstance(eos, int):
        bad("eos must be an int or an int32 tensor of one element")
    return B


def _sample_row_ref(l, tau, k, p, u):
    """One row of the contract in fp64 torch: (token, (theta, Z, before, weight))."""
    V = l.numel()
    lmax = l.max()
    if not tau > 0:
        return int((l == lmax).nonzero()[0]), (float(lmax), 1.0, 0.0, 1.0)
    w = torch.exp((l - lmax) / tau)
    theta = torch.topk(l, k).values[-1] if 0 < k < V else torch.tensor(-math.inf, dtype=l.dtype)
    if p < 1:
        kept = l >= theta
        vals, inv = torch.unique(l[kept], return_inverse=True)  # ascending
        cw = torch.zeros(vals.numel(), dtype=l.dtype).index_add_(0, inv, w[kept]).flip(0).cumsum(0)
        reached = (cw >= p * cw[-1]).nonzero()
        theta = vals.flip(0)[int(reached[0]) if reached.numel() else vals.numel() - 1]
    kept = l >= theta
    wk = torch.where(kept, w, torch.zeros_like(w))
    cum = wk.cumsum(0)
    Z = cum[-1]
    hit = (kept & (cum > u * Z)).nonzero()
    tok = int(hit[0]) if hit.numel() else int(kept.nonzero()[-1])
    return tok, (float(theta), float(Z), float(cum[tok] - wk[tok]), float(wk[tok]))


def sample_tokens(logits, V, T, pos, tokens, C, temperature, top_k, top_p, seed, request=0, prompt_len=None, eos=-1,
                  done=None, next_out=None, stats=None, workspace=None):
    """Choose the token at position ``n = pos[b] + T`` of every sequence from row ``b*T + T-1`` of
    ``logits`` (bf16 [B*T][>= V], V valid columns) and feed it back: ``tokens[b][n] = next[b]``
    where ``n >= prompt_len[b]`` and ``n < C``; inside the prompt ``next[b] = tokens[b][n]`` and
    nothing is written; a finished sequence (``done[b]``) goes on with ``eos``. ``temperature``,
    ``top_k``, ``top_p`` are tensors [B]; ``seed`` (int, or int64 [1]) and ``eos`` (int, or int32
    [1]) may live on the device so that a captured launch follows them. Returns (next, stats).
    GPU: sample.hip with ``workspace`` from ``sample_workspace``. CPU: fp64 torch."""
    B = _sample_check(logits, V, T, pos, tokens, C, temperature, top_k, top_p, seed, request, prompt_len, eos, done,
                      next_out, stats)
    dev = logits.device
    if next_out is None:
        next_out = torch.empty(B, dtype=torch.int32, device=dev)
    if stats is None:
        stats = torch.empty(B, 4, dtype=torch.float32, device=dev)
    if _gpu(logits):
        if workspace is None:
            raise ValueError("sample_tokens needs the workspace of sample_workspace on the GPU")
        if not isinstance(seed, torch.Tensor):
            s64 = seed & ((1 << 64) - 1)
            seed = torch.tensor([s64 - (1 << 64) if s64 >> 63 else s64], dtype=torch.int64, device=dev)
        if not isinstance(eos, torch.Tensor):
            eos = torch.tensor([eos], dtype=torch.int32, device=dev)
        ext().sample_tokens(logits, int(V), int(T), pos, tokens, int(C), temperature, top_k, top_p, seed,
                            int(request), prompt_len, eos, done, next_out, stats, workspace[0], workspace[1])
        return next_out, stats
    seed_i = int(seed.item()) if isinstance(seed, torch.Tensor) else seed
    eos_i = int(eos.item()) if isinstance(eos, torch.Tensor) else eos
    stream = tokens.view(B, C)
    st = stats.view(B, 4)
    for b in range(B):
        n = int(pos[b]) + T
        tok, row_stats = _sample_row_ref(logits[b * T + T - 1, :V].double(), float(temperature[b]), int(top_k[b]),
                                         float(top_p[b]), sample_uniform(seed_i, int(request), b, n))
        st[b] = torch.tensor(row_stats, dtype=torch.float64).float()
        if n < (int(prompt_len[b]) if prompt_len is not None else 0):
            if 0 <= n < C:
                tok = int(stream[b, n])
        else:
            if done is not None and int(done[b]):
                tok = eos_i
            if done is not None and eos_i >= 0 and tok == eos_i:
                done[b] = 1
            if 0 <= n < C:
                stream[b, n] = tok
        next_out[b] = tok
    return next_out, stats


def gelu(x, out=None):
    if _gpu(x):
        return ext().gelu(x.contiguous(), out)
    y = F.gelu(x.float(), approximate="tanh").to(x.dtype)
    return out.copy_(y) if out is not None else y


def add(a, b, out=None):
    if _gpu(a):
        return ext().add(a.contiguous(), b.contiguous(), out)
    y = (a.float() + b.float()).to(a.dtype)
    return out.copy_(y) if out is not None else y


def swiglu(gate_up, out=None):
    if _gpu(gate_up):
        y = ext().swiglu(gate_up, out)
        return y.view(gate_up.shape[:-1] + (gate_up.shape[-1] // 2,))
    f = gate_up.shape[-1] // 2
    y = (F.silu(gate_up[..., :f].float()) * gate_up[..., f:].float()).to(gate_up.dtype)
    return out.copy_(y) if out is not None else y


def embedding(tokens, wte, wpe=None, S=1, out=None, zero=None, stats=None):
    """``wte[tokens] (+ wpe[pos % S])``; ``zero`` (GPU fp32) is cleared by the same kernel;
    ``stats`` (fp32 [rows, 2], disjoint from ``zero``) receives each output row's (sum, sum of
    squares) for the next folded norm."""
    if _gpu(wte):
        return ext().embedding(tokens.to(torch.int32).contiguous(), wte, wpe, int(S), out, zero, stats)
    if zero is not None:
        zero.zero_()
    t = tokens.reshape(-1).long()
    y = wte.float()[t]
    if wpe is not None:
        y = y + wpe.float()[torch.arange(t.numel()) % S]
    y = y.to(wte.dtype)
    if stats is not None:
        yf = y.float()
        stats.view(-1, 2).copy_(torch.stack([yf.sum(1), (yf * yf).sum(1)], 1))
    return out.copy_(y) if out is not None else y


def rope_(qkv, S, n_head, n_kv_head, head_dim, k_col, cos_t, sin_t):
    if _gpu(qkv):
        ext().rope_(qkv, S, n_head, n_kv_head, head_dim, k_col, cos_t, sin_t)
        return qkv
    return ref_rope_(qkv, S, n_head, n_kv_head, head_dim, k_col, cos_t, sin_t)


# ------------------------------------------------------------------------- MoE

def moe_router(logits, topk):
    if _gpu(logits):
        return tuple(ext().moe_router(logits.contiguous(), int(topk)))
    # the kernel's rule (moe.hip select_topk): descending logit, ties to the lower expert index —
    # a stable sort; torch.topk breaks ties arbitrarily
    val, idx = torch.sort(logits.float(), dim=-1, descending=True, stable=True)
    val, idx = val[..., :topk], idx[..., :topk]
    w = torch.softmax(val, dim=-1)
    return idx.to(torch.int32), w


def moe_align(topk_idx, n_experts):
    """Counting sort of (token, k) assignments by expert -> (src_rows, slot_of, offsets)."""
    if _gpu(topk_idx):
        return tuple(ext().moe_align(topk_idx.contiguous(), int(n_experts)))
    flat = topk_idx.reshape(-1).long()
    k = topk_idx.shape[1]
    order = torch.sort(flat, stable=True).indices
    slot_of = torch.empty_like(order)
    slot_of[order] = torch.arange(order.numel())
    counts = torch.bincount(flat, minlength=n_experts)
    offsets = torch.zeros(n_experts + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    return (order // k).to(torch.int32), slot_of.to(torch.int32), offsets.to(torch.int32)


def moe_route(logits, topk, n_experts):
    """Router + align of one MoE layer: (idx, gate, src_rows, slot_of, offsets). GPU: ONE
    workgroup launch (route_kernel) with exactly the outputs of moe_router + moe_align."""
    if _gpu(logits) and logits.shape[0] * topk <= 16384 and logits.shape[1] == n_experts:
        return tuple(ext().moe_route(logits.contiguous(), int(topk)))
    idx, gate = moe_router(logits, topk)
    return (idx, gate) + moe_align(idx, n_experts)


def moe_gate_route(x, w_gate, topk, logits):
    """Router GEMM + routing of one MoE layer: ``logits`` (bf16 [M][E]) <- x @ w_gate^T and
    returns (idx, gate, src_rows, slot_of, offsets). GPU: ONE launch (the last workgroup to
    publish its logits routes every token) when the shape fits the kernel, else the GEMM and
    moe_route."""
    if _gpu(x):
        r = ext().moe_gate_route(x, w_gate, int(topk), logits.view(x.shape[0], -1))
        if r:
            return tuple(r)
    linear(x, w_gate, out=logits.view(x.shape[0], -1))
    return moe_route(logits.view(x.shape[0], -1), topk, w_gate.shape[0])


def moe_permute(x, src_rows, out=None):
    if _gpu(x):
        return ext().moe_permute(x.contiguous(), src_rows, out)
    y = x[src_rows.long()]
    return out.copy_(y) if out is not None else y


def moe_pack(x, src_rows, offsets, dests, ovf, unpack=False):
    """Expert-parallel capacity edges (fixed-size messages; kernels.h MoePackArgs). ``dests``:
    [(buf [cap][H], cap, experts, flag, ecaps, eflags)], one per expert GPU. Pack (``unpack``
    False): buf row c <- token row ``x[src_rows[j]]`` for the c-th routed row of the listed
    experts (expert-sorted order, experts in the listed order). Unpack: ``x`` holds the
    expert-sorted rows and row j <- buf row c. Rows past ``cap`` are not moved and set
    ``ovf[flag]``; an expert whose own count exceeds ``ecaps[k]`` sets ``ovf[eflags[k]]`` (its
    compact output travels back in an edge of that many rows). No host sync on the GPU."""
    if _gpu(x):
        ext().moe_pack(x, src_rows, offsets, [d[0] for d in dests], [int(d[1]) for d in dests],
                       [list(map(int, d[2])) for d in dests], [int(d[3]) for d in dests],
                       [list(map(int, d[4])) for d in dests], [list(map(int, d[5])) for d in dests], ovf, bool(unpack))
        return
    off = [int(v) for v in offsets.tolist()]
    H = x.shape[-1]
    for buf, cap, experts, flag, ecaps, eflags in dests:
        b2 = buf.view(-1)[:int(cap) * H].view(int(cap), H)
        c = 0
        for e, ecap, ef in zip(experts, ecaps, eflags):
            lo, hi = off[e], off[e + 1]
            if ef >= 0 and hi - lo > ecap:
                ovf[ef] = 1
            for j in range(lo, hi):
                if c >= cap:
                    break
                if unpack:
                    x[j] = b2[c]
                else:
                    b2[c] = x[int(src_rows[j])]
                c += 1
        if sum(off[e + 1] - off[e] for e in experts) > cap and flag >= 0:
            ovf[flag] = 1


XBATCH_MAX_REQ, XBATCH_MAX_GROUPS = 16, 64  # kXbatchMaxReq / kXbatchMaxGroups (kernels.h)


def moe_xbatch_index(offs, reqs, experts, bases, offsets, a_rows):
    """Row map of a cross-request expert batch (one grouped launch for several requests'
    experts): group g = (request ``reqs[g]``, expert ``experts[g]``) takes rows
    [offs[q][e], offs[q][e+1]) of request q's expert-sorted block, which starts at row
    ``bases[q]`` of the batch's token matrix. Writes ``offsets`` (int32 [G+1], prefix sums of
    the groups' device-side counts) and ``a_rows`` (the token row of each sorted row) — one
    workgroup on the GPU, no host sync."""
    if _gpu(offsets):
        ext().moe_xbatch_index(list(offs), list(reqs), list(experts), list(bases), offsets, a_rows)
        return offsets, a_rows
    a_rows.zero_()
    o = 0
    offsets[0] = 0
    for g, (q, e) in enumerate(zip(reqs, experts)):
        lo, hi = int(offs[q][e]), int(offs[q][e + 1])
        a_rows[o:o + hi - lo] = torch.arange(bases[q] + lo, bases[q] + hi, dtype=a_rows.dtype)
        o += hi - lo
        offsets[g + 1] = o
    return offsets, a_rows

def moe_combine(expert_out, slot_of, weights, slot_range=None, out=None):
    """y[m] = sum_j w[m,j] * expert_out[slot_of[m,j]]; with ``slot_range`` (device int32[2])
    only slots in [r0, r1) contribute (one expert's share, zero elsewhere)."""
    if _gpu(expert_out):
        return ext().moe_combine(expert_out.contiguous(), slot_of, weights.contiguous(), slot_range, out)
    M, k = weights.shape
    sl = slot_of.long().reshape(M, k)
    keep = torch.ones_like(sl, dtype=torch.bool)
    if slot_range is not None:
        keep = (sl >= int(slot_range[0])) & (sl < int(slot_range[1]))
    g = expert_out.float()[sl.clamp(0, expert_out.shape[0] - 1).reshape(-1)].reshape(M, k, -1)
    g = torch.where(keep[..., None], g, torch.zeros_like(g))  # rows outside the range are never read
    y = (g * weights.float()[..., None]).sum(1).to(expert_out.dtype)
    return out.copy_(y) if out is not None else y


def moe_gather_combine(experts, idx, slot_of, offsets, gate, residual=None, out=None, ptrs=None, post_norm=None):
    """``out[m] = residual[m] + sum_j gate[m,j] * experts[e][slot[m,j] - offsets[e]]``, e = idx[m,j],
    over COMPACT per-expert outputs (expert e's routed rows at rows 0..count_e-1 of its
    buffer). ``ptrs``: cached int64 device tensor of the expert buffers' addresses (GPU)."""
    M, k = idx.shape
    if _gpu(out):
        if ptrs is None:
            ptrs = torch.tensor([t.data_ptr() for t in experts], dtype=torch.int64, device=out.device)
        o2 = out.view(M, -1)
        return ext().moe_gather_combine([t.reshape(-1, o2.shape[1]) for t in experts], ptrs, idx, slot_of,
                                        offsets, gate.contiguous(), None if residual is None else
                                        residual.reshape(M, -1), o2,
                                        **(_post_norm_args(post_norm) if post_norm is not None else {}))
    H = out.shape[-1]
    acc = residual.reshape(M, H).float().clone() if residual is not None else torch.zeros(M, H)
    off = offsets.long()
    for j in range(k):
        e = idx[:, j].long()
        row = slot_of.reshape(M, k)[:, j].long() - off[e]
        for ee in range(len(experts)):
            sel = (e == ee).nonzero().flatten()
            if sel.numel():
                acc[sel] += gate.reshape(M, k)[sel, j, None].float() * experts[ee].reshape(-1, H)[row[sel]].float()
    out.view(M, H).copy_(acc.to(out.dtype))
    if post_norm is not None:
        _post_norm_ref(out, post_norm)
    return out


def moe_expert(h, router_logits, w_gate_up, w_down, expert, n_experts, top_k, out=None):
    """One expert's contribution for every token (zero where it is not routed): routing
    is recomputed from the router logits, only the expert's routed rows are gathered and
    run through gate_up GEMM -> SwiGLU -> down GEMM (grouped GEMM over a device-side row
    range: no host synchronisation)."""
    idx, gate = moe_router(router_logits, top_k)
    src, slot, off = moe_align(idx, n_experts)
    xp = moe_permute(h, src)
    rng = off[expert:expert + 2].contiguous()
    gu = grouped_gemm(xp, rng, w_gate_up.unsqueeze(0))
    a = swiglu(gu)
    y = grouped_gemm(a, rng, w_down.unsqueeze(0))
    return moe_combine(y, slot, gate, rng, out)


def gemm_grouped(x, weights, offsets, act=None, out=None, outs=None, w_ptrs=None, out_ptrs=None, rows_hint=None,
                 a_rows=None, shared_weights=False):
    """Every expert of an MoE layer in ONE GEMM launch (GPU: LDS-DMA kernel, grid = experts x
    column tiles). Expert e multiplies the expert-sorted rows [offsets[e], offsets[e+1]) of
    ``x`` by ``weights[e]`` ([N][K]; SwiGLU: gate/up-interleaved, N/2 outputs) and writes them
    at the same rows of ``out``, or compactly to rows 0.. of ``outs[e]`` (at most its row
    count). ``a_rows`` (int32 [R]): ``x`` is the TOKEN matrix and sorted row r is token
    ``a_rows[r]`` (the permute happens in the kernel's loads). ``w_ptrs`` / ``out_ptrs``:
    cached int64 device tensors of the tensors' addresses (built here when omitted — pass
    cached ones inside a hipGraph). ``shared_weights``: groups repeat weights (a cross-request
    expert batch) — the launch runs each weight panel's groups together on one XCD and keeps
    the weights cached, so a panel comes from HBM once."""
    a = ACT[act] if not isinstance(act, int) else act
    E = len(weights)
    N, K = weights[0].shape
    R = x.shape[0] if a_rows is None else a_rows.numel()
    if _gpu(x):
        if w_ptrs is None:
            w_ptrs = torch.tensor([w.data_ptr() for w in weights], dtype=torch.int64, device=x.device)
        if outs is not None and out_ptrs is None:
            out_ptrs = torch.tensor([o.data_ptr() for o in outs], dtype=torch.int64, device=x.device)
        hint = rows_hint or max(1, R // E)
        # grouped variants ("g"): tuned as GROUPS experts of `hint` rows in one launch; until
        # tuned, the per-expert row-range choice ("r") stands in
        cfg, _ = tuning.lookup_fused(hint, N, K, ("s" if a == SWIGLU else "") + "g")
        if cfg < 0:
            cfg, _ = tuning.lookup_fused(hint, N, K, tuning.tag(a, True))
        if cfg >= tuning.REGSTAGE:
            cfg = -1
        ext().gemm_grouped(x, list(weights), w_ptrs, offsets, a, out, list(outs) if outs is not None else [],
                           out_ptrs, cfg, a_rows, shared_weights)
        return out if outs is None else outs
    if a_rows is not None:
        x = x[a_rows.long()]
    off = [int(v) for v in offsets.tolist()]
    for e in range(E):
        r0, r1 = off[e], off[e + 1]
        if outs is not None:
            n = min(r1 - r0, outs[e].shape[0])
            if n > 0:
                outs[e][:n] = ref_linear(x[r0:r0 + n], weights[e], act=act)
        elif r1 > r0:
            out[r0:r1] = ref_linear(x[r0:r1], weights[e], act=act)
    return out if outs is None else outs


# Token rows of a decode step up to which the executor sends the two grouped expert launches of
# an MoE layer to the skinny kernel. The kernel takes any count and a pass of it covers 16 rows, but
# the bound is what was measured at Mixtral's shapes (benchmarks/bench_moe_decode.py,
# profiles/moe_decode/): the largest M up to which the skinny kernel is the faster in every
# alternating pair against gemm_grouped for BOTH launches (gate/up ties above M = 1: both kernels
# stream the routed weights at 5.7 TB/s) and the captured decode step with it is the faster in
# every alternating round (at 2, 8 and 16 rows the step with a skinny down launch alone was slower).
MOE_SKINNY_MAX_ROWS = 1


def grouped_skinny_ok(N: int, K: int, act=None) -> bool:
    """Does the skinny grouped kernel take an [N][K] expert weight with this activation?"""
    a = ACT[act] if not isinstance(act, int) else act
    if a not in (0, SWIGLU) or N <= 0 or K <= 0 or K % 32:
        return False
    return N % 32 == 0 if a == SWIGLU else N % 16 == 0


def gemm_grouped_skinny(x, weights, offsets, act=None, out=None, outs=None, w_ptrs=None, out_ptrs=None, a_rows=None):
    """``gemm_grouped`` for the at most 16 rows per expert of a decode step (GPU: the
    weight-streaming kernel of gemm_grouped_skinny.hip, grid = experts x 16-column strips, fixed
    by (E, N) alone). Same arguments and results as ``gemm_grouped``: expert e multiplies the
    sorted rows [offsets[e], offsets[e+1]) of ``x`` (token rows ``a_rows[r]`` when given) by
    ``weights[e]`` and writes them at the same rows of ``out`` or compactly into ``outs[e]``.
    bf16, ``act`` None or "swiglu", K % 32 == 0, N % 16 == 0 (SwiGLU: N % 32 == 0); any other
    shape raises ``ValueError``. Any row counts are legal: an expert without rows reads no weight
    byte, one with more than 16 takes further passes over its weight."""
    a = ACT[act] if not isinstance(act, int) else act
    E = len(weights)
    if E == 0:
        raise ValueError("gemm_grouped_skinny: at least one expert")
    if weights[0].dim() != 2 or x.dim() != 2:
        raise ValueError("gemm_grouped_skinny: x [rows][K] and expert weights [N][K]")
    N, K = weights[0].shape
    if a not in (0, SWIGLU):
        raise ValueError(f"gemm_grouped_skinny: act must be None or 'swiglu', not {act!r}")
    if not grouped_skinny_ok(N, K, a):
        raise ValueError(f"gemm_grouped_skinny: N = {N}, K = {K} not taken: K % 32 == 0 and N % 16 == 0 "
                         "(SwiGLU: N % 32 == 0)")
    if x.shape[1] != K or any(tuple(w.shape) != (N, K) for w in weights):
        raise ValueError("gemm_grouped_skinny: every expert weight must be [N][K] with K = x.shape[1]")
    if x.dtype != torch.bfloat16 or any(w.dtype != torch.bfloat16 for w in weights):
        raise ValueError("gemm_grouped_skinny: bf16 only")
    if x.stride(1) != 1 or x.stride(0) % 8 or x.data_ptr() % 16:
        raise ValueError("gemm_grouped_skinny: rows of x must be contiguous and 16-byte aligned (row stride % 8 == 0)")
    if any(not w.is_contiguous() or w.data_ptr() % 16 for w in weights):
        raise ValueError("gemm_grouped_skinny: expert weights must be contiguous and 16-byte aligned")
    if offsets.numel() != E + 1 or offsets.dtype != torch.int32:
        raise ValueError("gemm_grouped_skinny: offsets int32 [E+1]")
    if a_rows is not None and a_rows.dtype != torch.int32:
        raise ValueError("gemm_grouped_skinny: a_rows int32")
    if (out is None) == (outs is None):
        raise ValueError("gemm_grouped_skinny: exactly one of `out` and `outs`")
    NO = N // 2 if a == SWIGLU else N
    R = x.shape[0] if a_rows is None else a_rows.numel()
    if out is not None and tuple(out.shape) != (R, NO):
        raise ValueError(f"gemm_grouped_skinny: out must be [{R}][{NO}]")
    if outs is not None and (len(outs) != E or any(o.dim() != 2 or o.shape[1] != NO for o in outs)):
        raise ValueError(f"gemm_grouped_skinny: outs must be E tensors [cap][{NO}]")
    if _gpu(x):
        if w_ptrs is None:
            w_ptrs = torch.tensor([w.data_ptr() for w in weights], dtype=torch.int64, device=x.device)
        if outs is not None and out_ptrs is None:
            out_ptrs = torch.tensor([o.data_ptr() for o in outs], dtype=torch.int64, device=x.device)
        ext().gemm_grouped_skinny(x, list(weights), w_ptrs, offsets, a, out, list(outs) if outs is not None else [],
                                  out_ptrs, a_rows)
        return out if outs is None else outs
    return gemm_grouped(x, weights, offsets, act=a, out=out, outs=outs, a_rows=a_rows)


def w8_grouped_configs() -> int:
    """Number of tile configurations of the grouped fp8-weight GEMM (``gemm_grouped_w8(config=...)``)."""
    return int(ext().gemm_w8_grouped_num_configs())


def w8_grouped_tile_rows(config: int) -> int:
    """Row-tile height of a grouped fp8-weight GEMM configuration (a group of more rows takes
    several passes of its block)."""
    return int(ext().gemm_w8_grouped_tile_rows(int(config)))


def gemm_grouped_w8(x, qweights, scales, offsets, act=None, out=None, outs=None, w_ptrs=None, s_ptrs=None,
                    out_ptrs=None, rows_hint=None, a_rows=None, shared_weights=False, config=None):
    """:func:`gemm_grouped` with fp8 expert weights: group g multiplies its rows by
    ``qweights[g]`` (``float8_e4m3fn`` [N][K], K % 16 == 0) and ``scales[g]`` (fp32 [N], any
    positive values; applied once, after the fp32 accumulation). ``act``: ``None`` or
    ``"swiglu"`` (rows of q AND scale gate/up-interleaved in blocks of ``SWIGLU_BLOCK``, N/2
    outputs). Rows, ``a_rows``, ``out`` / compact ``outs`` and ``shared_weights`` as in
    :func:`gemm_grouped`; ``s_ptrs`` is the cached int64 device tensor of the scales' addresses,
    next to ``w_ptrs`` / ``out_ptrs`` (all built here when omitted — pass cached ones inside a
    hipGraph). GPU: ONE launch of gemm_w8_grouped.hip (the fp8 bytes go global -> registers,
    are converted to bf16 there and multiplied on the bf16 MFMA; no split-K, no atomics:
    bitwise reproducible). ``config``: ``None`` picks by ``(rows_hint, N, K)``; ``c`` forces tile
    configuration c (< :func:`w8_grouped_configs`). CPU tensors run :func:`gemm_grouped`'s
    reference loop on the dequantised weights."""
    a = ACT[act] if not isinstance(act, int) else act
    for q in qweights:
        if q.dtype != torch.float8_e4m3fn:
            raise TypeError(f"gemm_grouped_w8: the weights must be float8_e4m3fn, got {q.dtype}")
    if a not in (0, SWIGLU):
        raise ValueError("gemm_grouped_w8: act is None or 'swiglu'")
    E = len(qweights)
    N, K = qweights[0].shape
    R = x.shape[0] if a_rows is None else a_rows.numel()
    if _gpu(x):
        mk = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=x.device)  # noqa: E731
        if w_ptrs is None:
            w_ptrs = mk(qweights)
        if s_ptrs is None:
            s_ptrs = mk(scales)
        if outs is not None and out_ptrs is None:
            out_ptrs = mk(outs)
        ext().gemm_grouped_w8(x, list(qweights), list(scales), w_ptrs, s_ptrs, offsets, a, out,
                              list(outs) if outs is not None else [], out_ptrs,
                              -1 if config is None else int(config), int(rows_hint or max(1, R // E)), a_rows,
                              bool(shared_weights), _stream_pol(N, K) & 6)
        return out if outs is None else outs
    if K % 16:
        raise ValueError(f"gemm_grouped_w8: K must be a multiple of 16, got {K}")
    deq = [dequantize_fp8(q, s, torch.float32) for q, s in zip(qweights, scales)]
    return gemm_grouped(x, deq, offsets, act=act, out=out, outs=outs, a_rows=a_rows)


def w4a8_grouped_configs() -> int:
    """Number of tile configurations of the grouped MXFP4 x fp8 GEMM (``gemm_grouped_w4a8(config=...)``)."""
    return int(ext().gemm_w4a8_grouped_num_configs())


def w4a8_grouped_tile_rows(config: int) -> int:
    """Row-tile height of a grouped MXFP4 x fp8 GEMM configuration (a group of more rows takes
    several passes of its block)."""
    return int(ext().gemm_w4a8_grouped_tile_rows(int(config)))


def gemm_grouped_w4a8(xq, xscale, qweights, bscales, offsets, act=None, out=None, outs=None, w_ptrs=None,
                      s_ptrs=None, out_ptrs=None, rows_hint=None, a_rows=None, shared_weights=False, config=None):
    """:func:`gemm_grouped` with MXFP4 expert weights and fp8 activation rows: group g computes
    ``act(xscale[row(r)] * sum_k xq[row(r)][k] * W_g[n][k])`` over its sorted rows r, with
    ``row(r) = a_rows[r]`` when ``a_rows`` is given, else r. ``xq`` is e4m3 [rows, K] with one
    fp32 scale per row of ``xq`` (:func:`quantize_rows_fp8`) — with ``a_rows`` the scale is
    gathered with its row. ``W_g[n][k] = e2m1(qweights[g][n][k]) * 2^(bscales[g][n][k/32] - 127)``
    in the layout of :func:`quantize_mxfp4` (``q`` uint8 [N, K/2], ``s`` uint8 [N, K/32], any code
    0..254), K % 32 == 0, fp32 accumulation, bf16 output, no bias. ``act``: ``None`` or
    ``"swiglu"`` (rows of q AND s gate/up-interleaved in blocks of ``SWIGLU_BLOCK``, N/2 outputs).
    Rows, ``out`` / compact ``outs``, ``shared_weights`` and the cached pointer arrays as in
    :func:`gemm_grouped_w8`. GPU: ONE launch of gemm_w4a8_grouped.hip (the MXFP4 bytes go global ->
    registers -> the block-scaled MFMA, which applies the e8m0 scales; no split-K, no atomics:
    bitwise reproducible). ``config``: ``None`` picks by ``(rows_hint, N, K)``; ``c`` forces tile
    configuration c (< :func:`w4a8_grouped_configs`). CPU tensors run :func:`gemm_grouped`'s
    reference loop on the two dequantised operands."""
    a = ACT[act] if not isinstance(act, int) else act
    if xq.dtype != torch.float8_e4m3fn:
        raise TypeError(f"gemm_grouped_w4a8: the activations must be float8_e4m3fn, got {xq.dtype}")
    for q, s in zip(qweights, bscales):
        if q.dtype != torch.uint8 or s.dtype != torch.uint8:
            raise TypeError("gemm_grouped_w4a8: the MXFP4 weights and their block scales must be uint8, got "
                            f"{q.dtype} and {s.dtype}")
    if a not in (0, SWIGLU):
        raise ValueError("gemm_grouped_w4a8: act is None or 'swiglu'")
    E = len(qweights)
    if E == 0 or len(bscales) != E:
        raise ValueError("gemm_grouped_w4a8: one block-scale tensor per expert weight")
    if xq.dim() != 2:
        raise ValueError(f"gemm_grouped_w4a8: xq must be [rows, K], got {tuple(xq.shape)}")
    K = xq.shape[1]
    if K % 32 or K < 32:
        raise ValueError(f"gemm_grouped_w4a8: K must be a multiple of 32, got {K}")
    N = qweights[0].shape[0]
    for q, s in zip(qweights, bscales):
        if tuple(q.shape) != (N, K // 2) or tuple(s.shape) != (N, K // 32):
            raise ValueError(f"gemm_grouped_w4a8: expected q [{N}, {K // 2}] and s [{N}, {K // 32}], got "
                             f"{tuple(q.shape)} and {tuple(s.shape)}")
    if xscale.dtype != torch.float32 or xscale.numel() != xq.shape[0]:
        raise ValueError(f"gemm_grouped_w4a8: xscale must be fp32 with one entry per row of xq ({xq.shape[0]}), got "
                         f"{xscale.dtype} x {xscale.numel()}")
    R = xq.shape[0] if a_rows is None else a_rows.numel()
    if _gpu(xq):
        if config is not None and not 0 <= int(config) < w4a8_grouped_configs():
            raise ValueError(f"gemm_grouped_w4a8: config must be below {w4a8_grouped_configs()}, got {config}")
        for q in qweights:
            if q.data_ptr() % 16:
                raise ValueError("gemm_grouped_w4a8: the weights must be 16-byte aligned")
        mk = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=xq.device)  # noqa: E731
        if w_ptrs is None:
            w_ptrs = mk(qweights)
        if s_ptrs is None:
            s_ptrs = mk(bscales)
        if outs is not None and out_ptrs is None:
            out_ptrs = mk(outs)
        ext().gemm_grouped_w4a8(xq, xscale, list(qweights), list(bscales), w_ptrs, s_ptrs, offsets, a, out,
                                list(outs) if outs is not None else [], out_ptrs,
                                -1 if config is None else int(config), int(rows_hint or max(1, R // E)), a_rows,
                                bool(shared_weights), _stream_pol(N, K) & 6)
        return out if outs is None else outs
    xd = dequantize_fp8(xq, xscale, torch.float32)
    deq = [dequantize_mxfp4(q, s, torch.float32) for q, s in zip(qweights, bscales)]
    return gemm_grouped(xd, deq, offsets, act=act, out=out, outs=outs, a_rows=a_rows)


def grouped_gemm(X, offsets, W, act=None):
    """Per-expert ``act(X_e @ W_e^T)`` over expert-sorted rows; W is [E][N][K]."""
    a = ACT[act] if not isinstance(act, int) else act
    if _gpu(X):
        return ext().grouped_gemm(X.contiguous(), offsets, W.contiguous(), a)
    out = torch.zeros(X.shape[0], W.shape[1], dtype=X.dtype)
    off = offsets.tolist()
    for e in range(W.shape[0]):
        if off[e + 1] > off[e]:
            out[off[e]:off[e + 1]] = ref_linear(X[off[e]:off[e + 1]], W[e], act=a)
    return out
