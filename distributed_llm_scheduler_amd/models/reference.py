"""Plain PyTorch fp32 reference forwards over a :class:`ParamStore`.

These define what the DAG executor must produce (same weights, same tokens) and are
independent of the DAG machinery: a straight-line forward pass written from the model
definitions (GPT-2: pre-LN blocks, tanh-GELU MLP, tied LM head; Llama: RMSNorm, RoPE,
GQA, SwiGLU; Mixtral: top-k routed SwiGLU experts).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from .config import ModelConfig
from .params import ParamStore, dequantize_fp8, quantize_fp8


def _w(store: ParamStore, name: str) -> torch.Tensor:
    return store.tensor(name).float()


def _mm(store: ParamStore, x: torch.Tensor, name: str, a8: bool = False) -> torch.Tensor:
    """``x @ W^T``; with fp8 activations (``a8``) and a weight the store holds quantised, the
    input rows go through the per-row e4m3 quantise-dequantise first (quantize_fp8 of the rows:
    one power-of-two scale per row)."""
    if a8 and store.is_quantized(name):
        q, s = quantize_fp8(x.reshape(-1, x.shape[-1]))
        x = dequantize_fp8(q, s, torch.float32).reshape(x.shape)
    return x @ _w(store, name).t()


def _a8(act_dtype: str) -> bool:
    if act_dtype not in ("bf16", "fp8"):
        raise ValueError(f"act_dtype must be 'bf16' or 'fp8', got {act_dtype!r}")
    return act_dtype == "fp8"


def _kv8(kv_dtype: str) -> bool:
    if kv_dtype not in ("bf16", "fp8"):
        raise ValueError(f"kv_dtype must be 'bf16' or 'fp8', got {kv_dtype!r}")
    return kv_dtype == "fp8"


def _qdq_heads(x: torch.Tensor, D: int) -> torch.Tensor:
    """K or V rows [B, S, n_kv_head*D] through the e4m3 quantise-dequantise of an fp8 KV cache:
    one power-of-two scale per (position, KV head)."""
    q, s = quantize_fp8(x.reshape(-1, D))
    return dequantize_fp8(q, s, torch.float32).reshape(x.shape)


def _attn(q, k, v, nh, nkv, D, causal=True):
    B, S = q.shape[0], q.shape[1]
    q = q.view(B, S, nh, D).transpose(1, 2)
    k = k.view(B, S, nkv, D).transpose(1, 2)
    v = v.view(B, S, nkv, D).transpose(1, 2)
    if nh != nkv:
        k = k.repeat_interleave(nh // nkv, 1)
        v = v.repeat_interleave(nh // nkv, 1)
    s = q @ k.transpose(-1, -2) / math.sqrt(D)
    if causal:
        s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, S, nh * D)


@torch.no_grad()
def gpt2_forward(cfg: ModelConfig, store: ParamStore, tokens: torch.Tensor, hidden: list = None,
                 act_dtype: str = "bf16", kv_dtype: str = "bf16") -> torch.Tensor:
    """tokens [B, S] -> logits [B, S, V] (fp32). ``hidden`` (if a list) receives the residual
    stream after every block. ``act_dtype``, ``kv_dtype``: see :func:`forward`."""
    a8, kv8 = _a8(act_dtype), _kv8(kv_dtype)
    B, S = tokens.shape
    H, nh = cfg.n_embd, cfg.n_head
    x = _w(store, "wte")[tokens.long()] + _w(store, "wpe")[:S][None]
    for i in range(cfg.n_layer):
        p = f"h.{i}."
        h = F.layer_norm(x, (H,), _w(store, p + "ln_1.weight"), _w(store, p + "ln_1.bias"), cfg.norm_eps)
        qkv = _mm(store, h, p + "attn.c_attn.weight", a8) + _w(store, p + "attn.c_attn.bias")
        k, v = qkv[..., H:2 * H], qkv[..., 2 * H:]
        if kv8:
            k, v = _qdq_heads(k, cfg.head_dim), _qdq_heads(v, cfg.head_dim)
        a = _attn(qkv[..., :H], k, v, nh, nh, cfg.head_dim)
        x = x + _mm(store, a, p + "attn.c_proj.weight", a8) + _w(store, p + "attn.c_proj.bias")
        h = F.layer_norm(x, (H,), _w(store, p + "ln_2.weight"), _w(store, p + "ln_2.bias"), cfg.norm_eps)
        h = F.gelu(_mm(store, h, p + "mlp.c_fc.weight", a8) + _w(store, p + "mlp.c_fc.bias"), approximate="tanh")
        x = x + _mm(store, h, p + "mlp.c_proj.weight", a8) + _w(store, p + "mlp.c_proj.bias")
        if hidden is not None:
            hidden.append(x.clone())
    x = F.layer_norm(x, (H,), _w(store, "ln_f.weight"), _w(store, "ln_f.bias"), cfg.norm_eps)
    return _mm(store, x, "wte", a8)


def _rope(x, S, D, theta):
    inv = 1.0 / (theta ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    ang = torch.arange(S, dtype=torch.float64)[:, None] * inv[None]
    c, s = ang.cos().float(), ang.sin().float()
    B = x.shape[0]
    x = x.view(B, S, -1, D)
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    c, s = c[None, :, None, :], s[None, :, None, :]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).view(B, S, -1)


def _rms(x, w, eps):
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w


@torch.no_grad()
def llama_forward(cfg: ModelConfig, store: ParamStore, tokens: torch.Tensor, router_margins: list = None,
                  act_dtype: str = "bf16", kv_dtype: str = "bf16") -> torch.Tensor:
    """Llama-3 / Mixtral forward (fp32): tokens [B, S] -> logits [B, S, V]. ``router_margins``
    (if a list) receives, per MoE layer, the [B, S] gap between the k-th and (k+1)-th router
    logit: tokens with a tiny gap may legitimately route differently under bf16 logits.
    ``act_dtype``, ``kv_dtype``: see :func:`forward`."""
    a8, kv8 = _a8(act_dtype), _kv8(kv_dtype)
    B, S = tokens.shape
    nh, nkv, D = cfg.n_head, cfg.kv_heads, cfg.head_dim
    x = _w(store, "tok_embeddings")[tokens.long()]
    for i in range(cfg.n_layer):
        p = f"layers.{i}."
        h = _rms(x, _w(store, p + "attention_norm.weight"), cfg.norm_eps)
        qkv = _mm(store, h, p + "attention.wqkv", a8)
        q, k, v = qkv[..., :nh * D], qkv[..., nh * D:(nh + nkv) * D], qkv[..., (nh + nkv) * D:]
        q, k = _rope(q, S, D, cfg.rope_theta), _rope(k, S, D, cfg.rope_theta)
        if kv8:
            k, v = _qdq_heads(k, D), _qdq_heads(v, D)
        x = x + _mm(store, _attn(q, k, v, nh, nkv, D), p + "attention.wo", a8)
        h = _rms(x, _w(store, p + "ffn_norm.weight"), cfg.norm_eps)
        if cfg.n_experts:
            logits = _mm(store, h, p + "moe.gate", a8)
            val, idx = torch.topk(logits, cfg.top_k, -1)
            if router_margins is not None:
                srt = torch.sort(logits, -1, descending=True).values
                router_margins.append(srt[..., cfg.top_k - 1] - srt[..., cfg.top_k])
            gate = torch.softmax(val, -1)
            out = torch.zeros_like(h)
            for e in range(cfg.n_experts):
                gu = _mm(store, h, p + f"moe.experts.{e}.w13", a8)
                y = F.silu(gu[..., :cfg.ffn]) * gu[..., cfg.ffn:]
                y = _mm(store, y, p + f"moe.experts.{e}.w2", a8)
                wgt = (gate * (idx == e)).sum(-1, keepdim=True)
                out = out + wgt * y
            x = x + out
        else:
            gu = _mm(store, h, p + "feed_forward.w13", a8)
            x = x + _mm(store, (F.silu(gu[..., :cfg.ffn]) * gu[..., cfg.ffn:]), p + "feed_forward.w2", a8)
    x = _rms(x, _w(store, "norm.weight"), cfg.norm_eps)
    return _mm(store, x, "output.weight", a8)


def forward(cfg: ModelConfig, store: ParamStore, tokens: torch.Tensor, router_margins: list = None,
            act_dtype: str = "bf16", kv_dtype: str = "bf16") -> torch.Tensor:
    """``act_dtype="fp8"``: the input of every GEMM whose weight the store holds quantised is
    quantise-dequantised per row (``quantize_fp8`` / ``dequantize_fp8``: e4m3, one power-of-two
    scale per row) — what the executor's fp8-activation mode multiplies, over fp8 and mxfp4
    weights alike (``store.tensor`` is the dequantised weight in either format). ``kv_dtype="fp8"``:
    K (after RoPE) and V are quantise-dequantised per (position, KV head) before attention — what
    an fp8 KV cache holds. The defaults change nothing."""
    if cfg.family == "gpt2":
        return gpt2_forward(cfg, store, tokens, act_dtype=act_dtype, kv_dtype=kv_dtype)
    return llama_forward(cfg, store, tokens, router_margins, act_dtype=act_dtype, kv_dtype=kv_dtype)
