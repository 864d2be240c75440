"""Parameter groups: scheduler parameter ids -> the real tensors behind them.

The scheduler reasons about opaque parameter ids (``"layer_3_attn_qkv_weights"``); the
executor needs bytes. A :class:`ParamGroup` lists the tensors one id stands for, in the
layout the HIP kernels consume:

* every GEMM weight is stored **[N][K] (K contiguous)**, bf16, so both MFMA operands of
  ``y = x @ W^T`` stream K-contiguous rows (GPT-2's Conv1D stores [K][N]; the checkpoint
  converter transposes once at load time, never per call);
* norms/biases are bf16 vectors (the kernels accumulate in fp32).

Initialisation is deterministic per tensor name (random-init weights of the named
architecture; there are no checkpoints offline).
"""
from __future__ import annotations

import hashlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch


@dataclass
class TensorSpec:
    name: str
    shape: Tuple[int, ...]
    init: str = "normal"  # normal | ln | bias | ones | zeros
    std: float = 0.02
    parent: Optional["TensorSpec"] = None  # shard of a larger tensor (tensor parallelism)
    slc: Optional[tuple] = None            # (dim, start, stop) or ("rows", ((a, b), ...))
    # fp8 weight storage (registry.build weight_dtype="fp8"): a GEMM weight [N, K] kept as e4m3
    # bytes [N][K] followed (256-B aligned) by one fp32 scale per output channel [N]
    quant: bool = False
    # storage format of a quantised tensor: "fp8" (above) or "mxfp4" (weight_dtype="mxfp4"): OCP
    # MXFP4, N*K/2 bytes of e2m1 pairs followed (256-B aligned) by N*K/32 e8m0 block-scale bytes
    qfmt: str = "fp8"

    @property
    def numel(self) -> int:
        n = 1
        for s in self.shape:
            n *= s
        return n


@dataclass
class ParamGroup:
    pid: str
    tensors: List[TensorSpec] = field(default_factory=list)

    def nbytes(self, dtype_bytes: int = 2) -> int:
        return sum(sum(quant_parts(t)[::2]) if t.quant else t.numel * dtype_bytes for t in self.tensors)


def quant_parts(spec: TensorSpec) -> Tuple[int, int, int]:
    """A quantised tensor inside its group: (bytes of the data part, byte offset of the scales
    from the tensor's start, bytes of the scales). fp8: N*K e4m3 bytes and N fp32 scales; mxfp4:
    N*K/2 bytes of e2m1 pairs and N*K/32 e8m0 bytes."""
    if spec.qfmt == "mxfp4":
        qb = spec.numel // 2
        return qb, _align(qb), spec.numel // MX_BLOCK
    qb = spec.numel
    return qb, _align(qb), 4 * spec.shape[0]


def quantize_fp8(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-output-channel e4m3 quantisation with POWER-OF-TWO scales: row n of ``w`` [N, K]
    becomes ``q[n] = rne(w[n] / scale[n])`` with ``scale[n]`` the smallest 2^e such that
    ``amax_n / 2^e <= 448`` (an all-zero row: 1). Every e4m3 value times a power of two is a
    bf16 value, so :func:`dequantize_fp8` of the result is exactly a bf16 tensor. Runs on
    ``w``'s device. Returns ``(q float8_e4m3fn [N, K], scale fp32 [N])``."""
    w2 = w.detach().reshape(w.shape[0], -1)
    N, K = w2.shape
    q = torch.empty((N, K), dtype=torch.float8_e4m3fn, device=w.device)
    scale = torch.empty(N, dtype=torch.float32, device=w.device)
    step = max(1, (1 << 26) // max(K, 1))  # rows per pass: the fp32 temporaries stay small
    for r in range(0, N, step):
        wf = w2[r:r + step].float()
        amax = wf.abs().amax(dim=1)
        m, ex = torch.frexp(amax)  # amax = m * 2^ex, m in [0.5, 1); 448 = 0.875 * 2^9
        e = torch.where(m <= 0.875, ex - 9, ex - 8)
        s = torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), e), torch.ones_like(amax))
        scale[r:r + step] = s
        q[r:r + step] = (wf / s[:, None]).clamp_(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.reshape(w.shape), scale


def dequantize_fp8(q: torch.Tensor, scale: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """``q[n][k] * scale[n]`` (exact in bf16 for power-of-two scales)."""
    return (q.float() * scale.float().reshape(-1, *([1] * (q.dim() - 1)))).to(dtype)


MX_BLOCK = 32  # elements per e8m0 block scale (OCP MX)
_E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def quantize_mxfp4(w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """OCP MXFP4 quantisation of ``w`` [N, K] (K % 32 == 0): every 32 consecutive elements of a
    row share one e8m0 scale ``2^e``, the smallest with ``amax_block / 2^e <= 6`` (e clamped to
    [-127, 127]; an all-zero block: 2^0), and become e2m1 codes (bit 3 the sign, codes 0..7 =
    0, 0.5, 1, 1.5, 2, 3, 4, 6) of ``w / 2^e`` rounded to nearest, ties to even, saturating at
    +-6. Every e2m1 value times a power of two is a bf16 value, so :func:`dequantize_mxfp4` of
    the result is exactly a bf16 tensor. Runs on ``w``'s device. Returns ``(q uint8 [N, K/2],
    s uint8 [N, K/32])``: element k of a row is the low (k even) / high (k odd) nibble of byte
    k/2, and scale code c means 2^(c - 127) (255 is never written)."""
    w2 = w.detach().reshape(w.shape[0], -1)
    N, K = w2.shape
    if K % MX_BLOCK:
        raise ValueError(f"quantize_mxfp4: K must be a multiple of {MX_BLOCK}, got {K}")
    q = torch.empty((N, K // 2), dtype=torch.uint8, device=w.device)
    s = torch.empty((N, K // MX_BLOCK), dtype=torch.uint8, device=w.device)
    step = max(1, (1 << 26) // max(K, 1))  # rows per pass: the fp32 temporaries stay small
    for r in range(0, N, step):
        wf = w2[r:r + step].float().reshape(-1, K // MX_BLOCK, MX_BLOCK)
        amax = wf.abs().amax(dim=2)
        m, ex = torch.frexp(amax)  # amax = m * 2^ex, m in [0.5, 1); 6 = 0.75 * 2^3
        e = torch.where(m <= 0.75, ex - 3, ex - 2).clamp_(-127, 127)
        e = torch.where(amax > 0, e, torch.zeros_like(e))
        s[r:r + step] = (e + 127).to(torch.uint8)
        x = torch.ldexp(wf, -e[:, :, None])
        a = x.abs().clamp_(max=6.0)
        # round half to even on the grid: steps of 0.5 below 2, of 1 below 4, of 2 above
        v = torch.where(a < 2, torch.round(a * 2) / 2, torch.where(a < 4, torch.round(a), torch.round(a / 2) * 2))
        code = torch.where(v < 2, v * 2, torch.where(v < 4, v + 2, v / 2 + 4)).to(torch.uint8)
        code = (code | (torch.signbit(x).to(torch.uint8) << 3)).reshape(-1, K)
        q[r:r + step] = code[:, 0::2] | (code[:, 1::2] << 4)
    return q, s


def dequantize_mxfp4(q: torch.Tensor, s: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """``e2m1(q[n][k]) * 2^(s[n][k/32] - 127)`` as ``dtype`` [N, K] (exact in bf16)."""
    N, K = q.shape[0], q.shape[1] * 2
    lut = torch.tensor(_E2M1 + tuple(-v for v in _E2M1), dtype=torch.float32, device=q.device)
    out = torch.empty((N, K), dtype=dtype, device=q.device)
    step = max(1, (1 << 26) // max(K, 1))
    for r in range(0, N, step):
        qq = q[r:r + step]
        codes = torch.stack((qq & 15, qq >> 4), dim=2).reshape(-1, K // MX_BLOCK, MX_BLOCK)
        e = s[r:r + step].to(torch.int32) - 127
        out[r:r + step] = torch.ldexp(lut[codes.long()], e[:, :, None]).reshape(-1, K).to(dtype)
    return out


def _seed(name: str, base: int) -> int:
    return (int(hashlib.sha1(name.encode()).hexdigest()[:12], 16) + base) % (2 ** 62)


def _take(full: torch.Tensor, slc) -> torch.Tensor:
    if slc[0] == "rows":
        return torch.cat([full[a:b] for a, b in slc[1]], 0).contiguous()
    dim, a, b = slc
    return full.narrow(dim, a, b - a).contiguous()


def materialize(spec: TensorSpec, dtype=torch.bfloat16, device="cpu", seed: int = 0) -> torch.Tensor:
    """Deterministic random-init tensor for ``spec`` (fp32 generation, cast once). A shard
    is the matching slice of its parent, so sharded and unsharded models are identical."""
    if spec.parent is not None:
        return _take(materialize(spec.parent, dtype, device, seed), spec.slc)
    if spec.init == "ones":
        return torch.ones(spec.shape, dtype=dtype, device=device)
    if spec.init == "zeros":
        return torch.zeros(spec.shape, dtype=dtype, device=device)
    g = torch.Generator().manual_seed(_seed(spec.name, seed))
    if spec.init == "ln":  # non-trivial LayerNorm/RMSNorm gains so tests exercise them
        t = 1.0 + 0.1 * torch.randn(spec.shape, generator=g)
    elif spec.init == "bias":
        t = 0.02 * torch.randn(spec.shape, generator=g)
    else:
        t = spec.std * torch.randn(spec.shape, generator=g)
    return t.to(dtype=dtype, device=device)


def fill_on_device(spec: TensorSpec, out: torch.Tensor, seed: int = 0) -> None:
    """Random-init ``out`` (already in HBM) for ``spec`` with the device RNG: no host
    master copy, no PCIe traffic — how the large-model benchmarks (Llama-3-8B 16 GB,
    Mixtral-8x7B 93 GB) get their weights. Deterministic per name, but a different
    stream from :func:`materialize` (so not comparable to the CPU reference)."""
    if spec.parent is not None:
        full = torch.empty(spec.parent.shape, dtype=out.dtype, device=out.device)
        fill_on_device(spec.parent, full, seed)
        out.copy_(_take(full, spec.slc))
        return
    if spec.init == "ones":
        out.fill_(1.0)
        return
    if spec.init == "zeros":
        out.zero_()
        return
    g = torch.Generator(device=out.device).manual_seed(_seed(spec.name, seed))
    if spec.init == "ln":
        out.normal_(1.0, 0.1, generator=g)
    elif spec.init == "bias":
        out.normal_(0.0, 0.02, generator=g)
    else:
        out.normal_(0.0, spec.std, generator=g)


class ParamStore:
    """Host-side master copy of every parameter group (pinned when a GPU is present),
    materialised lazily; the executor copies groups into its HBM arena on demand.
    ``device_init=True`` skips the host copy: groups are random-initialised directly in
    the arena (benchmarks of models whose host materialisation would dominate setup)."""

    def __init__(self, groups: Dict[str, ParamGroup], dtype=torch.bfloat16, seed: int = 0, pin: bool = None,
                 device_init: bool = False):
        self.groups = groups
        self.dtype = dtype
        self.seed = seed
        self.device_init = device_init
        self.pin = (torch.cuda.is_available() and not device_init) if pin is None else pin
        self._host: Dict[str, torch.Tensor] = {}
        self._images: Dict[str, torch.Tensor] = {}
        self._quant: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}  # quantised name -> (q, scale)
        self._specs: Dict[str, TensorSpec] = {}
        for g in groups.values():
            for sp in g.tensors:
                while sp is not None:  # shards and the full tensors they slice
                    self._specs.setdefault(sp.name, sp)
                    sp = sp.parent

    def tensor(self, name: str) -> torch.Tensor:
        """The tensor as the model computes with it: for a quantised name, the DEQUANTISED
        weight (exactly a bf16 tensor: power-of-two scales)."""
        t = self._host.get(name)
        if t is None:
            spec = self._spec(name)
            if spec.parent is not None:
                t = _take(self.tensor(spec.parent.name), spec.slc)
            else:
                t = materialize(spec, self.dtype, "cpu", self.seed)
            if spec.quant:
                t = self._quantize(name, t)
            if self.pin:
                t = t.pin_memory()
            self._host[name] = t
        return t

    def _quantize(self, name: str, t: torch.Tensor) -> torch.Tensor:
        mx = self._spec(name).qfmt == "mxfp4"
        q, scale = quantize_mxfp4(t) if mx else quantize_fp8(t)
        self._quant[name] = (q.pin_memory(), scale.pin_memory()) if self.pin else (q, scale)
        return (dequantize_mxfp4(q, scale, self.dtype).reshape(t.shape) if mx
                else dequantize_fp8(q, scale, self.dtype))

    def quantized(self, name: str) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(q e4m3 [N, K], scale fp32 [N])`` of an fp8 tensor, ``(q uint8 [N, K/2], s uint8
        [N, K/32])`` of an mxfp4 one (``tensor(name)`` is the dequantised product)."""
        if not self._spec(name).quant:
            raise KeyError(f"{name} is not stored quantised")
        if name not in self._quant:
            self.tensor(name)
        return self._quant[name]

    def is_quantized(self, name: str) -> bool:
        sp = self._specs.get(name)
        return sp is not None and sp.quant

    def quant_format(self, name: str) -> Optional[str]:
        """``"fp8"`` / ``"mxfp4"`` for a quantised tensor, ``None`` for a bf16 one."""
        sp = self._specs.get(name)
        return sp.qfmt if sp is not None and sp.quant else None

    def _spec(self, name: str) -> TensorSpec:
        return self._specs[name]

    def fill(self, name: str, out: torch.Tensor, scale_out: Optional[torch.Tensor] = None) -> None:
        """Write tensor ``name`` into ``out`` (an HBM arena view); a quantised tensor's data
        part into ``out`` and its scales into ``scale_out``."""
        spec = self._spec(name)
        if spec.quant:
            if self.device_init and out.is_cuda and name not in self._host:
                # bf16 scratch in HBM, quantised there: still no host copy
                full = torch.empty(spec.shape, dtype=self.dtype, device=out.device)
                fill_on_device(spec, full, self.seed)
                q, scale = quantize_mxfp4(full) if spec.qfmt == "mxfp4" else quantize_fp8(full)
                out.copy_(q)
                scale_out.copy_(scale)
            else:
                q, scale = self.quantized(name)
                out.copy_(q, non_blocking=True)
                scale_out.copy_(scale, non_blocking=True)
        elif self.device_init and out.is_cuda and name not in self._host:
            fill_on_device(spec, out, self.seed)
        else:
            out.copy_(self.tensor(name), non_blocking=True)

    def group_image(self, pid: str) -> Optional[torch.Tensor]:
        """The group as ONE host byte image in its arena layout (pinned), so a refill is a
        single DMA of the whole group instead of a copy per tensor; ``None`` for
        device-initialised stores (nothing on the host to copy)."""
        if self.device_init:
            return None
        img = self._images.get(pid)
        if img is None:
            total, layout = group_layout(self.groups[pid], torch.tensor([], dtype=self.dtype).element_size())
            img = torch.zeros(total, dtype=torch.uint8)
            for spec, off in layout:
                if spec.quant:
                    q, scale = self.quantized(spec.name)
                    qb, s_off, sb = quant_parts(spec)
                    img[off:off + qb].copy_(q.contiguous().view(-1).view(torch.uint8))
                    img[off + s_off:off + s_off + sb].copy_(scale.contiguous().view(-1).view(torch.uint8))
                    continue
                t = self.tensor(spec.name).contiguous()
                img[off:off + t.numel() * t.element_size()].copy_(t.view(-1).view(torch.uint8))
            if self.pin:
                img = img.pin_memory()
            self._images[pid] = img
        return img

    def group_tensors(self, pid: str) -> List[Tuple[TensorSpec, torch.Tensor]]:
        return [(s, self.tensor(s.name)) for s in self.groups[pid].tensors]

    def nbytes(self, pid: str) -> int:
        """Bytes the group occupies in the HBM parameter arena (256-B aligned tensors)."""
        return group_layout(self.groups[pid], torch.tensor([], dtype=self.dtype).element_size())[0]

    def set_tensor(self, name: str, value: torch.Tensor) -> None:
        """Install real weights (e.g. converted from a checkpoint) for ``name``."""
        spec = self._spec(name)
        if tuple(value.shape) != tuple(spec.shape):
            raise ValueError(f"{name}: expected shape {spec.shape}, got {tuple(value.shape)}")
        t = value.detach().to("cpu", self.dtype).contiguous()
        if spec.quant:  # stored quantised: what tensor() returns is what the kernels multiply
            t = self._quantize(name, t)
        self._host[name] = t.pin_memory() if self.pin else t
        self._images = {k: v for k, v in self._images.items()
                        if all(sp.name != name for sp in self.groups[k].tensors)}


GROUP_ALIGN = 256


def _align(n: int) -> int:
    return (n + GROUP_ALIGN - 1) // GROUP_ALIGN * GROUP_ALIGN


def group_layout(group: ParamGroup, dtype_bytes: int = 2):
    """Byte layout of a parameter group inside the HBM parameter arena: every tensor
    starts 256-B aligned (16-B vector loads, cache-line aligned rows). A quantised tensor
    (``spec.quant``) takes its data bytes and, 256-B aligned behind them, its scale bytes
    (:func:`quant_parts`: fp8 N*K and 4*N, mxfp4 N*K/2 and N*K/32).
    Returns ``(total_bytes, [(spec, byte_offset), ...])``."""
    off, out = 0, []
    for spec in group.tensors:
        out.append((spec, off))
        if spec.quant:
            qb, s_off, sb = quant_parts(spec)
            off += s_off + _align(sb)
        else:
            off += _align(spec.numel * dtype_bytes)
    return off, out
