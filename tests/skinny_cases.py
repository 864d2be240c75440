"""Cases, runner, a torch model of the kernel and mutants of it for the dense skinny GEMM
(``ops.linear_skinny``, csrc/kernels/gemm_skinny.hip), shared by test_skinny_cpu.py and
test_skinny_gpu.py. Inputs, float64 references and checks are those of gemm_cases.py /
gemm_checks.py: NaN-padded strided operands, canaries around the output, the per-element bound
with the families' ``C_BOUND`` and ``torch.equal`` on the exact probes.

Shapes (N, K), each with M in {1, 2, 5, 16} and every W in {4, 8, 16}:
  (16, 32)      half a slice
  (48, 96)      fewer slices than waves (empty waves), K % 64 != 0
  (50, 64)      ragged last strip, odd ldc (scalar stores)
  (272, 1056)   slices do not divide by W, more than one ring trip, a partial last slice
  (1041, 256)   ragged, LM-head-like
  (64, 4160)    long run, K % 64 == 0 with a remainder over the waves
  (64, 14336)
"""
import functools
import math
from collections import namedtuple

import torch

import gemm_cases as gc
import gemm_checks as gk
from distributed_llm_scheduler_amd import ops

BF = torch.bfloat16
NAN = float("nan")
MS = (1, 2, 5, 16)
WAVES = (4, 8, 16)
PLAIN = ((16, 32), (48, 96), (50, 64), (272, 1056), (1041, 256), (64, 4160), (64, 14336))
SWIGLU = ((32, 32), (96, 160), (512, 256), (96, 4160))
ROPE = dict(N=512, D=64, cols=384, K=256, S=(1, 4))
FOLDED_K = (96, 256, 1056)
FOLDED = (("layernorm", "gelu", 80), ("rmsnorm", "swiglu", 96))  # (mode, act, N)

# name -> (family, bias, act, residual, alpha)
Epi = namedtuple("Epi", "name family bias act res alpha")
EPIS = (Epi("none", "linear", False, None, False, 1.0), Epi("bias", "linear", True, None, False, 1.0),
        Epi("bias_relu_res", "linear", True, "relu", True, 1.0), Epi("bias_gelu_res", "gelu", True, "gelu", True, 1.0),
        Epi("bias_silu_res", "silu", True, "silu", True, 1.0), Epi("alpha_half", "linear", False, None, False, 0.5))
SWIGLU_EPIS = (Epi("none", "swiglu", False, "swiglu", False, 1.0), Epi("bias_res", "swiglu", True, "swiglu", True, 1.0),
               Epi("alpha_half", "swiglu", False, "swiglu", False, 0.5))

# Largest err / derived bound per family over the bounded cases on an MI355X (the tests print every
# figure); the bounds held are gemm_checks.C_BOUND, unchanged.
MEASURED = {
    "linear": 1.909,     # bias + relu + residual: two roundings
    "gelu": 1.852,       # bias + gelu + residual
    "silu": 1.905,       # bias + silu + residual (gemm_checks' 0.93 is silu WITHOUT a residual: one rounding)
    "swiglu": 1.866,     # bias + residual after SwiGLU (the tile kernel takes no residual there: 0.94 is one rounding)
    "rope": 0.9596,
    "layernorm": 0.9505,  # in-kernel statistics + gelu
    "rmsnorm": 0.8794,   # in-kernel statistics + SwiGLU
}
# silu and swiglu come within 7 % of their C = 2 here because these cases add a residual, a second
# honest rounding: two roundings reach at most 2 (gemm_checks' derivation), one reaches 1. The same
# kernel without a residual measures 0.924 (SwiGLU) and 0.973 (linear, bias only) — every family's
# figure above 1 is a residual case, between 1.85 and 1.91. Nothing is widened.

EXACT_SHAPES = ((1, 16, 32), (5, 48, 96), (16, 50, 64), (16, 272, 1056), (2, 1041, 256), (16, 64, 4160), (3, 769, 768))


def case_id(c):
    return "-".join(str(v) for v in c)


PLAIN_CASES = [(M, N, K) for (N, K) in PLAIN for M in MS]
SWIGLU_CASES = [(M, N, K) for (N, K) in SWIGLU for M in MS]
ROPE_CASES = [(M, S) for S in ROPE["S"] for M in MS]
FOLDED_CASES = [(mode, act, M, N, K) for (mode, act, N) in FOLDED for K in FOLDED_K for M in MS]
EXACT_CASES = [(kind,) + s for s in EXACT_SHAPES for kind in ("integer", "scaled", "selector")]


# ---------------------------------------------------------------------------------------------
# One launch on poisoned operands

def _padded(x, w, res, n_out, dev):
    """gemm_cases.padded with an [M][n_out] output / residual (SwiGLU: n_out = N / 2); the output
    view is pre-filled with NaN inside its canary buffer."""
    M = x.shape[0]
    pd = gc.padded(x, w, None, dev)
    rbuf = rv = None
    if res is not None:
        rbuf = torch.full((M + gc.PAD_ROWS, gc.out_ld(n_out)), NAN, dtype=BF)
        rbuf[:M, :n_out] = res
        rbuf = rbuf.to(dev)
        rv = rbuf[:M, :n_out]
    obuf = torch.full((M + gc.PAD_ROWS, gc.out_ld(n_out)), gc.CANARY, dtype=BF, device=dev)
    out = obuf[:M, :n_out]
    out.fill_(NAN)
    return pd._replace(res=rv, rbuf=rbuf, out=out, obuf=obuf)


def launch(fn, dev, x, w, bias=None, act=None, res=None, alpha=1.0, rope=None, norm=None, waves=None, what="",
           **kw):
    """fn on NaN-padded strided copies of the operands; checks the canaries and the residual buffer
    and returns the output view on the CPU."""
    M, N = x.shape[0], w.shape[0]
    n_out = N // 2 if act == "swiglu" else N
    pd = _padded(x, w, res, n_out, dev)
    if rope is not None:
        rope = (rope[0].to(dev), rope[1].to(dev)) + tuple(rope[2:])
    if norm is not None:
        norm = (norm[0].to(dev),) + tuple(norm[1:])
    y = fn(pd.a, pd.w, bias=None if bias is None else bias.to(dev), act=act, residual=pd.res, alpha=alpha, out=pd.out,
           rope=rope, norm=norm, waves=waves, **kw)
    assert y is pd.out
    gk.check_canary(pd, M, n_out, res, what)
    return pd.out.cpu()


@functools.lru_cache(maxsize=None)
def plain_ref(M, N, K, epi):
    c = gc.random_operands(M, N, K)
    bias, res = (c["bias"] if epi.bias else None), (c["res"] if epi.res else None)
    pre, ref = gk.ref64(c["x"], c["w"], bias, epi.act, res, epi.alpha)
    return c["x"], c["w"], bias, res, pre, ref, gk.absprod64(c["x"], c["w"])


def run_plain(fn, dev, case, waves=WAVES, epis=EPIS, **kw):
    M, N, K = case
    for epi in epis:
        x, w, bias, res, pre, ref, ap = plain_ref(M, N, K, epi)
        for W in waves:
            what = f"{epi.name} {(M, N, K)} W {W}"
            y = launch(fn, dev, x, w, bias, epi.act, res, epi.alpha, waves=W, what=what, **kw)
            gk.check_bound(y, pre, ref, ap, K, epi.family, what)


@functools.lru_cache(maxsize=None)
def swiglu_ref(M, N, K, epi):
    c = gc.random_operands(M, N, K)
    bias = c["bias"] if epi.bias else None
    res = c["res"][:, :N // 2].contiguous() if epi.res else None
    pre, ap = gk.ref64_swiglu(c["x"], c["w"], bias, epi.alpha)
    return c["x"], c["w"], bias, res, pre, (pre if res is None else pre + res.double()), ap


def run_swiglu(fn, dev, case, waves=WAVES, epis=SWIGLU_EPIS, **kw):
    M, N, K = case
    for epi in epis:
        x, w, bias, res, pre, ref, ap = swiglu_ref(M, N, K, epi)
        for W in waves:
            what = f"swiglu {epi.name} {(M, N, K)} W {W}"
            y = launch(fn, dev, x, w, bias, "swiglu", res, epi.alpha, waves=W, what=what, **kw)
            gk.check_bound(y, pre, ref, ap, K, "swiglu", what)


@functools.lru_cache(maxsize=None)
def rope_ref(M, S, with_bias):
    N, D, cols, K = ROPE["N"], ROPE["D"], ROPE["cols"], ROPE["K"]
    c = gc.random_operands(M, N, K)
    cos_t, sin_t = ops.rope_tables(S, D, 10000.0)
    bias = c["bias"] if with_bias else None
    ref, ap = gk.ref64_rope(c["x"], c["w"], bias, cos_t, sin_t, S, D, cols)
    return c["x"], c["w"], bias, (cos_t, sin_t, S, D, cols), ref, ap


def run_rope(fn, dev, case, waves=WAVES, **kw):
    M, S = case
    for with_bias in (False, True):
        x, w, bias, rope, ref, ap = rope_ref(M, S, with_bias)
        for W in waves:
            what = f"rope S {S} bias {with_bias} M {M} W {W}"
            y = launch(fn, dev, x, w, bias, None, None, 1.0, rope=rope, waves=W, what=what, **kw)
            gk.check_bound(y, ref, ref, ap, ROPE["K"], "rope", what)


@functools.lru_cache(maxsize=None)
def folded_ref(mode, act, M, N, K):
    """The derived operands of ops.derive_norm_gemm and the float64 reference on them; the row
    statistics come from x (the kernel takes them itself)."""
    c = gc.random_operands(M, N, K)
    wd, cs, bd = ops.derive_norm_gemm(c["w"], c["nw"], c["nb"] if mode == "layernorm" else None, c["bias"])
    ap = gk.absprod64(c["x"], wd)
    if act == "swiglu":
        v, _ = gk.ref64_folded(c["x"], wd, cs, bd, mode, None)
        v = v.reshape(M, N // 32, 2, 16)
        pre = (gk.act64(v[:, :, 0], "silu") * v[:, :, 1]).reshape(M, N // 2)
        ap = ap.reshape(M, N // 32, 2, 16).sum(2).reshape(M, N // 2)
    else:
        pre, _ = gk.ref64_folded(c["x"], wd, cs, bd, mode, act)
    return c["x"], wd, cs, bd, pre, ap


def run_folded(fn, dev, case, waves=WAVES, **kw):
    mode, act, M, N, K = case
    x, wd, cs, bd, pre, ap = folded_ref(mode, act, M, N, K)
    for W in waves:
        what = f"{mode} {act} {(M, N, K)} W {W}"
        y = launch(fn, dev, x, wd, bd, act, None, 1.0, norm=(cs, mode, gk.EPS), waves=W, what=what, **kw)
        gk.check_bound(y, pre, pre, ap, K, mode, what)


def run_exact(fn, dev, case, waves=WAVES, **kw):
    kind, M, N, K = case
    p = gc.probe(kind, M, N, K)
    for epi in (gc.EPI_NONE, gc.EPI_FULL):
        # (1, 16, 32) holds 32 values of x and 512 of w: too few for the SAMPLE statistics among the
        # preconditions (75 % non-zeros within 5 %, all 128 mantissas); what makes torch.equal the
        # right metric — every value exact in bf16 — is asserted by expected_exact for every shape
        if p.x.numel() >= 64:
            gk.check_probe_preconditions(p, epi)
        want = gk.expected_exact(p, epi)
        bias, res, act, alpha = gc.operands(p, epi)
        for W in waves:
            what = f"{kind} {epi.name} {(M, N, K)} W {W}"
            gk.check_exact(launch(fn, dev, p.x, p.w, bias, act, res, alpha, waves=W, what=what, **kw), want, what)


# One-hot probes whose selected k reaches every slice of K = 1056 (17 slices, the last one 32
# wide), so every wave's run of every W and the partial slice carry an output: gemm_cases.selector_k
# only reaches k < 116 at M <= 16.
ONEHOT_K = 1056
ONEHOT_SEL = (tuple(64 * m + (37 * m) % 64 for m in range(16)),
              (1055, 1024) + tuple(64 * (16 - m) - 1 - m for m in range(2, 16)))


def onehot_probe(which, N=272):
    sel = torch.tensor(ONEHOT_SEL[which])
    w = gc.selector_probe(16, N, ONEHOT_K).w
    x = torch.zeros(16, ONEHOT_K, dtype=BF)
    x[torch.arange(16), sel] = 1.0
    return x, w, w[:, sel].T.contiguous()


def check_onehot_coverage():
    slices = {k // 64 for s in ONEHOT_SEL for k in s}
    assert slices == set(range(17)), sorted(slices)
    assert any(k >= 1024 for s in ONEHOT_SEL for k in s)
    for W in WAVES:  # every non-empty wave run of every W holds a selected slice
        per = -(-17 // W)
        for wv in range(W):
            run = set(range(wv * per, min(17, wv * per + per)))
            assert not run or run & slices


def run_onehot(fn, dev, waves=WAVES, **kw):
    check_onehot_coverage()
    for which in (0, 1):
        x, w, want = onehot_probe(which)
        for W in waves:
            what = f"one-hot {which} W {W}"
            gk.check_exact(launch(fn, dev, x, w, waves=W, what=what, **kw), want, what)
            half = (0.5 * want.double()).clamp_min(0).to(BF)
            gk.check_exact(launch(fn, dev, x, w, act="relu", alpha=0.5, waves=W, what=what, **kw), half, what + " relu")


# ---------------------------------------------------------------------------------------------
# A torch model of the kernel, and what subtly wrong kernels would return

MUTANTS = ("first_wave_only", "last_slice_dropped", "ragged_row_n", "gate_up_off_by_one", "rope_partner_next_lane",
           "ln_mean_skipped", "residual_before_act")


def model(mutant=None):
    """``fn(x, w, ...)`` with linear_skinny's signature: fp32 partial sums per wave run of 64-wide
    slices, added in ascending wave order, the epilogue in the kernel's order, two roundings.
    ``mutant`` names one defect."""

    def fn(x, w, bias=None, act=None, residual=None, alpha=1.0, out=None, rope=None, norm=None, waves=None, **_):
        (M, K), N = x.shape, w.shape[0]
        W = waves or ops.skinny_waves(N, K, act)
        xf, wf = x.float(), w.float().clone()
        if mutant == "ragged_row_n" and N % 16 and w._base is not None:
            wf[N - 1] = w._base[N, :K].float()  # the last strip's clamp is off by one row
        nk = -(-K // 64)
        per = -(-nk // W)
        acc = torch.zeros(M, N)
        for wv in range(1 if mutant == "first_wave_only" else W):
            k0, k1 = wv * per * 64, min(K, (wv * per + per) * 64)
            if mutant == "last_slice_dropped" and K % 64:
                k1 = min(k1, K // 64 * 64)
            if k0 < k1:
                acc = acc + xf[:, k0:k1] @ wf[:, k0:k1].T
        v = alpha * acc
        if norm is not None:
            cs, mode, eps = norm
            ms = (xf * xf).sum(1, keepdim=True) / K
            if mode == "layernorm":
                mu = xf.sum(1, keepdim=True) / K
                rs = torch.rsqrt((ms - mu * mu).clamp_min(0) + eps)
                v = rs * (v if mutant == "ln_mean_skipped" else v - mu * cs.float())
            else:
                v = torch.rsqrt(ms + eps) * v
        if bias is not None:
            v = v + bias.float()
        r = None if residual is None else residual.float()
        if mutant == "residual_before_act" and r is not None and act != "swiglu":
            v, r = v + r, None
        if rope is not None:
            cos_t, sin_t, S, D, cols = rope
            pos = torch.arange(M) % S
            j = (torch.arange(cols) % D) // 2
            c, s = cos_t.float()[pos][:, j], sin_t.float()[pos][:, j]
            even = torch.arange(cols) % 2 == 0
            partner = torch.arange(cols) + torch.where(even, 1, -1)
            if mutant == "rope_partner_next_lane":
                partner = torch.where(even, (partner + 4) % cols, partner)
            p = v[:, :cols]
            rot = torch.where(even, p * c - p[:, partner] * s, p * c + p[:, partner] * s)
            v = torch.cat([rot, v[:, cols:]], 1)
        if act == "swiglu":
            blk = v.reshape(M, N // 32, 2, 16)
            up = blk[:, :, 1]
            if mutant == "gate_up_off_by_one":
                up = up.roll(-1, 1)
            v = (torch.nn.functional.silu(blk[:, :, 0]) * up).reshape(M, N // 2)
        else:
            v = gk.act64(v.double(), act).float()
        y = v.to(BF)
        if r is not None:
            y = (y.float() + r).to(BF)
        out.copy_(y)
        return out

    return fn
