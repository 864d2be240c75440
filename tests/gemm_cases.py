"""Inputs of the bf16 GEMM tests (test_gemm_ref_cpu.py, test_gemm_exact_gpu.py), built on the CPU
once per shape; the checks and references live in gemm_checks.py.

Three kinds of probe have an output that is exact in EVERY summation order, so a kernel is held
to ``torch.equal`` with no tolerance:

* integer probes: x, w in {-1, 0, 1} (75 % non-zeros), bias an integer in [-8, 8], the residual an
  integer in [-16, 16], alpha 1 or 0.5. Every partial sum is an integer below 2^24 (exact in
  fp32) and every value the epilogue forms is an integer or half-integer that bf16 holds;
* scaled probes: the same integers with row m of x times 2^(m % 5 - 2) and row n of w times
  2^(n % 7 - 3): output (m, n) is the integer sum times one power of two, so the exponent bits
  of both operands take part and nothing rounds;
* selector probes: x is one-hot at k = (7 m + 3) mod K and w is random bf16 with full mantissas
  and magnitudes across 2^+-30: the output is w[:, sel].T, bit for bit.

``padded`` puts A, W, the residual and the output into larger buffers whose padding columns and
three extra rows hold NaN (the output: a canary), so a read past a row's K-th element or past
row M - 1 / N - 1 that reaches the output turns it into NaN and a store outside [M][N] shows.
"""
import functools
from collections import namedtuple

import torch

BF = torch.bfloat16

# (bm, bn, K step) of every LDS-DMA config as the kernels are instantiated: the shapes below
# follow from it. The GPU tests hold the binding's gemm_glds_tile / gemm_glds_kstep to this table.
TILES = {
    0: (256, 128, 64), 1: (128, 128, 64), 2: (128, 64, 64), 3: (64, 64, 64), 4: (64, 128, 64), 5: (64, 64, 64),
    6: (128, 64, 64), 7: (128, 128, 64), 8: (256, 256, 64), 9: (256, 256, 64), 10: (256, 128, 64),
    11: (128, 128, 64), 12: (256, 256, 64), 13: (256, 256, 64), 14: (256, 128, 64), 15: (128, 128, 64),
    16: (64, 64, 128), 17: (64, 64, 128), 18: (128, 64, 128), 19: (64, 128, 128), 20: (64, 64, 256),
    21: (64, 64, 256), 22: (64, 96, 64), 23: (32, 144, 64), 24: (32, 48, 64), 25: (64, 96, 128),
    26: (32, 144, 128), 27: (32, 48, 128), 28: (128, 128, 128), 29: (192, 128, 64), 30: (192, 128, 128),
    31: (192, 128, 64), 32: (192, 128, 64), 33: (192, 128, 64), 34: (256, 256, 64), 35: (256, 256, 64),
    36: (256, 224, 64), 37: (256, 224, 64), 38: (128, 96, 64), 39: (128, 96, 128), 40: (128, 64, 128),
    41: (192, 128, 64), 42: (256, 144, 64), 43: (256, 192, 64), 44: (160, 256, 64), 45: (32, 48, 256),
    46: (128, 128, 64), 47: (128, 128, 64),
}
GLDS = sorted(TILES)
# register-staged kernel (any K % 8 == 0): ids 100..103, tiles 128x128, 64x128, 64x64, 32x64
REGSTAGE = {100: (128, 128, 64), 101: (64, 128, 64), 102: (64, 64, 64), 103: (32, 64, 64)}
ALL_CONFIGS = GLDS + sorted(REGSTAGE)
# configs whose wave tiles cannot pair SwiGLU gate/up fragments (the launcher reroutes them)
SWIGLU_BAD = {22, 23, 24, 25, 26, 27, 36, 38, 39, 42, 45}
N_KINDS = ("seg", "odd")  # N = bn + 24: whole 16-byte segments; bn + 2: unaligned rows, scalar stores


def tile(config):
    return TILES.get(config) or REGSTAGE[config]


def shape(config, n_kind, ksteps=12):
    """(M, N, K) of a config's probes: two row tiles, the second with five rows; a partial second
    column tile; K = 12 K steps, so every ring of 2 to 8 stages wraps and K splits into 2, 3 and
    4 slices of whole steps."""
    bm, bn, ks = tile(config)
    return bm + 5, bn + (24 if n_kind == "seg" else 2), ksteps * ks


def probe_shapes():
    """Every distinct (M, N, K) the exact probes run at."""
    return sorted({shape(c, n) for c in ALL_CONFIGS for n in N_KINDS})


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def _ternary(rows, cols, seed):
    g = _gen(seed)
    sign = torch.randint(0, 2, (rows, cols), generator=g) * 2 - 1
    keep = torch.rand(rows, cols, generator=g) < 0.75
    return (sign * keep).to(BF)


Probe = namedtuple("Probe", "kind x w bias res")


@functools.lru_cache(maxsize=None)
def integer_probe(M, N, K):
    g = _gen(7000 + M + 3 * N + 5 * K)
    return Probe("integer", _ternary(M, K, 7100 + M + K), _ternary(N, K, 7200 + N + K),
                 torch.randint(-8, 9, (N,), generator=g).to(BF), torch.randint(-16, 17, (M, N), generator=g).to(BF))


@functools.lru_cache(maxsize=None)
def scaled_probe(M, N, K):
    p = integer_probe(M, N, K)
    sx = torch.pow(2.0, (torch.arange(M) % 5 - 2).float())[:, None]
    sw = torch.pow(2.0, (torch.arange(N) % 7 - 3).float())[:, None]
    return Probe("scaled", (p.x.float() * sx).to(BF), (p.w.float() * sw).to(BF), None, None)


def selector_k(M, K):
    return (7 * torch.arange(M) + 3) % K


@functools.lru_cache(maxsize=None)
def selector_probe(M, N, K):
    """x one-hot; w from random bits: sign, a biased exponent in [97, 157] (2^-30 .. 2^30) and a
    full 7-bit mantissa — no zero, subnormal, Inf or NaN."""
    g = _gen(7300 + M + 3 * N + 5 * K)
    x = torch.zeros(M, K, dtype=BF)
    x[torch.arange(M), selector_k(M, K)] = 1.0
    bits = (torch.randint(0, 2, (N, K), generator=g) << 15) | (torch.randint(97, 158, (N, K), generator=g) << 7) \
        | torch.randint(0, 128, (N, K), generator=g)
    w = torch.where(bits >= 32768, bits - 65536, bits).to(torch.int16).view(BF)  # the 16 bits, as bf16
    return Probe("selector", x, w, None, None)


PROBES = {"integer": integer_probe, "scaled": scaled_probe, "selector": selector_probe}


def probe(kind, M, N, K):
    return PROBES[kind](M, N, K)


# The two epilogues of the exact probes. Bias and residual exist on the integer probes only (on
# the others they would round); alpha and the activation apply to all three.
Epilogue = namedtuple("Epilogue", "name bias res act alpha")
EPI_NONE = Epilogue("none", False, False, None, 1.0)
EPI_FULL = Epilogue("bias_relu_res_half", True, True, "relu", 0.5)


def operands(p, epi):
    """(bias, residual, act, alpha) a probe runs ``epi`` with."""
    return (p.bias if epi.bias else None), (p.res if epi.res else None), epi.act, epi.alpha


# ---------------------------------------------------------------------------------------------
# Poisoned, strided operands

PAD_ROWS = 3
CANARY = -7.0
Padded = namedtuple("Padded", "a w res out abuf wbuf rbuf obuf")


def out_ld(N):
    """Row stride of a padded output / residual: 16-byte rows where N allows them (whole-segment
    stores next to live canary bytes), odd otherwise."""
    return N + 8 if N % 8 == 0 else N + 3


def padded(x, w, res, device="cpu"):
    """Views [M][K] / [N][K] / [M][N] into NaN-filled buffers with lda = K + 8, ldw = K + 16, three
    extra rows each; the output view sits in a canary buffer."""
    (M, K), N = x.shape, w.shape[0]
    nan = float("nan")
    abuf = torch.full((M + PAD_ROWS, K + 8), nan, dtype=BF)
    wbuf = torch.full((N + PAD_ROWS, K + 16), nan, dtype=BF)
    abuf[:M, :K] = x
    wbuf[:N, :K] = w
    rbuf = None
    if res is not None:
        rbuf = torch.full((M + PAD_ROWS, out_ld(N)), nan, dtype=BF)
        rbuf[:M, :N] = res
        rbuf = rbuf.to(device)
    abuf, wbuf = abuf.to(device), wbuf.to(device)
    obuf = torch.full((M + PAD_ROWS, out_ld(N)), CANARY, dtype=BF, device=device)
    return Padded(abuf[:M, :K], wbuf[:N, :K], None if rbuf is None else rbuf[:M, :N], obuf[:M, :N],
                  abuf, wbuf, rbuf, obuf)


# ---------------------------------------------------------------------------------------------
# Random operands of the bounded epilogues (rows with a non-zero mean, asymmetric)

def _rand(*shp, scale=1.0, seed=0):
    return (scale * torch.randn(*shp, generator=_gen(seed))).to(BF)


@functools.lru_cache(maxsize=None)
def random_operands(M, N, K):
    """x ~ 0.4 + 2 N(0, 1), w ~ 0.04 N(0, 1), bias, residual, a norm gain / bias over K (folded
    norms) and over N (post-norm), and x's row statistics in fp32 as a producer would emit them."""
    s = 7500 + M + 3 * N + 5 * K
    c = {
        "x": _rand(M, K, scale=2.0, seed=s) + 0.4,
        "w": _rand(N, K, scale=0.04, seed=s + 1),
        "bias": _rand(N, scale=0.2, seed=s + 2),
        "res": _rand(M, N, seed=s + 3),
        "nw": (1 + 0.2 * _rand(K, seed=s + 4).float()).to(BF),
        "nb": _rand(K, scale=0.1, seed=s + 5),
        "pw": (1 + 0.2 * _rand(N, seed=s + 6).float()).to(BF),
        "pb": _rand(N, scale=0.1, seed=s + 7),
    }
    xd = c["x"].double()
    c["stats"] = torch.stack([xd.sum(1), (xd * xd).sum(1)], 1).float()
    return c
