"""MXFP4 expert weights on the GPU: the grouped W4A8 GEMM (csrc/kernels/gemm_w4a8_grouped.hip: fp4 x
fp8 on the block-scaled MFMA, weights global -> registers, the gathered e4m3 rows through LDS) and
the executor with ``weight_dtype="mxfp4-experts", act_dtype="fp8"``.

The lane maps (nibble order, the e4m3 operand's k order, which scale byte a lane group takes) and
the row-scale gather are proved by the exact tests: one-hot activations pick single weights and
every token carries its own power-of-two scale, so a wrong pairing gives a wrong value, not a
small error. Random operands are held to the fp32 product of the same dequantised values within
2e-2 of the reference's max (the measure of tests/test_w8_gpu.py): what remains is bf16 output
rounding and fp32 summation order.

Executor, measured on the CPU backend (weight_dtype="mxfp4-experts", act_dtype="fp8", against
reference.forward(act_dtype="fp8") on the same store, batch 2 x 64), as (max-abs error / max
|logit|, rms-relative error): the all-k variant of mini-mixtral (top_k = n_experts = 4: every
expert takes every token, so routing cannot differ) 0.0090 and 0.0085. Both backends are held
to 2 x those values with no row exempt (tests/test_mxfp4_experts_cpu.py holds the CPU executor to
the same rule). The ordinary top-2 mini-mixtral takes the margin measure of
tests/test_w8_experts_gpu.py: a row may be over the tolerance only if one of its router margins
is below 0.05 (44.5 % of the 128 rows in the reference), and fewer than 10 % of rows may be. Its
tolerance follows the same 2 x rule: over the rows whose margins are all >= 0.05 the CPU backend's
largest row error is 0.0159 of max |logit|, so the tolerance is 0.0318; the CPU backend itself has
1 of 128 rows (0.8 %, a row with a near-tie) over it."""
import functools

import pytest
import torch

from distributed_llm_scheduler_amd import ops
from distributed_llm_scheduler_amd.models import config, reference
from distributed_llm_scheduler_amd.parallel import executor as exm
from distributed_llm_scheduler_amd.parallel import runtime
from distributed_llm_scheduler_amd.parallel.executor import synthetic_tokens

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-2
WD = "mxfp4-experts"
F8 = torch.float8_e4m3fn
SENTINEL = 1000.0  # a bf16 value
E2M1 = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float32)
NCFG = 6  # (the last one sizes its tile by each group's count: up to its tile_rows, or 256 rows)
CFGS = [None] + list(range(NCFG))


def _h(cfg):
    """Tile height the counts are built around (config=None: the tall tiles' 128)."""
    return 128 if cfg is None else ops.w4a8_grouped_tile_rows(cfg)


def _counts(cfg):
    h = _h(cfg)
    return (0, 1, h - 1, h, h + 1, 2 * h + 3)


def _close(a, b, tol=TOL):
    err = (a.float() - b.float()).abs().max().item()
    ref = b.float().abs().max().item() + 1e-6
    assert err <= tol * ref, f"max abs err {err:.4g} vs ref max {ref:.4g} (rel tol {tol})"


def _same(y, want, what):
    """Exact equality of every value (a zero of either sign equals a zero)."""
    assert y.shape == want.shape, what
    assert torch.equal(y.float().cpu(), want.float().cpu()), what


def _pack(codes):
    """e2m1 codes [N, K] -> bytes [N, K/2]: even k in the low nibble."""
    codes = codes.to(torch.uint8)
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def _offsets(counts):
    return torch.tensor([0] + torch.tensor(list(counts)).cumsum(0).tolist(), dtype=torch.int32, device=DEV)


def _twice(T, seed):
    """A random order of the token rows 0..T-1 in which every token appears twice (top-2)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.arange(T).repeat(2)[torch.randperm(2 * T, generator=g)].to(torch.int32)


def _run(xq, xs, qs, ss, off, R, NO, cfg, act=None, a_rows=None, **kw):
    out = torch.full((R, NO), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ops.gemm_grouped_w4a8(xq, xs, qs, ss, off, act=act, out=out, a_rows=a_rows, config=cfg, **kw)
    return out


def test_config_table():
    assert ops.w4a8_grouped_configs() == NCFG  # (CFGS above covers every config)
    hs = [ops.w4a8_grouped_tile_rows(c) for c in range(NCFG)]
    assert min(hs) <= 32 and max(hs) >= 128 and all(h % 16 == 0 for h in hs)
    for hint, N, K, G in [(1, 28672, 4096, 8), (128, 28672, 4096, 8), (128, 4096, 14336, 8), (200, 4096, 14336, 8)]:
        assert 0 <= ops.ext().gemm_w4a8_grouped_pick(hint, N, K, G) < NCFG


# -------------------------------------------------------------------------- exact lane maps
@pytest.mark.parametrize("K", [128, 256])
def test_all_codes_bit_exact(K):
    """One-hot e4m3 rows reached through a random a_rows; group grp's weight row n holds code
    (n + k + 5 grp) % 16 at k, scale code 127: the output [r][n] is the decoded code at
    k = a_rows[r], bit for bit — the nibble order and the k pairing, through the gather."""
    N = 48
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    g = torch.Generator(device="cpu").manual_seed(3)
    a_rows = torch.cat([torch.randperm(K, generator=g), torch.randperm(K, generator=g)]).to(torch.int32)
    qs, ss, wants = [], [], []
    for grp in range(2):
        codes = (n + k + 5 * grp) % 16
        qs.append(_pack(codes).to(DEV))
        ss.append(torch.full((N, K // 32), 127, dtype=torch.uint8, device=DEV))
        wants.append(E2M1[codes].t()[a_rows[grp * K:(grp + 1) * K].long()])
    want = torch.cat(wants).to(torch.bfloat16)
    xq, xs = torch.eye(K).to(F8).to(DEV), torch.ones(K, device=DEV)
    off = _offsets([K, K])
    for cfg in CFGS:
        _same(_run(xq, xs, qs, ss, off, 2 * K, N, cfg, a_rows=a_rows.to(DEV)), want, f"config {cfg}")


@pytest.mark.parametrize("K", [416, 512])
def test_scale_placement_bit_exact(K):
    """Weights 1.0, scale code 120 + (3n + b + grp) % 15 at (row n, block b, group grp): a wrong
    scale byte, lane group, slice, row or group gives another power of two. K = 416: scale rows
    of 13 bytes (the byte loads, a last slice of one block); K = 512: 16 bytes (the dword loads)."""
    N = 48
    qs, ss, wants = [], [], []
    for grp in range(2):
        sc = 120 + (3 * torch.arange(N)[:, None] + torch.arange(K // 32)[None, :] + grp) % 15
        qs.append(torch.full((N, K // 2), 0x22, dtype=torch.uint8, device=DEV))
        ss.append(sc.to(torch.uint8).to(DEV))
        wants.append(torch.ldexp(torch.ones(K, N), (sc.t().repeat_interleave(32, 0) - 127).int()))
    want = torch.cat(wants).to(torch.bfloat16)
    xq = torch.eye(K).repeat(2, 1).to(F8).to(DEV)
    xs = torch.ones(2 * K, device=DEV)
    off = _offsets([K, K])
    for cfg in CFGS:
        _same(_run(xq, xs, qs, ss, off, 2 * K, N, cfg), want, f"config {cfg}")


@pytest.mark.parametrize("codes", [[0, 1, 2, 64, 126, 127, 128, 190, 253, 254],
                                   [0, 254, 1, 253, 2, 64, 126, 127, 128, 190, 0, 254]])
def test_extreme_scale_codes(codes):
    """Any scale code 0..254: weights 1.0, one block per code, one-hot rows (gathered) whose row
    scales bring 2^(code - 127) into the normal bf16 range. 10 codes: byte loads; 12: dword loads."""
    sc = torch.tensor(codes)
    N, K = 16, 32 * len(codes)
    q = torch.full((N, K // 2), 0x22, dtype=torch.uint8, device=DEV)
    s = sc.to(torch.uint8)[None, :].repeat(N, 1).to(DEV)
    e = (sc - 127).repeat_interleave(32)  # per k = per token
    xe = torch.where(e < -100, 40, torch.where(e > 100, -40, 0))
    xq = torch.eye(K).to(F8).to(DEV)
    xs = torch.ldexp(torch.ones(K), xe.int()).to(DEV)
    a_rows = torch.randperm(K, generator=torch.Generator().manual_seed(4)).to(torch.int32)
    want = torch.ldexp(torch.ones(K, N), (e + xe).int()[:, None].expand(K, N))[a_rows.long()].to(torch.bfloat16)
    for cfg in CFGS:
        _same(_run(xq, xs, [q], [s], _offsets([K]), K, N, cfg, a_rows=a_rows.to(DEV)), want, f"config {cfg}")


@functools.lru_cache(maxsize=None)
def _integer_problem(counts, K, gather):
    """The construction of tests/test_mxfp4_gpu.py::test_exact_integers_asymmetric per group: W in
    {+-0.5 .. +-6} with block scales 2^{0,1,2}, integer activations in [-8, 8]: every partial sum
    is a multiple of 0.5 below 2^20 (K <= 1152: 1152 * 24 * 8 < 2^18), so fp32 accumulation is
    exact in any order. Token t carries the row scale 2^((7t % 199) - 99): 199 different powers
    of two (all that keep 0.5 .. 2^18 times the scale inside bf16's normal range), different for
    any two tokens less than 199 apart — a scale taken at the sorted index r instead of the token
    index a_rows[r] is another power of two."""
    N, G, R = 130, len(counts), sum(counts)
    g = torch.Generator().manual_seed(5 + K + R)
    T = R // 2 if gather else R
    xi = torch.randint(-8, 9, (T, K), generator=g).float()
    xs = torch.ldexp(torch.ones(T), ((7 * torch.arange(T)) % 199 - 99).int())
    a_rows = _twice(T, 6) if gather else None
    rows = a_rows.long() if gather else torch.arange(R)
    qs, ss, want, lo = [], [], torch.zeros(R, N), 0
    for c in counts:
        codes = torch.randint(1, 8, (N, K), generator=g) + 8 * torch.randint(0, 2, (N, K), generator=g)
        sc = 127 + torch.randint(0, 3, (N, K // 32), generator=g)
        wd = E2M1[codes] * torch.ldexp(torch.ones(N, K // 32), (sc - 127).int()).repeat_interleave(32, 1)
        qs.append(_pack(codes).to(DEV))
        ss.append(sc.to(torch.uint8).to(DEV))
        r = rows[lo:lo + c]
        want[lo:lo + c] = (xi[r] @ wd.t()) * xs[r][:, None]
        lo += c
    xq = xi.to(F8)
    assert torch.equal(xq.float(), xi)
    return (xq.to(DEV), xs.to(DEV), qs, ss, _offsets(counts), None if a_rows is None else a_rows.to(DEV),
            want.to(torch.bfloat16))


@pytest.mark.parametrize("cfg", CFGS)
def test_exact_integers_asymmetric_bit_exact(cfg):
    """Counts spanning the tile edges in both orders, N = 130 (no tile multiple), K = 416 (a last
    slice of one block) and K = 1152 (9 slices: the weight ring wraps on a partial turn), with and
    without a_rows, a distinct power-of-two row scale per token."""
    for K in (416, 1152):
        for counts in (_counts(cfg), _counts(cfg)[::-1]):
            for gather in (False, True):
                if gather and sum(counts) % 2:
                    counts = counts[:-1] + (counts[-1] + 1,)
                xq, xs, qs, ss, off, a_rows, want = _integer_problem(counts, K, gather)
                y = _run(xq, xs, qs, ss, off, sum(counts), 130, cfg, a_rows=a_rows)
                _same(y, want, f"config {cfg} K {K} counts {counts} gather {gather}")


# ----------------------------------------------------------------------------------- random
class _Problem:
    """G groups over ``counts`` rows: e4m3 token rows (quantised N(0, 1)) with arbitrary fp32 row
    scales in [1e-3, 10], MXFP4 weights (quantised N(0, 0.02); gate/up rows of q AND s interleaved
    for SwiGLU), and the fp32 product of the same dequantised values for every sorted row."""

    def __init__(self, counts, N, K, swiglu, gather, seed=0, weights_of=None):
        G, R = len(counts), sum(counts)
        self.counts, self.R, self.swiglu = counts, R, swiglu
        self.NO = N // 2 if swiglu else N
        self.act = "swiglu" if swiglu else None
        weights_of = weights_of or list(range(G))
        g = torch.Generator(device="cpu").manual_seed(500 + seed)
        if gather:
            assert R % 2 == 0
            T, self.a_rows = R // 2, _twice(R // 2, seed + 2).to(DEV)
        else:
            T, self.a_rows = R, None
        xq, _ = ops.quantize_fp8(torch.randn(T, K, generator=g).to(torch.bfloat16))
        xs = torch.exp(torch.empty(T).uniform_(-6.9077, 2.3026, generator=g)).clamp_(1e-3, 10.0)
        self.xq, self.xs = xq.to(DEV), xs.to(DEV)
        xd = self.xq.float() * self.xs[:, None]
        if gather:
            xd = xd[self.a_rows.long()]
        nat = {}
        for w in sorted(set(weights_of)):
            q, s = ops.quantize_mxfp4((0.02 * torch.randn(N, K, generator=g)).to(torch.bfloat16))
            nat[w] = (q.to(DEV), s.to(DEV))
        il = (lambda t: ops.interleave_gate_up(t)) if swiglu else (lambda t: t)
        given = {w: (il(q), il(s)) for w, (q, s) in nat.items()}
        self.qs = [given[w][0] for w in weights_of]
        self.ss = [given[w][1] for w in weights_of]
        self.off = _offsets(counts)
        ref = torch.zeros(R, self.NO, device=DEV)
        lo = 0
        for gi, c in enumerate(counts):
            q, s = nat[weights_of[gi]]
            y = xd[lo:lo + c] @ ops.dequantize_mxfp4(q, s, torch.float32).t()
            ref[lo:lo + c] = torch.nn.functional.silu(y[:, :N // 2]) * y[:, N // 2:] if swiglu else y
            lo += c
        self.ref = ref

    def run(self, cfg, **kw):
        return _run(self.xq, self.xs, self.qs, self.ss, self.off, self.R, self.NO, cfg, act=self.act,
                    a_rows=self.a_rows, **kw)


@functools.lru_cache(maxsize=None)
def _problem(counts, N, K, swiglu, gather, seed=0):
    return _Problem(list(counts), N, K, swiglu, gather, seed)


@pytest.mark.parametrize("cfg", CFGS)
def test_random_operands_every_config(cfg):
    """N = 48 / 136 / 256 (and 512 with SwiGLU): column tails and whole tiles; K = 32 and 160 end
    in a partial slice, 416 in a slice of one block (byte-wise scale loads), 1024 is whole slices
    (dword loads); counts around the config's tile height, forwards without and backwards with the
    row gather."""
    c = _counts(cfg)
    even = c[:-1] + (c[-1] + sum(c) % 2,)
    for N, sw in [(48, False), (136, False), (256, False), (512, True)]:
        for K in (32, 160, 416, 1024):
            for counts, gather in ((c, False), (even[::-1], True)):
                pb = _problem(counts, N, K, sw, gather, seed=K + N)
                _close(pb.run(cfg), pb.ref)


@pytest.mark.parametrize("N,K,sw", [(256, 4096, True), (128, 14336, False)])
def test_mixtral_full_k_on_a_narrow_column_slice(N, K, sw):
    """Mixtral's K of gate/up (4096, SwiGLU) and down (14336) on a few columns, counts around the
    tile heights and a real step's spread."""
    pb = _Problem([0, 1, 97, 128, 149, 192, 193, 264], N, K, sw, gather=sw, seed=5)
    for cfg in CFGS:
        _close(pb.run(cfg), pb.ref)


@pytest.mark.parametrize("col0", [8, 3])
def test_no_stray_writes_out_view(col0):
    """``out`` is a view inside a sentinel-filled buffer (8-byte aligned and unaligned: vector
    and scalar stores), row and column tails; rows of ``out`` that belong to no group (before
    offsets[0], after offsets[G]) stay untouched."""
    for N, K, sw in [(136, 224, False), (96, 64, True)]:
        pb = _problem((5, 0, 37, 70), N, K, sw, False, seed=7)
        lead, trail = 3, 4
        off = pb.off + lead
        g = torch.Generator().manual_seed(1)
        pad = lambda n: torch.randn(n, K, generator=g).to(F8).to(DEV)  # noqa: E731
        xq = torch.cat([pad(lead), pb.xq, pad(trail)])
        xs = torch.cat([torch.ones(lead, device=DEV), pb.xs, torch.ones(trail, device=DEV)])
        R = xq.shape[0]
        for cfg in CFGS:
            big = torch.full((R + 5, pb.NO + 24), SENTINEL, dtype=torch.bfloat16, device=DEV)
            out = big[2:2 + R, col0:col0 + pb.NO]
            ops.gemm_grouped_w4a8(xq, xs, pb.qs, pb.ss, off, act=pb.act, out=out, config=cfg)
            _close(out[lead:lead + pb.R], pb.ref)
            mask = torch.ones_like(big, dtype=torch.bool)
            mask[2 + lead:2 + lead + pb.R, col0:col0 + pb.NO] = False
            assert (big[mask] == SENTINEL).all(), f"config {cfg}"


def test_no_stray_writes_compact_outputs():
    """Compact ``outs[g]`` with fewer rows than the largest group's count: rows past
    min(count, cap) unwritten, the buffer behind each output untouched."""
    counts, cap = (5, 0, 37, 70), 40
    for N, K, sw in [(136, 224, False), (96, 64, True)]:
        pb = _problem(counts, N, K, sw, True, seed=9)
        for cfg in CFGS:
            big = torch.full((len(counts), cap + 3, pb.NO), SENTINEL, dtype=torch.bfloat16, device=DEV)
            outs = [big[g, :cap] for g in range(len(counts))]
            ops.gemm_grouped_w4a8(pb.xq, pb.xs, pb.qs, pb.ss, pb.off, act=pb.act, outs=outs, a_rows=pb.a_rows,
                                  config=cfg)
            lo = 0
            for g, c in enumerate(counts):
                n = min(c, cap)
                if n:
                    _close(outs[g][:n], pb.ref[lo:lo + n])
                assert (big[g, n:] == SENTINEL).all(), f"config {cfg} group {g}"
                lo += c


def test_shared_weights():
    """4 groups over 2 distinct weights (a cross-request expert batch: same-weight groups
    adjacent) equal the per-group run bitwise."""
    for sw, N in [(False, 136), (True, 256)]:
        pb = _Problem([33, 70, 1, 130], N, 224, sw, gather=True, seed=11, weights_of=[0, 0, 1, 1])
        assert pb.qs[0].data_ptr() == pb.qs[1].data_ptr() != pb.qs[2].data_ptr()
        for cfg in CFGS:
            y = pb.run(cfg, shared_weights=True)
            _close(y, pb.ref)
            assert torch.equal(y, pb.run(cfg)), f"config {cfg}"


def test_two_runs_are_bitwise_equal():
    pb = _Problem([0, 1, 97, 128, 149, 192, 193, 264], 256, 1024, True, gather=True, seed=13)
    for cfg in CFGS:
        assert torch.equal(pb.run(cfg), pb.run(cfg)), f"config {cfg}"


def test_wrong_operands_are_refused():
    pb = _problem((4, 4), 64, 64, False, False)
    out = torch.empty(8, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(TypeError):  # bf16 activations
        ops.gemm_grouped_w4a8(pb.xq.float().to(torch.bfloat16), pb.xs, pb.qs, pb.ss, pb.off, out=out)
    with pytest.raises(TypeError):  # e4m3-typed weights
        ops.gemm_grouped_w4a8(pb.xq, pb.xs, [q.view(F8) for q in pb.qs], pb.ss, pb.off, out=out)
    with pytest.raises(TypeError):  # fp32 block scales
        ops.gemm_grouped_w4a8(pb.xq, pb.xs, pb.qs, [s.float() for s in pb.ss], pb.off, out=out)
    with pytest.raises(ValueError, match="multiple of 32"):  # K = 48
        ops.gemm_grouped_w4a8(pb.xq[:, :48].contiguous(), pb.xs, [q[:, :24].contiguous() for q in pb.qs], pb.ss,
                              pb.off, out=out)
    with pytest.raises(ValueError, match="expected q"):
        ops.gemm_grouped_w4a8(pb.xq, pb.xs, pb.qs, [s[:, :1] for s in pb.ss], pb.off, out=out)
    with pytest.raises(ValueError, match="xscale"):  # one entry per row of xq
        ops.gemm_grouped_w4a8(pb.xq, pb.xs[:4], pb.qs, pb.ss, pb.off, out=out)
    with pytest.raises(ValueError, match="config"):
        ops.gemm_grouped_w4a8(pb.xq, pb.xs, pb.qs, pb.ss, pb.off, out=out, config=ops.w4a8_grouped_configs())
    with pytest.raises(RuntimeError, match="config"):  # the binding's own check
        ops.ext().gemm_grouped_w4a8(pb.xq, pb.xs, pb.qs, pb.ss, torch.zeros(2, dtype=torch.int64, device=DEV),
                                    torch.zeros(2, dtype=torch.int64, device=DEV), pb.off, 0, out, [], None,
                                    ops.w4a8_grouped_configs())


def test_expert_layer_chain_with_device_routing():
    """route -> gate/up (rows AND row scales gathered by the device's src_rows, SwiGLU) -> row
    quantiser -> down (compact outputs) -> gather-combine, against fp32 using the idx / gate
    tensors the device produced: no row is exempt."""
    M, E, H, F, topk = 128, 4, 256, 256, 2
    g = torch.Generator(device="cpu").manual_seed(21)
    x = torch.randn(M, H, generator=g).to(torch.bfloat16).to(DEV)
    logits = torch.randn(M, E, generator=g).to(torch.bfloat16).to(DEV)
    idx, gate, src, slot, off = ops.moe_route(logits, topk, E)
    mk = lambda n, k: ops.quantize_mxfp4((0.05 * torch.randn(n, k, generator=g)).to(torch.bfloat16).to(DEV))  # noqa: E731
    w13 = [mk(2 * F, H) for _ in range(E)]
    w2 = [mk(H, F) for _ in range(E)]
    q13 = [ops.interleave_gate_up(q) for q, _ in w13]
    s13 = [ops.interleave_gate_up(s) for _, s in w13]
    hbuf = torch.zeros(M * topk, F, dtype=torch.bfloat16, device=DEV)
    outs = [torch.zeros(M, H, dtype=torch.bfloat16, device=DEV) for _ in range(E)]
    y = torch.zeros(M, H, dtype=torch.bfloat16, device=DEV)
    xq, xs = ops.quantize_rows_fp8(x)
    ops.gemm_grouped_w4a8(xq, xs, q13, s13, off, act="swiglu", out=hbuf, a_rows=src, rows_hint=M * topk // E)
    hq, hs = ops.quantize_rows_fp8(hbuf)
    ops.gemm_grouped_w4a8(hq, hs, [q for q, _ in w2], [s for _, s in w2], off, outs=outs, rows_hint=M * topk // E)
    ops.moe_gather_combine(outs, idx, slot, off, gate, out=y)
    torch.cuda.synchronize()
    want = torch.zeros(M, H, device=DEV)
    xd = ops.dequantize_fp8(*ops.quantize_fp8(x), torch.float32)
    for e in range(E):
        gu = xd @ ops.dequantize_mxfp4(*w13[e], torch.float32).t()
        h = (torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]).to(torch.bfloat16)  # hbuf is bf16
        hd = ops.dequantize_fp8(*ops.quantize_fp8(h), torch.float32)
        ye = hd @ ops.dequantize_mxfp4(*w2[e], torch.float32).t()
        for j in range(topk):
            sel = idx[:, j].long() == e
            want[sel] += gate[sel, j, None].float() * ye[sel]
    assert int(off[-1]) == M * topk
    _close(y, want)


# ------------------------------------------------------------------------------ executor
ALLK = "mini-mixtral-allk"
ALLK_CPU = (0.0090, 0.0085)  # CPU backend, all-k mini-mixtral, batch 2 x 64 (the header)
TOP2_TOL = 2 * 0.0159       # CPU backend, top-2 mini-mixtral, rows with every margin >= 0.05


@pytest.fixture
def allk(monkeypatch):
    c = config.PRESETS["mini-mixtral"]
    monkeypatch.setitem(config.PRESETS, ALLK, c.with_(name=ALLK, top_k=c.n_experts))
    return ALLK


def _plan(model, **kw):
    p = runtime.plan(model, world=1, seq=64, batch=2, weight_dtype=WD, act_dtype="fp8", **kw)
    assert p.completed == p.total and p.args["weight_dtype"] == WD
    return p


def _check_allk(p, ex, store, rid=""):
    """No row exempt: every expert takes every token, so routing cannot differ."""
    out = ex.output(f"{rid}output_projection").float().cpu()
    B, S = out.shape[0], out.shape[1]
    tok = synthetic_tokens(f"{rid}@tokens", B * S, p.cfg.vocab_size).view(B, S)
    ref = reference.forward(p.cfg, store, tok, act_dtype="fp8")
    d = out - ref
    maxrel = d.abs().max().item() / ref.abs().max().item()
    rmsrel = (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    print(f"{p.cfg.name} {rid}: max-abs / max-|logit| {maxrel:.4f}, rms-relative {rmsrel:.4f}")
    assert maxrel <= 2 * ALLK_CPU[0] and rmsrel <= 2 * ALLK_CPU[1], (maxrel, rmsrel)


def _check(p, ex, store, tol, rid=""):
    """The measure of tests/test_w8_experts_gpu.py::_check, against the fp8-activation reference."""
    out = ex.output(f"{rid}output_projection").float().cpu()
    B, S = out.shape[0], out.shape[1]
    tok = synthetic_tokens(f"{rid}@tokens", B * S, p.cfg.vocab_size).view(B, S)
    margins = []
    ref = reference.forward(p.cfg, store, tok, router_margins=margins, act_dtype="fp8")
    scale = ref.abs().max().item()
    assert margins
    row_err = (out - ref).abs().amax(-1)
    risky = torch.stack([m.abs() < 0.05 for m in margins]).any(0)
    bad = row_err > tol * scale
    print(f"{p.cfg.name} {rid}: bad rows {int(bad.sum())}/{bad.numel()}, risky {int(risky.sum())}, "
          f"max row err / scale {row_err.max().item() / scale:.4f}")
    assert bad.float().mean().item() < 0.1, (int(bad.sum()), int(risky.sum()), row_err.max().item(), scale)
    assert not (bad & ~risky).any(), (int((bad & ~risky).sum()), int(bad.sum()), row_err[~risky].max().item(), scale)


@pytest.mark.parametrize("graph", [False, True])
def test_all_k_dag_on_gpu_matches_reference(allk, graph):
    p = _plan(allk)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, torch.device("cuda:0"), store, use_graph=graph)
    assert len(ex._moe_batch) == p.cfg.n_layer
    ex.step()
    if graph:
        assert ex.capture()  # the whole step is one captured graph, nothing allocated inside
        ex.step()
        first = ex.output("output_projection").clone()
        ex.step()
        assert torch.equal(ex.output("output_projection"), first)  # a second replay is bitwise equal
    torch.cuda.synchronize()
    _check_allk(p, ex, store)


@pytest.mark.parametrize("graph", [False, True])
def test_top2_dag_on_gpu_matches_reference(graph):
    p = _plan("mini-mixtral")
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, torch.device("cuda:0"), store, use_graph=graph)
    assert len(ex._moe_batch) == p.cfg.n_layer  # the grouped launch pair per layer
    ex.step()
    if graph:
        assert ex.capture()
        ex.step()
        first = ex.output("output_projection").clone()
        ex.step()
        assert torch.equal(ex.output("output_projection"), first)
    torch.cuda.synchronize()
    name = next(s.name for g in p.groups.values() for s in g.tensors if s.quant)
    assert ex._w(name).dtype == torch.uint8 and ex._w(name + "@scale").dtype == torch.uint8
    assert ex._w("layers.0.moe.gate").dtype == torch.bfloat16
    _check(p, ex, store, TOP2_TOL)


def test_executor_without_fp8_activations_is_refused():
    p = _plan("mini-mixtral")
    store = runtime.make_store(p)
    with pytest.raises(ValueError, match="act_dtype"):
        exm.DAGExecutor(p.tasks, p.programs[0], store, torch.device("cuda:0"), model_cfg=p.cfg, autotune=False)


def test_memory_capped_reloads_on_gpu(allk):
    """0.6 x the mode's bytes: refills land in other arena regions, so the interleaved q / s must
    have reached the host image the refills copy."""
    for model, check in ((allk, _check_allk), ("mini-mixtral", lambda *a: _check(*a, TOP2_TOL))):
        need = sum(runtime.make_store(_plan(model)).nbytes(g) for g in _plan(model).groups) / 1e9
        p = _plan(model, cap_gb=need * 0.6)
        store = runtime.make_store(p)
        ex = runtime.make_executor(p, 0, torch.device("cuda:0"), store, use_graph=False)
        for _ in range(2):
            st = ex.step()
        assert st.param_fills > 0
        torch.cuda.synchronize()
        check(p, ex, store)


def test_cross_request_batch_on_gpu(allk, monkeypatch):
    """Two requests on one GPU: each layer's expert nodes of both requests run as one grouped
    launch pair with shared weights (_run_moe_xbatch), checked per request."""
    monkeypatch.setattr(exm, "MOE_BATCH", False)  # the per-request batch would take the nodes first
    for model, check in ((allk, _check_allk), ("mini-mixtral", lambda *a: _check(a[0], a[1], a[2], TOP2_TOL, a[3]))):
        p = _plan(model, replicas=2)
        store = runtime.make_store(p)
        ex = runtime.make_executor(p, 0, torch.device("cuda:0"), store, use_graph=False)
        assert len(ex._xbatch) == p.cfg.n_layer and not ex._moe_batch
        ex.step()
        torch.cuda.synchronize()
        for rid in ("r0/", "r1/"):
            check(p, ex, store, rid)


def test_single_expert_nodes_on_gpu(allk, monkeypatch):
    """With the batches switched off every expert node runs alone (_moe_expert: a one-group
    launch pair; the permuted rows are quantised once per layer and shared)."""
    monkeypatch.setattr(exm, "MOE_BATCH", False)
    monkeypatch.setattr(exm, "MOE_XBATCH", False)
    for model, check in ((allk, _check_allk), ("mini-mixtral", lambda *a: _check(*a, TOP2_TOL))):
        p = _plan(model)
        store = runtime.make_store(p)
        ex = runtime.make_executor(p, 0, torch.device("cuda:0"), store, use_graph=False)
        assert not ex._moe_batch and not ex._xbatch
        ex.step()
        torch.cuda.synchronize()
        check(p, ex, store)
