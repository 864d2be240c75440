"""``ops.gemm_grouped_skinny_w8`` (csrc/kernels/gemm_grouped_skinny_w8.hip): the random weights of
moe_skinny_cases.build quantised by ``ops.quantize_fp8``, the float64 reference on
``q.double() * scale``, ``gemm_checks.check_bound`` with ``C_BOUND`` unchanged, under
moe_skinny_cases.make_run's poison; every weight sits between bytes of the e4m3 NaN code (the weights
are contiguous: that is where "past K" is). (16 / 32, 32): a quarter slice; (48 / 96, 160): a slice
and a quarter, empty waves, an odd count of 32-column strips; (64, 2112): 16.5 slices, uneven runs."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as gc  # noqa: E402
import gemm_checks as gk  # noqa: E402
import moe_skinny_cases as S  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
FN = ops.gemm_grouped_skinny_w8
BF = torch.bfloat16
PLAIN, SWIGLU = ((16, 32), (48, 160), (64, 2112)), ((32, 32), (96, 160), (64, 2112))
COUNTS = ((0, 0, 0, 2), (1, 0, 16, 7), (0,) * 7 + (1,), (17, 0, 33, 5))
CASES = {"none": [("none", nk, c) for nk in PLAIN for c in COUNTS], "swiglu": [("swiglu", nk, c) for nk in SWIGLU for c in COUNTS]}
INSTANCES = {"none": [(W, s) for W in (4, 8) for s in (16, 32)], "swiglu": [(4, 16), (8, 16)]}


def refs64(act, rows, counts, w64):
    refs, pres, aps, r = [], [], [], 0
    for e, n in enumerate(counts):
        x = rows[r:r + n]
        r += n
        if act == "swiglu":
            ref, ap = gk.ref64_swiglu(x, w64[e])
            pre = ref
        else:
            (pre, ref), ap = gk.ref64(x, w64[e]), gk.absprod64(x, w64[e])
        refs.append(ref), pres.append(pre), aps.append(ap)
    return dict(refs=tuple(refs), pres=tuple(pres), aps=tuple(aps))


@functools.lru_cache(maxsize=None)
def build(act, nk, counts, arbitrary=False):
    """(moe_skinny_cases.Case with the references of the quantised weights, q list, scale list).
    ``arbitrary``: the scales replaced by positive fp32 values in [2^-12, 2^-2], no powers of two."""
    c = S.build(act, nk, counts)
    qs = [ops.quantize_fp8(w) for w in c.weights]
    if arbitrary:
        g = torch.Generator().manual_seed(sum(nk))
        qs = [(q, (2.0 ** -12 * 1024.0 ** torch.rand(nk[0], generator=g)).float()) for q, _ in qs]
    w64 = [q.float().double() * s.double()[:, None] for q, s in qs]
    return c._replace(**refs64(act, c.rows, counts, w64)), [q for q, _ in qs], [s for _, s in qs]


def on_device(qs, ss):
    out = []
    for q in qs:  # 16 bytes of the NaN code before the weight, 48 after it
        buf = torch.full((q.numel() + 64,), 0x7f, dtype=torch.uint8)
        buf[16:16 + q.numel()] = q.contiguous().view(torch.uint8).flatten()
        out.append(buf.to(DEV)[16:16 + q.numel()].view(torch.float8_e4m3fn).view(q.shape))
    return out, [s.to(DEV) for s in ss]


def launch(c, qd, sd, run, W=None, strip=None, **kw):
    FN(run.x, qd, sd, run.offsets, act=None if c.act == "none" else c.act, out=run.out, outs=run.outs,
       a_rows=run.a_rows, waves=W, strip=strip, **kw)


def verify(c, run, what):
    """Bounds of the owned rows; NaN where nobody owns a row; every canary whole."""
    worst = 0.0
    for e, (got, n) in enumerate(S.group_outputs(c, run)):
        if n:
            worst = max(worst, gk.check_bound(got, c.pres[e][:n], c.refs[e][:n], c.aps[e][:n], c.K,
                                              "swiglu" if c.act == "swiglu" else "linear", f"{what} group {e}"))
    ob = run.obuf.cpu()
    if run.mode == "out":
        o, first, R = run.out.cpu(), int(run.offsets[0]), sum(c.counts)
        assert bool(o[:first].isnan().all()) and bool(o[first + R:].isnan().all()), f"{what}: an unowned row was written"
        ob[:o.shape[0], :c.NO] = gc.CANARY
    else:
        for e, n in enumerate(c.counts):
            assert bool(run.outs[e][min(n, run.cap):].isnan().all()), f"{what}: group {e} wrote past its rows"
            ob[1 + e * (run.cap + 1):1 + e * (run.cap + 1) + run.cap] = gc.CANARY
    assert bool((ob == gc.CANARY).all()), f"{what}: a canary was written"
    return worst


@pytest.mark.parametrize("act", ["none", "swiglu"])
def test_bounded(act):
    """Every (shape, counts) case of the form at every instance and variant, each launched twice."""
    for case in CASES[act]:
        c, qs, ss = build(*case)
        qd, sd = on_device(qs, ss)
        worst = 0.0
        for W, strip in INSTANCES[c.act]:
            for use_a_rows, mode in S.VARIANTS:
                what = f"{S.case_id(case)} W {W} strip {strip} a_rows={int(use_a_rows)} {mode}"
                r1, r2 = S.make_run(c, use_a_rows, mode, DEV), S.make_run(c, use_a_rows, mode, DEV)
                launch(c, qd, sd, r1, W, strip)
                launch(c, qd, sd, r2, W, strip)
                worst = max(worst, verify(c, r1, what))
                assert torch.equal(S.bits(r1), S.bits(r2)), f"{what}: two launches differ"
        print(f"moe_skinny_w8 worst ratio {S.case_id(case)}: {worst:.4g}")


def test_a_row_is_the_same_bits_at_count_1_and_16():
    """Under arbitrary positive scales, no powers of two, with both load policies."""
    for act in ("none", "swiglu"):
        _count_1_and_16(act, (64, 2112))


def _count_1_and_16(act, nk):
    c, qs, ss = build(act, nk, (16,), True)
    qd, sd = on_device(qs, ss)
    x = c.rows.to(DEV)
    off16 = torch.tensor([0, 16], dtype=torch.int32, device=DEV)
    off1 = torch.arange(17, dtype=torch.int32, device=DEV)  # sixteen groups of one row over the same weight
    for W, strip in INSTANCES[act]:
        kw = dict(act=None if act == "none" else act, waves=W, strip=strip)
        for nt in (False, True):
            a = FN(x, qd, sd, off16, out=torch.empty(16, c.NO, dtype=BF, device=DEV), nt=nt, **kw)
            b = FN(x, qd * 16, sd * 16, off1, out=torch.empty(16, c.NO, dtype=BF, device=DEV), nt=nt, **kw)
            assert torch.equal(a, b), (W, strip, nt)
            gk.check_bound(a.cpu(), c.pres[0], c.refs[0], c.aps[0], c.K, "swiglu" if act == "swiglu" else "linear", "nt")


def code_probe(N, K, ks, swiglu):
    """q[n][k] = byte (n K + k) mod 256 (NaN codes -> 0), power-of-two scales, x row m one-hot at
    ks[m]: out[m][n] = float(q[n][ks[m]]) * scale[n] exactly. SwiGLU: column K - 33 holds the gate,
    32 x 2^(block % 3) in the gate rows (zero elsewhere) against x = 1, so silu(gate) = gate exactly
    and out = gate(block) * up: a gate block paired with another block's up shows."""
    b = ((torch.arange(N)[:, None] * K + torch.arange(K)[None, :]) % 256).to(torch.uint8)
    b[(b == 0x7f) | (b == 0xff)] = 0
    s = torch.pow(2.0, (torch.arange(N) % 5 - 3).float())
    x = torch.zeros(len(ks), K, dtype=BF)
    x[torch.arange(len(ks)), torch.tensor(ks)] = 1.0
    if swiglu:
        kg, gate_rows = K - 33, (torch.arange(N) // 16) % 2 == 0
        assert kg not in ks
        b[gate_rows] = 0
        b[:, kg] = 0
        b[gate_rows, kg] = (torch.tensor([32.0, 64.0, 128.0])[(torch.arange(N) // 32) % 3][gate_rows]
                            .to(torch.float8_e4m3fn).view(torch.uint8))
        s[gate_rows] = 1.0
        x[:, kg] = 1.0
    q = b.view(torch.float8_e4m3fn)
    w = q.float() * s[:, None]
    full = x.float() @ w.T
    if not swiglu:
        return x, q, s, full
    v = full.view(len(ks), N // 32, 2, 16)
    want = (v[:, :, 0] * v[:, :, 1]).reshape(len(ks), N // 2)
    shifted = (v[:, :, 0] * torch.roll(v[:, :, 1], -1, 1)).reshape(len(ks), N // 2)
    assert not torch.equal(want, shifted), "an up block shifted by one must fail"
    return x, q, s, want


def test_one_hot_codes():
    N, K = 96, 2112
    nk = -(-K // 128)
    for act, (W, strip) in [(a, i) for a in ("none", "swiglu") for i in INSTANCES[a]]:
        ks = [k for k in range(0, nk * 128, -(-nk // W) * 128)] + list(range(K - 32, K))
        x, q, s, want = code_probe(N, K, ks, act == "swiglu")
        assert torch.equal(want.to(BF).float(), want)
        (qd,), (sd,) = on_device([q], [s])
        off = torch.tensor([0, len(ks)], dtype=torch.int32, device=DEV)
        out = torch.full(want.shape, float("nan"), dtype=BF, device=DEV)
        FN(x.to(DEV), [qd], [sd], off, act=None if act == "none" else act, out=out, waves=W, strip=strip)
        gk.check_exact(out.cpu(), want.to(BF), f"codes {act} W {W} strip {strip}")


def test_graph_replay_follows_device_routing():
    """Captured with one routing, replayed twice without a sync after offsets and a_rows changed on the device."""
    for act, nk, strip in (("none", (48, 160), 16), ("none", (48, 160), 32), ("swiglu", (96, 160), 16)):
        for mode in ("out", "outs"):
            _replay(act, nk, strip, mode)


def _replay(act, nk, strip, mode):
    first, qs, ss = build(act, nk, (1, 0, 16, 7))
    qd, sd = on_device(qs, ss)
    run = S.make_run(first, True, mode, DEV)
    mk = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64, device=DEV)  # noqa: E731
    kw = dict(w_ptrs=mk(qd), s_ptrs=mk(sd), out_ptrs=None if run.outs is None else mk(run.outs))
    launch(first, qd, sd, run, 4, strip, **kw)  # warm-up outside the capture
    eager = S.bits(run).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(first, qd, sd, run, 4, strip, **kw)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(S.bits(run), eager)
    # group 0 loses its row, group 2 keeps its first 9, group 3 all 7: the references are prefixes of the first's
    second, old = first._replace(counts=(0, 0, 9, 7)), run.a_rows.clone()
    run.a_rows[:9], run.a_rows[9:16] = old[1:10], old[17:24]
    run.offsets.copy_(torch.tensor([0, 0, 0, 9, 16], dtype=torch.int32, device=DEV))
    for o in ([run.out] if run.outs is None else run.outs):
        o.fill_(float("nan"))
    torch.cuda.set_sync_debug_mode("error")
    try:
        g.replay()
        g.replay()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    verify(second, run, "replay, second routing")


def test_refused_shapes():
    z = lambda *s, dt=BF: torch.zeros(*s, device=DEV).to(dt)  # noqa: E731
    off = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    f8 = torch.float8_e4m3fn
    for N, K, act, kw in ((16, 48, None, {}), (24, 32, None, {}), (48, 32, "swiglu", {}), (64, 32, "swiglu", dict(strip=32)),
                          (16, 32, None, dict(waves=16))):
        assert ops.grouped_skinny_w8_ok(N, K, act) == (not (K % 32 or N % (32 if act else 16)))
        with pytest.raises(ValueError):
            FN(z(4, K), [z(N, K, dt=f8)], [z(N, dt=torch.float32)], off, act=act, out=z(4, N // 2 if act else N), **kw)
    with pytest.raises(ValueError):  # bf16 weights
        FN(z(4, 32), [z(16, 32)], [z(16, dt=torch.float32)], off, out=z(4, 16))
    e = ops.ext()  # the launcher's rule and its mirror
    for N, K, a in ((4096, 14336, 0), (64, 2112, 0), (28672, 4096, ops.SWIGLU)):
        assert (ops.grouped_skinny_w8_waves(N, K, a), ops.grouped_skinny_w8_strip(N, K, a), ops.grouped_skinny_w8_nt(N, K, a)) \
            == (e.gemm_grouped_skinny_w8_waves(N, K, a), e.gemm_grouped_skinny_w8_strip(N, K, a), e.gemm_grouped_skinny_w8_nt(N, K, a))
