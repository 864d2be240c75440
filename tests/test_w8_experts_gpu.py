"""The grouped fp8-weight GEMM (csrc/kernels/gemm_w8_grouped.hip) and the fp8-experts executor
mode on the GPU.

Kernel reference: ``(x.float()[rows] @ q.float().T) * scale`` per group in fp32 — the same e4m3
values the kernel multiplies, so what remains is bf16 output rounding (2^-9 relative) plus fp32
summation order: far inside the 2e-2 of ``_close`` (the measure of tests/test_w8_gpu.py)."""
import pytest
import torch

from distributed_llm_scheduler_amd import ops
from distributed_llm_scheduler_amd.models import reference
from distributed_llm_scheduler_amd.parallel import executor as exm
from distributed_llm_scheduler_amd.parallel import runtime
from distributed_llm_scheduler_amd.parallel.executor import synthetic_tokens

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-2
WD = "fp8-experts"
SENTINEL = 1000.0  # a bf16 value


def _configs():
    return list(range(ops.w8_grouped_configs()))


def _close(a, b, tol=TOL):
    err = (a.float() - b.float()).abs().max().item()
    ref = b.float().abs().max().item() + 1e-6
    assert err <= tol * ref, f"max abs err {err:.4g} vs ref max {ref:.4g} (rel tol {tol})"


def _rand(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(torch.bfloat16).to(DEV)


def _weight(N, K, seed=0):
    """q e4m3 [N, K] (quantised N(0, 0.02) weights) and arbitrary fp32 scales in [1e-3, 10] (a
    checkpoint quantised elsewhere): the weight side of tests/test_w8_gpu.py::_problem."""
    g = torch.Generator(device="cpu").manual_seed(100 + seed)
    q, _ = ops.quantize_fp8((0.02 * torch.randn(N, K, generator=g)).to(torch.bfloat16))
    scale = torch.exp(torch.empty(N).uniform_(-6.9077, 2.3026, generator=g)).clamp_(1e-3, 10.0)
    return q.to(DEV), scale.to(DEV)


def _twice(T, seed):
    """A random order of the token rows 0..T-1 in which every token appears twice (top-2)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.arange(T).repeat(2)[torch.randperm(2 * T, generator=g)].to(torch.int32).to(DEV)


class _Problem:
    """G groups over ``counts`` rows; natural weights, the tensors the kernel takes (gate/up
    interleaved for SwiGLU) and the fp32 reference of every sorted row."""

    def __init__(self, counts, N, K, swiglu, gather, seed=0, weights_of=None):
        G, R = len(counts), sum(counts)
        self.counts, self.R, self.swiglu = counts, R, swiglu
        self.NO = N // 2 if swiglu else N
        self.act = "swiglu" if swiglu else None
        weights_of = weights_of or list(range(G))
        nat = {w: _weight(N, K, seed=seed + 10 * w) for w in set(weights_of)}
        if gather:
            assert R % 2 == 0
            self.x, self.a_rows = _rand(R // 2, K, seed=seed + 1), _twice(R // 2, seed + 2)
            xs = self.x.float()[self.a_rows.long()]
        else:
            self.x, self.a_rows = _rand(R, K, seed=seed + 1), None
            xs = self.x.float()
        il = (lambda t: ops.interleave_gate_up(t)) if swiglu else (lambda t: t)
        given = {w: (il(q.view(torch.uint8)).view(torch.float8_e4m3fn), il(s)) for w, (q, s) in nat.items()}
        self.qs = [given[w][0] for w in weights_of]
        self.ss = [given[w][1] for w in weights_of]
        self.off = torch.tensor([0] + torch.tensor(counts).cumsum(0).tolist(), dtype=torch.int32, device=DEV)
        ref = torch.zeros(R, self.NO, device=DEV)
        lo = 0
        for g, c in enumerate(counts):
            q, s = nat[weights_of[g]]
            y = (xs[lo:lo + c] @ q.float().t()) * s
            ref[lo:lo + c] = torch.nn.functional.silu(y[:, :N // 2]) * y[:, N // 2:] if swiglu else y
            lo += c
        self.ref = ref

    def run(self, cfg, out=None, **kw):
        out = torch.full((self.R, self.NO), SENTINEL, dtype=torch.bfloat16, device=DEV) if out is None else out
        ops.gemm_grouped_w8(self.x, self.qs, self.ss, self.off, act=self.act, out=out, a_rows=self.a_rows,
                            config=cfg, **kw)
        return out


def test_config_table():
    hs = [ops.w8_grouped_tile_rows(c) for c in _configs()]
    assert len(hs) >= 2 and min(hs) <= 32 and max(hs) >= 128 and all(h % 16 == 0 for h in hs)


@pytest.mark.parametrize("cfg", range(5))
def test_row_counts_every_config(cfg):
    """Zero rows, one row, one short of a tile, a tile, one past it, more than two tiles — in
    both orders; column and K tails; with and without the row gather."""
    assert ops.w8_grouped_configs() == 5  # (the parametrisation above covers every config)
    h = ops.w8_grouped_tile_rows(cfg)
    counts = [0, 1, h - 1, h, h + 1, 2 * h + 3]
    for N, K, sw in [(136, 208, False), (256, 256, False), (512, 256, True)]:
        for cs in (counts, counts[::-1]):
            for gather in (False, True):
                pb = _Problem(cs, N, K, sw, gather, seed=cfg)
                _close(pb.run(cfg), pb.ref)


def test_all_codes_bit_exact():
    """x = identity rows reached through a_rows: a group's output rows are columns of its
    dequantised weight, bit for bit — every finite e4m3 code through the conversion, two groups
    with different weights, every config (the construction of tests/test_w8_gpu.py)."""
    K, N = 256, 272
    codes = torch.arange(256, dtype=torch.uint8)
    codes = codes[(codes & 0x7F) != 0x7F]
    n, k = torch.arange(N)[:, None], torch.arange(K)[None, :]
    qs, ss, wants = [], [], []
    g = torch.Generator(device="cpu").manual_seed(3)
    a_rows = torch.cat([torch.randperm(K, generator=g), torch.randperm(K, generator=g)]).to(torch.int32).to(DEV)
    for grp in range(2):
        qb = codes[(3 * n + k + 57 * grp) % 254]  # asymmetric; every row holds every code
        q = qb.contiguous().view(torch.float8_e4m3fn).to(DEV)
        scale = (2.0 ** ((torch.arange(N) % 13) - 8 + grp).float()).to(DEV)
        want = ops.dequantize_fp8(q, scale).t().contiguous()  # [K][N]: row = token (k index)
        assert torch.equal(want.float(), (q.float() * scale[:, None]).t())  # exactly bf16 values
        qs.append(q)
        ss.append(scale)
        wants.append(want[a_rows[grp * K:(grp + 1) * K].long()])
    want = torch.cat(wants)
    x = torch.eye(K, dtype=torch.bfloat16, device=DEV)
    off = torch.tensor([0, K, 2 * K], dtype=torch.int32, device=DEV)

    def bits(t):  # -0 -> +0: an accumulator that starts at +0 cannot return -0
        return torch.where(t == 0, torch.zeros_like(t), t).view(torch.int16)

    assert (want == 0).sum().item() >= 4 * K
    for cfg in [None] + _configs():
        y = torch.full((2 * K, N), SENTINEL, dtype=torch.bfloat16, device=DEV)
        ops.gemm_grouped_w8(x, qs, ss, off, out=y, a_rows=a_rows, config=cfg)
        assert torch.equal(bits(y), bits(want)), f"config {cfg}"


@pytest.mark.parametrize("N,K,sw", [(256, 4096, True), (128, 14336, False)])
def test_full_width_k_on_a_narrow_column_slice(N, K, sw):
    """Mixtral's K of gate/up (4096) and down (14336) on a few columns, counts around the
    tile heights and a real step's spread."""
    pb = _Problem([0, 1, 97, 128, 149, 192, 193, 264], N, K, sw, gather=sw, seed=5)
    for cfg in [None] + _configs():
        _close(pb.run(cfg), pb.ref)


@pytest.mark.parametrize("col0", [8, 3])
def test_no_stray_writes_out_view(col0):
    """``out`` is a view inside a sentinel-filled buffer (8-byte aligned and unaligned: vector
    and scalar stores), row and column tails; rows of ``out`` that belong to no group (before
    offsets[0], after offsets[G]) stay untouched."""
    for N, K, sw in [(136, 208, False), (96, 64, True)]:
        pb = _Problem([5, 0, 37, 70], N, K, sw, gather=False, seed=7)
        lead, trail = 3, 4
        off = pb.off + lead
        x = torch.cat([_rand(lead, K, seed=1), pb.x, _rand(trail, K, seed=2)])
        R = x.shape[0]
        for cfg in [None] + _configs():
            big = torch.full((R + 5, pb.NO + 24), SENTINEL, dtype=torch.bfloat16, device=DEV)
            out = big[2:2 + R, col0:col0 + pb.NO]
            ops.gemm_grouped_w8(x, pb.qs, pb.ss, off, act=pb.act, out=out, config=cfg)
            _close(out[lead:lead + pb.R], pb.ref)
            mask = torch.ones_like(big, dtype=torch.bool)
            mask[2 + lead:2 + lead + pb.R, col0:col0 + pb.NO] = False
            assert (big[mask] == SENTINEL).all(), f"config {cfg}"


def test_no_stray_writes_compact_outputs():
    """Compact ``outs[g]`` with fewer rows than the largest group's count: rows past
    min(count, cap) unwritten, the buffer behind each output untouched."""
    counts, cap = [5, 0, 37, 70], 40
    for N, K, sw in [(136, 208, False), (96, 64, True)]:
        pb = _Problem(counts, N, K, sw, gather=True, seed=9)
        for cfg in [None] + _configs():
            big = torch.full((len(counts), cap + 3, pb.NO), SENTINEL, dtype=torch.bfloat16, device=DEV)
            outs = [big[g, :cap] for g in range(len(counts))]
            ops.gemm_grouped_w8(pb.x, pb.qs, pb.ss, pb.off, act=pb.act, outs=outs, a_rows=pb.a_rows, config=cfg)
            lo = 0
            for g, c in enumerate(counts):
                n = min(c, cap)
                if n:
                    _close(outs[g][:n], pb.ref[lo:lo + n])
                assert (big[g, n:] == SENTINEL).all(), f"config {cfg} group {g}"
                lo += c


def test_shared_weights():
    """4 groups over 2 distinct weights (a cross-request expert batch: same-weight groups
    adjacent) equal the per-group reference."""
    for sw, N in [(False, 136), (True, 256)]:
        pb = _Problem([33, 70, 1, 130], N, 208, sw, gather=True, seed=11, weights_of=[0, 0, 1, 1])
        assert pb.qs[0].data_ptr() == pb.qs[1].data_ptr() != pb.qs[2].data_ptr()
        for cfg in [None] + _configs():
            _close(pb.run(cfg, shared_weights=True), pb.ref)
            assert torch.equal(pb.run(cfg, shared_weights=True), pb.run(cfg))


def test_two_runs_are_bitwise_equal():
    pb = _Problem([0, 1, 97, 128, 149, 192, 193, 264], 256, 1024, True, gather=True, seed=13)
    for cfg in [None] + _configs():
        assert torch.equal(pb.run(cfg), pb.run(cfg)), f"config {cfg}"


def test_wrong_operands_are_refused():
    pb = _Problem([4, 4], 64, 64, False, gather=False)
    out = torch.empty(8, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(TypeError):
        ops.gemm_grouped_w8(pb.x, [q.float().to(torch.bfloat16) for q in pb.qs], pb.ss, pb.off, out=out)
    with pytest.raises(RuntimeError, match="K % 16"):
        ops.gemm_grouped_w8(pb.x[:, :40].contiguous(), [q[:, :40].contiguous() for q in pb.qs], pb.ss, pb.off, out=out)
    with pytest.raises(RuntimeError, match="config"):
        ops.gemm_grouped_w8(pb.x, pb.qs, pb.ss, pb.off, out=out, config=ops.w8_grouped_configs())


def test_expert_layer_chain_with_device_routing():
    """route -> gate/up (rows gathered by the device's src_rows, SwiGLU) -> down (compact
    outputs) -> gather-combine, against fp32 using the idx / gate tensors the device produced:
    no row is exempt."""
    M, E, H, F, topk = 128, 4, 256, 256, 2
    x = _rand(M, H, seed=21)
    logits = _rand(M, E, seed=22)
    idx, gate, src, slot, off = ops.moe_route(logits, topk, E)
    w13 = [_weight(2 * F, H, seed=30 + e) for e in range(E)]
    w2 = [_weight(H, F, seed=40 + e) for e in range(E)]
    q13 = [ops.interleave_gate_up(q.view(torch.uint8)).view(torch.float8_e4m3fn) for q, _ in w13]
    s13 = [ops.interleave_gate_up(s) for _, s in w13]
    hbuf = torch.zeros(M * topk, F, dtype=torch.bfloat16, device=DEV)
    outs = [torch.zeros(M, H, dtype=torch.bfloat16, device=DEV) for _ in range(E)]
    y = torch.zeros(M, H, dtype=torch.bfloat16, device=DEV)
    ops.gemm_grouped_w8(x, q13, s13, off, act="swiglu", out=hbuf, a_rows=src, rows_hint=M * topk // E)
    ops.gemm_grouped_w8(hbuf, [q for q, _ in w2], [s for _, s in w2], off, outs=outs, rows_hint=M * topk // E)
    ops.moe_gather_combine(outs, idx, slot, off, gate, out=y)
    torch.cuda.synchronize()
    want = torch.zeros(M, H, device=DEV)
    xf = x.float()
    for e in range(E):
        (q1, s1), (q2, s2) = w13[e], w2[e]
        gu = (xf @ q1.float().t()) * s1
        h = (torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]).to(torch.bfloat16).float()  # hbuf is bf16
        ye = (h @ q2.float().t()) * s2
        for j in range(topk):
            sel = idx[:, j].long() == e
            want[sel] += gate[sel, j, None].float() * ye[sel]
    assert int(off[-1]) == M * topk
    _close(y, want)


# ------------------------------------------------------------------------------ executor
def _check(p, ex, store, tol, rid=""):
    """The measure of tests/test_executor_gpu.py::_check."""
    out = ex.output(f"{rid}output_projection").float().cpu()
    B, S = out.shape[0], out.shape[1]
    tok = synthetic_tokens(f"{rid}@tokens", B * S, p.cfg.vocab_size).view(B, S)
    margins = []
    ref = reference.forward(p.cfg, store, tok, router_margins=margins)
    scale = ref.abs().max().item()
    assert margins
    row_err = (out - ref).abs().amax(-1)
    risky = torch.stack([m.abs() < 0.05 for m in margins]).any(0)
    bad = row_err > tol * scale
    assert bad.float().mean().item() < 0.1, (int(bad.sum()), int(risky.sum()), row_err.max().item(), scale)
    assert not (bad & ~risky).any(), (int((bad & ~risky).sum()), int(bad.sum()), row_err[~risky].max().item(), scale)


@pytest.mark.parametrize("graph", [False, True])
def test_fp8_experts_dag_on_gpu_matches_reference(graph):
    p = runtime.plan("mini-mixtral", world=1, seq=64, batch=2, weight_dtype=WD)
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, torch.device("cuda:0"), store, use_graph=graph)
    assert len(ex._moe_batch) == p.cfg.n_layer  # the grouped launch pair per layer
    ex.step()
    if graph:
        assert ex.capture()
        ex.step()
    torch.cuda.synchronize()
    name = next(s.name for g in p.groups.values() for s in g.tensors if s.quant)
    assert ex._w(name).dtype == torch.float8_e4m3fn and ex._w("layers.0.moe.gate").dtype == torch.bfloat16
    _check(p, ex, store, 0.03)


def test_fp8_experts_memory_capped_reloads_on_gpu():
    full = runtime.plan("mini-mixtral", world=1, seq=64, batch=2, weight_dtype=WD)
    need = sum(runtime.make_store(full).nbytes(g) for g in full.groups) / 1e9
    p = runtime.plan("mini-mixtral", world=1, seq=64, batch=2, cap_gb=need * 0.6, weight_dtype=WD)
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, torch.device("cuda:0"), store, use_graph=False)
    for _ in range(2):
        st = ex.step()
    assert st.param_fills > 0
    torch.cuda.synchronize()
    _check(p, ex, store, 0.03)


def test_fp8_experts_cross_request_batch_on_gpu(monkeypatch):
    """Two requests on one GPU: each layer's expert nodes of both requests run as one grouped
    launch pair with shared weights (_run_moe_xbatch)."""
    monkeypatch.setattr(exm, "MOE_BATCH", False)  # the per-request batch would take the nodes first
    p = runtime.plan("mini-mixtral", world=1, seq=64, batch=2, replicas=2, weight_dtype=WD)
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, torch.device("cuda:0"), store, use_graph=False)
    assert len(ex._xbatch) == p.cfg.n_layer and not ex._moe_batch
    ex.step()
    torch.cuda.synchronize()
    for rid in ("r0/", "r1/"):
        _check(p, ex, store, 0.03, rid)


def test_fp8_experts_single_expert_nodes_on_gpu(monkeypatch):
    """With the batches switched off (DLS_MOE_BATCH=0) every expert node runs alone
    (_moe_expert: a one-group launch pair)."""
    monkeypatch.setattr(exm, "MOE_BATCH", False)
    monkeypatch.setattr(exm, "MOE_XBATCH", False)
    p = runtime.plan("mini-mixtral", world=1, seq=64, batch=2, weight_dtype=WD)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, torch.device("cuda:0"), store, use_graph=False)
    assert not ex._moe_batch and not ex._xbatch
    ex.step()
    torch.cuda.synchronize()
    _check(p, ex, store, 0.03)
