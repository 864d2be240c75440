"""The e4m3 prompt-chunk attention (csrc/kernels/attn_chunk_fp8.hip): ``kv_append`` with scales, then
``attention_chunk(..., native=True)`` — against the float64 oracle over the dequantised cache per
(row, head), selector cases bit for bit, NaN-poisoned stale rows and scales, a captured launch that
follows ``pos``, a strided ``out``, and the refusals. The cases are those of attn_chunk_cases.py
(rep 1 and 2) plus rep 4 and 8 at T = 17 (a last tile of one token; three tiles at rep 8) and
T = 200 (several tiles, keys crossing whole stages), all on C = 640. A test walks its cases in a
loop (the whole file is a few seconds), so the suite grows by four tests, not by a hundred.

Tolerance: attn_chunk_cases.ROW_TOL (2^-6), by that file's rule. Worst row error measured on an
MI355X over the random, packed and poison cases here: 4.692e-3 in f8native_d64_h8x1_t200_edge
(3 x 4.692e-3 = 0.01408 < 2^-6 = 0.015625; the rep 1 and 2 cases stay at attn_chunk_cases' 4.483e-3).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attn_checks as K  # noqa: E402
import attn_chunk_cases as CC  # noqa: E402
import attn_decode_cases as C  # noqa: E402
import attn_decode_fp8_cases as F  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -55.0

# rep 4 and 8: (D, n_head, n_kv_head, T, pos set)
PACKED = [(D, nh, nkv, T, p) for D in (64, 128) for nh, nkv in ((8, 2), (8, 1)) for T, p in ((17, "edge"), (200, "edge"),
                                                                                             (200, "full"))]
_cases = {f"f8native_d{D}_h{nh}x{nkv}_t{T}_{p}": (D, nh, nkv, T, p) for D, nh, nkv, T, p in PACKED}
_built = {}


def _case(name):
    if name not in _cases:
        return CC.case8(name)
    if name not in _built:
        _built[name] = F._build_random(*_cases[name], name=name)
    return _built[name]


def _step(c8, out=None, layout=0):
    qkv = c8.k_new._base.to(DEV)
    nq, nk = c8.nh * c8.D, c8.nkv * c8.D
    q, k, v = qkv[:, :nq], qkv[:, nq:nq + nk], qkv[:, nq + nk:]
    kq, vq, ks, vs = (t.to(DEV) for t in (c8.k_cache, c8.v_cache, c8.k_scale, c8.v_scale))
    pos = torch.tensor(c8.pos, dtype=torch.int32, device=DEV)
    ops.kv_append(k, v, kq, vq, pos, c8.T, ks, vs)
    return ops.attention_chunk(q, kq, vq, pos, c8.T, c8.nh, c8.nkv, c8.D, out=out, k_scale=ks, v_scale=vs, native=True,
                               layout=layout)


def test_against_oracle():
    """Every random case of attn_chunk_cases (rep 1 and 2), the packed cases (rep 4 and 8) and the
    poison cases, one after the other: a failure names its case. Prints the worst row error."""
    worst, where = 0.0, None
    for name in CC.RANDOM_CASES8 + tuple(_cases) + CC.POISON_CASES8:
        c8 = _case(name)
        err = CC.check(_step(c8), c8.eq, CC.ROW_TOL, name)
        if err > worst:
            worst, where = err, name
    print(f"largest row error: {worst:.4g} in {where}")


def test_every_layout_and_the_refusals():
    """Each (NW query tiles, KS key groups) layout the launcher can take: an odd tile count leaves
    the last workgroup of two tiles with one (17 tokens in tiles of 8), and a tile stages keys past
    its own. Then what the entry refuses."""
    for name in ("f8native_d64_h8x1_t17_edge", "f8native_d128_h8x2_t200_edge", "f8chunk_d128_h2x2_t40_full",
                 "f8chunkpoison_d64_t40_ragged_v1_upto20"):
        c8 = _case(name)
        for layout in ops.CHUNK_FP8_LAYOUTS:
            CC.check(_step(c8, layout=layout), c8.eq, CC.ROW_TOL, f"{name} layout {layout}")
    pos = torch.zeros(CC.B, dtype=torch.int32, device=DEV)
    q = torch.zeros(CC.B * 4, 256, dtype=torch.bfloat16, device=DEV)
    k16 = torch.zeros(CC.B, CC.CAP, 128, dtype=torch.bfloat16, device=DEV)
    k8 = torch.zeros(CC.B, CC.CAP, 128, dtype=torch.uint8, device=DEV)
    ones = torch.ones(CC.B, 2, CC.CAP, device=DEV)
    with pytest.raises(RuntimeError, match="fp8"):
        ops.attention_chunk(q, k16, k16, pos, 4, 4, 2, 64, native=True)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.attention_chunk(q, k8, k8, pos, 4, 4, 2, 64, k_scale=ones, v_scale=ones, workspace=(k16, k16), native=True)
    with pytest.raises(RuntimeError, match="layout"):
        ops.attention_chunk(q, k8, k8, pos, 4, 4, 2, 64, k_scale=ones, v_scale=ones, native=True, layout=13)
    k96 = torch.zeros(CC.B, CC.CAP, 192, dtype=torch.uint8, device=DEV)
    why = ops.attention_chunk_native_refusal(4, 4, 2, 96)
    with pytest.raises(RuntimeError) as e:
        ops.attention_chunk(q, k96, k96, pos, 4, 4, 2, 96, k_scale=ones, v_scale=ones, native=True)
    assert why and why in str(e.value)


def test_selector():
    """The output is the selected key's dequantised value row, bit for bit (every map, both D and
    both position sets of attn_decode_cases, T = 40)."""
    for m in C.SELECTOR_MAPS:
        for D in (64, 128):
            for p in C.SELECTOR_POS:
                c = F._build_selector(m, D, 40, p)
                K.check_exact(_step(c), c.want, c.name, c.T)


def test_captured_launch_follows_pos_into_a_strided_out():
    """One captured launch, replayed after q, the caches, the scales and pos changed, equals the
    eager result at the new positions; its ``out`` is a view inside a sentinel-filled buffer, and
    nothing outside the view is written."""
    a, b = CC.case8("f8chunk_d128_h4x2_t40_edge"), CC.case8("f8chunk_d128_h4x2_t40_empty")
    eager = [_step(c) for c in (a, b)]
    bufs = [t.to(DEV) for t in (a.k_new._base, *F._appended8(a))]
    qkv, kq, vq, ks, vs = bufs
    pos = torch.tensor(a.pos, dtype=torch.int32, device=DEV)
    rows, cols, gr, gc = CC.B * a.T, a.nh * a.D, 3, 32
    buf = torch.full((rows + 2 * gr, cols + 2 * gc), SENTINEL, dtype=torch.bfloat16, device=DEV)
    o = buf[gr:gr + rows, gc:gc + cols]
    run = lambda: ops.attention_chunk(qkv[:, :a.nh * a.D], kq, vq, pos, a.T, a.nh, a.nkv, a.D, out=o, k_scale=ks,  # noqa: E731
                                      v_scale=vs, native=True)
    got = run()  # (warm-up outside the capture)
    assert got.data_ptr() == o.data_ptr() and got.stride() == o.stride()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    g.replay()
    assert torch.equal(o, eager[0])
    for dst, src in zip(bufs, (b.k_new._base, *F._appended8(b))):
        dst.copy_(src)
    pos.copy_(torch.tensor(b.pos, dtype=torch.int32))
    for _ in range(2):
        g.replay()
        assert torch.equal(o, eager[1])
    guard = buf.cpu()
    guard[gr:gr + rows, gc:gc + cols] = SENTINEL
    assert (guard == SENTINEL).all()
