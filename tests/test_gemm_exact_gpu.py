"""The LDS-DMA bf16 GEMM (csrc/kernels/gemm_glds_impl.h) and the register-staged one, every tile
config through every launch form, held to bit-exact probes: integer, power-of-two scaled and
selector inputs whose output is the same in every summation order (gemm_cases.py), compared with
``torch.equal`` against a float64 reference (gemm_checks.py) — plain, NaN-padded strided operands
inside a canary, split-K with the in-launch combine and with the reduce kernels, row ranges,
compact outputs, grouped and persistent launches. Epilogues that round (GELU, SiLU, SwiGLU, RoPE,
folded and post norms) are held to a bound per element. The last tests hold the split-K ticket
pool to the tile grid of the config that runs. test_gemm_ref_cpu.py shows that these checks
reject mutants of an honest kernel.

Shapes per config: M = bm + 5 (two row tiles, the second with five rows), N = bn + 24 (a partial
column tile of whole 16-byte segments) or bn + 2 (unaligned rows: scalar stores), K = 12 K steps.
"""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gemm_cases as C  # noqa: E402
import gemm_checks as K  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
ACT = {None: 0, "gelu": 1, "silu": 2, "relu": 3, "swiglu": 4}
SENTINEL = 5.0
EPIS = {e.name: e for e in (C.EPI_NONE, C.EPI_FULL)}


@functools.lru_cache(maxsize=None)
def _dev(kind, M, N, Kk):
    p = C.probe(kind, M, N, Kk)
    return C.Probe(p.kind, *(None if t is None else t.to(DEV) for t in (p.x, p.w, p.bias, p.res)))


@functools.lru_cache(maxsize=None)
def _want(kind, M, N, Kk, epi):
    return K.expected_exact(C.probe(kind, M, N, Kk), EPIS[epi])


def _gemm(p, epi, config, splitk=1, out=None, a=None, w=None, res=None, **kw):
    bias, r, act, alpha = C.operands(p, epi)
    if r is not None and res is not None:
        r = res
    return ops.ext().gemm(p.x if a is None else a, p.w if w is None else w, bias, r, ACT[act], alpha, out, config,
                          splitk, **kw)


def _sentinel(M, N):
    return torch.full((M, N), SENTINEL, dtype=BF, device=DEV)


def test_tile_accessors_match_the_table():
    e = ops.ext()
    assert e.gemm_glds_num_configs() == len(C.TILES)
    for c, (bm, bn, ks) in C.TILES.items():
        assert tuple(e.gemm_glds_tile(c)) == (bm, bn) and e.gemm_glds_kstep(c) == ks, c
        assert tuple(e.gemm_glds_tile(c + e.PERSIST)) == (bm, bn), c


# ---------------------------------------------------------------------------------------------
# Plain launches

@pytest.mark.parametrize("kind", list(C.PROBES))
@pytest.mark.parametrize("epi", list(EPIS))
@pytest.mark.parametrize("n_kind", C.N_KINDS)
@pytest.mark.parametrize("config", C.ALL_CONFIGS)
def test_plain_exact(config, n_kind, epi, kind):
    M, N, Kk = C.shape(config, n_kind)
    out = _sentinel(M, N)
    _gemm(_dev(kind, M, N, Kk), EPIS[epi], config, out=out)
    K.check_exact(out, _want(kind, M, N, Kk, epi), f"config {config} {kind} {epi} {(M, N, Kk)}")


@pytest.mark.parametrize("n_kind", C.N_KINDS)
@pytest.mark.parametrize("config", C.ALL_CONFIGS)
def test_poisoned_strided_operands(config, n_kind):
    """A, W, the residual and the output as views into NaN-padded buffers (lda = K + 8,
    ldw = K + 16, three extra rows): the result equals the contiguous run bit for bit, and
    nothing around the output or in the residual buffer changed."""
    M, N, Kk = C.shape(config, n_kind)
    p, d = C.integer_probe(M, N, Kk), _dev("integer", M, N, Kk)
    pd = C.padded(p.x, p.w, p.res, DEV)
    K.check_poison_placement(pd, M, N, Kk)
    _gemm(d, C.EPI_FULL, config, out=pd.out, a=pd.a, w=pd.w, res=pd.res)
    plain = _sentinel(M, N)
    _gemm(d, C.EPI_FULL, config, out=plain)
    what = f"config {config} poisoned {(M, N, Kk)}"
    assert torch.equal(pd.out, plain), f"{what}: differs from the contiguous run"
    K.check_exact(pd.out.contiguous(), _want("integer", M, N, Kk, C.EPI_FULL.name), what)
    K.check_canary(pd, M, N, p.res, what)


# ---------------------------------------------------------------------------------------------
# Split-K

def _splitk_path(config, splitk):
    """The tile size alone decides: the last arriver of a tile reads (splitk - 1) fp32 slabs of
    it, in the launch while they stay within 64 KiB, else the reduce kernels run."""
    bm, bn, _ = C.tile(config)
    return "combine" if (splitk - 1) * bm * bn * 4 <= 64 * 1024 else "reduce"


SPLITK_CASES = [pytest.param(c, s, _splitk_path(c, s), id=f"{c}-sk{s}-{_splitk_path(c, s)}")
                for c in C.GLDS for s in (2, 3, 4)]


@pytest.mark.parametrize("config,splitk,path", SPLITK_CASES)
def test_splitk_exact_and_repeatable(config, splitk, path):
    M, N, Kk = C.shape(config, "seg")
    d = _dev("integer", M, N, Kk)
    o1, o2 = _sentinel(M, N), _sentinel(M, N)
    _gemm(d, C.EPI_FULL, config, splitk, out=o1)
    _gemm(d, C.EPI_FULL, config, splitk, out=o2)
    assert torch.equal(o1, o2), f"config {config} split-K {splitk} ({path}): two runs differ"
    K.check_exact(o1, _want("integer", M, N, Kk, C.EPI_FULL.name), f"config {config} split-K {splitk} ({path})")


def test_splitk_cases_reach_both_paths():
    paths = {(c, s): _splitk_path(c, s) for c in C.GLDS for s in (2, 3, 4)}
    assert paths[(24, 4)] == "combine" and paths[(3, 4)] == "combine" and paths[(0, 2)] == "reduce"
    assert paths[(1, 2)] == "combine" and paths[(1, 3)] == "reduce"  # 128 x 128: 64 KiB per slab
    assert sum(v == "combine" for v in paths.values()) >= 40 and sum(v == "reduce" for v in paths.values()) >= 40


# ---------------------------------------------------------------------------------------------
# Row ranges, compact outputs, grouped and persistent launches

@pytest.mark.parametrize("config", C.GLDS)
def test_row_range_and_compact(config):
    M, N, Kk = C.shape(config, "seg")
    d = _dev("integer", M, N, Kk)
    want = _want("integer", M, N, Kk, C.EPI_FULL.name)
    r0, r1 = 3, M - 2
    rows = torch.tensor([r0, r1], dtype=torch.int32, device=DEV)
    out = _sentinel(M, N)
    _gemm(d, C.EPI_FULL, config, out=out, rows=rows)
    o = out.cpu()
    assert bool((o[:r0] == SENTINEL).all()) and bool((o[r1:] == SENTINEL).all()), "rows outside the range were written"
    K.check_exact(o[r0:r1].contiguous(), want[r0:r1].contiguous(), f"config {config} rows [{r0}, {r1})")
    # the empty range writes nothing
    out = _sentinel(M, N)
    _gemm(d, C.EPI_FULL, config, out=out, rows=torch.tensor([5, 5], dtype=torch.int32, device=DEV))
    assert bool((out == SENTINEL).all()), "an empty row range wrote output"
    # compact: the range lands at rows 0.. of an output with spare rows, and of one that is too short
    nores = C.Epilogue("bias_relu_half", True, False, "relu", 0.5)
    pre, _ = K.ref64(*C.integer_probe(M, N, Kk)[1:4], "relu", None, 0.5)
    cw = pre.to(BF)
    for cap in (r1 - r0 + 2, r1 - r0 - 2):
        out = _sentinel(cap, N)
        _gemm(d, nores, config, out=out, rows=rows, compact_rows=True)
        n = min(cap, r1 - r0)
        o = out.cpu()
        assert bool((o[n:] == SENTINEL).all()), "compact rows past the range were written"
        K.check_exact(o[:n].contiguous(), cw[r0:r0 + n].contiguous(), f"config {config} compact, {cap} rows")


@functools.lru_cache(maxsize=None)
def _grouped_case(bm, N, Kk):
    counts = [bm + 5, 0, 7]
    R = sum(counts)
    p = C.integer_probe(R, N, Kk)
    ws = [p.w, C._ternary(N, Kk, 7400 + N + Kk), C._ternary(N, Kk, 7401 + N + Kk)]
    want = torch.full((R, N), SENTINEL, dtype=BF)
    off = [0, counts[0], counts[0], R]
    for g in range(3):
        if off[g + 1] > off[g]:
            want[off[g]:off[g + 1]] = K.ref64(p.x[off[g]:off[g + 1]], ws[g], None, "relu")[1].to(BF)
    return p.x.to(DEV), [w.to(DEV) for w in ws], off, want


@pytest.mark.parametrize("config", C.GLDS)
def test_grouped_exact(config):
    """Three groups of bm + 5, 0 and 7 rows, each with its own weight, into a sentinel-filled
    output: the empty group's tiles exit, every row of the others is exact."""
    bm, bn, ks = C.tile(config)
    x, ws, off, want = _grouped_case(bm, bn + 24, 12 * ks)
    offd = torch.tensor(off, dtype=torch.int32, device=DEV)
    wp = torch.tensor([w.data_ptr() for w in ws], dtype=torch.int64, device=DEV)
    out = _sentinel(*want.shape)
    ops.ext().gemm_grouped(x, ws, wp, offd, ACT["relu"], out, [], None, config)
    K.check_exact(out, want, f"config {config} grouped {off}")


# resident workgroups per CU, bounded by the 160 KiB of LDS (the stage rings of the config take
# 144, 64, 160, 64 and 128 KiB): registers can only lower it, and more tiles than needed still
# make every workgroup walk several
PERSIST_WG_PER_CU = {0: 1, 3: 2, 14: 1, 17: 2, 34: 1}


@pytest.mark.parametrize("config", sorted(PERSIST_WG_PER_CU))
def test_persistent_more_tiles_than_workgroups(config):
    bm, bn, ks = C.tile(config)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    col_tiles = -(-int(2.1 * cus * PERSIST_WG_PER_CU[config] + 1) // 2)
    M, N, Kk = bm + 5, (col_tiles - 1) * bn + 24, 4 * ks
    assert 2 * col_tiles >= 2.1 * cus * PERSIST_WG_PER_CU[config]
    epi = C.Epilogue("bias_res", True, True, None, 1.0)
    p = C.integer_probe(M, N, Kk)
    K.check_probe_preconditions(p, epi)
    want = K.expected_exact(p, epi)
    out = _sentinel(M, N)
    _gemm(_dev("integer", M, N, Kk), epi, config + ops.ext().PERSIST, out=out)
    K.check_exact(out, want, f"config {config} persistent, {2 * col_tiles} tiles")


# ---------------------------------------------------------------------------------------------
# Register-staged ids

def test_config_ids_100_to_103_are_the_register_staged_kernel():
    """Ids 100..103 also read as "persistent 36..39": they run the register-staged kernel — which
    alone takes K % 64 != 0, and draws no split-K tickets — and larger ids are refused."""
    e = ops.ext()
    for config in sorted(C.REGSTAGE):
        bm, bn, _ = C.tile(config)
        M, N, Kk = bm + 5, bn + 2, 72
        p = C.integer_probe(M, N, Kk)
        K.check_probe_preconditions(p, C.EPI_FULL)
        out = _sentinel(M, N)
        _gemm(_dev("integer", M, N, Kk), C.EPI_FULL, config, out=out)
        K.check_exact(out, K.expected_exact(p, C.EPI_FULL), f"config {config} K = 72")
        M, N, Kk = C.shape(config, "seg")
        before = e._split_k_cursor(0)
        _gemm(_dev("integer", M, N, Kk), C.EPI_FULL, config, 2, out=_sentinel(M, N))
        assert e._split_k_cursor(0) == before, f"config {config} drew split-K tickets: not the register-staged kernel"
    d = _dev("integer", *C.shape(3, "seg"))
    for config in (104, 111, 128, 1000):
        with pytest.raises(RuntimeError, match="unknown GEMM config"):
            e.gemm(d.x, d.w, None, None, 0, 1.0, None, config, 1)


# ---------------------------------------------------------------------------------------------
# Epilogues that round: the per-element bound

BOUNDED_CONFIGS = [3, 0, 13, 34, 17, 20, 45, 38, 44]


@functools.lru_cache(maxsize=None)
def _rand_dev(M, N, Kk):
    c = C.random_operands(M, N, Kk)
    d = {k: v.to(DEV) for k, v in c.items()}
    for mode in ("layernorm", "rmsnorm"):
        d[mode] = ops.derive_norm_gemm(d["w"], d["nw"], d["nb"] if mode == "layernorm" else None, d["bias"])
    return c, d


@functools.lru_cache(maxsize=None)
def _absprod(M, N, Kk):
    c = C.random_operands(M, N, Kk)
    return K.absprod64(c["x"], c["w"])


@functools.lru_cache(maxsize=None)
def _ref_linear(M, N, Kk, act, res, alpha):
    c = C.random_operands(M, N, Kk)
    return K.ref64(c["x"], c["w"], c["bias"], act, c["res"] if res else None, alpha)


LINEAR_EPIS = [("linear", None, True, 0.5), ("linear", "relu", True, 1.0), ("gelu", "gelu", True, 1.0),
               ("silu", "silu", False, 1.0)]


@pytest.mark.parametrize("family,act,res,alpha", LINEAR_EPIS)
@pytest.mark.parametrize("n_kind", C.N_KINDS)
@pytest.mark.parametrize("config", BOUNDED_CONFIGS)
def test_bounded_activations(config, n_kind, family, act, res, alpha):
    M, N, Kk = C.shape(config, n_kind)
    _, d = _rand_dev(M, N, Kk)
    y = ops.ext().gemm(d["x"], d["w"], d["bias"], d["res"] if res else None, ACT[act], alpha, _sentinel(M, N), config, 1)
    pre, ref = _ref_linear(M, N, Kk, act, res, alpha)
    K.check_bound(y, pre, ref, _absprod(M, N, Kk), Kk, family, f"config {config} {act} {(M, N, Kk)}")


@pytest.mark.parametrize("config", [c for c in BOUNDED_CONFIGS if c not in C.SWIGLU_BAD])
def test_bounded_swiglu(config):
    """W rows interleave gate / up blocks of 16, so N is a multiple of 32 (bn + 32: a second
    column tile of one gate / up pair) and the output, N / 2 wide, has 16-byte rows."""
    bm, bn, ks = C.tile(config)
    M, N, Kk = bm + 5, bn + 32, 12 * ks
    c, d = _rand_dev(M, N, Kk)
    y = ops.ext().gemm(d["x"], d["w"], d["bias"], None, ACT["swiglu"], 1.0, _sentinel(M, N // 2), config, 1)
    ref, ap = K.ref64_swiglu(c["x"], c["w"], c["bias"])
    K.check_bound(y, ref, ref, ap, Kk, "swiglu", f"config {config} swiglu {(M, N, Kk)}")


@pytest.mark.parametrize("n_kind", C.N_KINDS)
@pytest.mark.parametrize("config", BOUNDED_CONFIGS)
def test_bounded_rope(config, n_kind):
    M, N, Kk = C.shape(config, n_kind)
    S, D = 16, 32
    cols = N // D * D  # whole heads, across the column-tile edge; the last columns stay unrotated
    c, d = _rand_dev(M, N, Kk)
    cos_t, sin_t = ops.rope_tables(S, D, 10000.0)
    y = ops.ext().gemm(d["x"], d["w"], d["bias"], d["res"], 0, 1.0, _sentinel(M, N), config, 1, None, 0, 1e-5, None, False,
                       cos_t.to(DEV), sin_t.to(DEV), S, D, cols)
    pre, ap = K.ref64_rope(c["x"], c["w"], c["bias"], cos_t, sin_t, S, D, cols)
    K.check_bound(y, pre, pre + c["res"].double(), ap, Kk, "rope", f"config {config} rope {(M, N, Kk)}")


@pytest.mark.parametrize("mode,stats,act", [("layernorm", "in", None), ("layernorm", "ext", None),
                                            ("layernorm", "ext", "gelu"), ("rmsnorm", "in", None),
                                            ("rmsnorm", "ext", "silu")])
@pytest.mark.parametrize("n_kind", C.N_KINDS)
@pytest.mark.parametrize("config", BOUNDED_CONFIGS)
def test_bounded_folded_norm(config, n_kind, mode, stats, act):
    """The reference takes what the kernel takes: the derived bf16 weight and bias, the fp32
    column sums and, handed over, the fp32 row sums ("in": the kernel sums x itself)."""
    M, N, Kk = C.shape(config, n_kind)
    c, d = _rand_dev(M, N, Kk)
    wd, cs, bd = d[mode]
    y = ops.ext().gemm(d["x"], wd, bd, None, ACT[act], 1.0, _sentinel(M, N), config, 1, cs, 1 if mode == "layernorm" else 2,
                       1e-5, None, False, None, None, 1, 2, 0, None, d["stats"] if stats == "ext" else None)
    pre, ref = K.ref64_folded(c["x"], wd.cpu(), cs.cpu(), bd.cpu(), mode, act, c["stats"] if stats == "ext" else None)
    K.check_bound(y, pre, ref, K.absprod64(c["x"], wd.cpu()), Kk, mode, f"config {config} {mode} {stats} {act} {(M, N, Kk)}")


@pytest.mark.parametrize("n_kind", C.N_KINDS)
@pytest.mark.parametrize("config", BOUNDED_CONFIGS)
def test_stats_out(config, n_kind):
    M, N, Kk = C.shape(config, n_kind)
    _, d = _rand_dev(M, N, Kk)
    st = torch.zeros(M, 2, dtype=torch.float32, device=DEV)
    y = ops.ext().gemm(d["x"], d["w"], d["bias"], d["res"], 0, 1.0, _sentinel(M, N), config, 1, stats_out=st)
    pre, ref = _ref_linear(M, N, Kk, None, True, 1.0)
    K.check_bound(y, pre, ref, _absprod(M, N, Kk), Kk, "linear", f"config {config} stats_out {(M, N, Kk)}")
    K.check_stats(st, y, f"config {config} {(M, N, Kk)}")


@pytest.mark.parametrize("mode", ["layernorm", "rmsnorm"])
@pytest.mark.parametrize("n_kind,splitk", [("seg", 1), ("odd", 1), ("seg", 4)])
@pytest.mark.parametrize("config", BOUNDED_CONFIGS)
def test_bounded_post_norm(config, n_kind, splitk, mode):
    """The next norm of the output rows, from the norm kernel (one slice) or the row-owning
    split-K reduce (four slices). Both move rows as 16-byte chunks: N = bn + 2 is refused (it used
    to be accepted, and the norm kernel then dropped each row's last N % 8 columns and read the
    rows from the wrong offsets: errors a thousand times the bound)."""
    M, N, Kk = C.shape(config, n_kind)
    c, d = _rand_dev(M, N, Kk)
    yn = _sentinel(M, N)
    if N % 8:
        with pytest.raises(RuntimeError, match="post-norm needs N % 8 == 0"):
            ops.ext().gemm(d["x"], d["w"], d["bias"], d["res"], 0, 1.0, _sentinel(M, N), config, splitk, norm_out=yn,
                           norm_w=d["pw"], norm_b=d["pb"] if mode == "layernorm" else None,
                           norm_mode=1 if mode == "layernorm" else 2, norm_eps=1e-5)
        assert bool((yn == SENTINEL).all())
        return
    y = ops.ext().gemm(d["x"], d["w"], d["bias"], d["res"], 0, 1.0, _sentinel(M, N), config, splitk, norm_out=yn,
                       norm_w=d["pw"], norm_b=d["pb"] if mode == "layernorm" else None,
                       norm_mode=1 if mode == "layernorm" else 2, norm_eps=1e-5)
    what = f"config {config} post-{mode} split-K {splitk} {(M, N, Kk)}"
    pre, ref = _ref_linear(M, N, Kk, None, True, 1.0)
    ap = _absprod(M, N, Kk)
    K.check_bound(y, pre, ref, ap, Kk, "linear", what)
    yr, z, rs = K.ref64_postnorm(ref, c["pw"], c["pb"], mode)
    K.check_within(yn, yr, K.postnorm_bound(ref, pre, ap, Kk, z, rs, c["pw"], yr, mode), "postnorm", what)


def test_zz_report_bound_ratios():
    """Prints the largest err / derived bound per family seen by the tests above: the source of
    gemm_checks.MEASURED / C_BOUND."""
    for fam in sorted(K.ratios):
        print(f"largest bound ratio {fam}: {K.ratios[fam]:.4g} (C = {K.C_BOUND[fam]})")
        assert K.ratios[fam] <= K.C_BOUND[fam]


# ---------------------------------------------------------------------------------------------
# Split-K tickets

def _advance(before, after):
    return after - before if after >= before else after  # (the pool restarts at 0 when a request does not fit)


@pytest.mark.parametrize("config", C.GLDS)
def test_tickets_cover_the_tile_grid(config):
    """A split-K launch reserves at least one counter per output tile OF ITS CONFIG (the pool's
    cursor advances by the reservation). 256 x 768: 128 tiles of 32 x 48, 12 of 64 x 64."""
    e = ops.ext()
    bm, bn, ks = C.tile(config)
    M, N, Kk = 256, 768, 2 * ks
    d = _dev("integer", M, N, Kk)
    before = e._split_k_cursor(0)
    out = _sentinel(M, N)
    _gemm(d, C.EPI_NONE, config, 2, out=out)
    adv = _advance(before, e._split_k_cursor(0))
    assert adv >= -(-M // bm) * -(-N // bn), f"config {config}: {adv} counters for {-(-M // bm) * -(-N // bn)} tiles"
    K.check_exact(out, _want("integer", M, N, Kk, "none"), f"config {config} split-K 2 {(M, N, Kk)}")


def test_tickets_two_streams_in_flight():
    """Two streams each issue config 27, split-K 2, 512 x 768 x 3072 (256 tiles of 32 x 48, the
    tuner's candidate) on operands of their own, interleaved: launches in flight together must
    not share counters, so every output is exact."""
    M, N, Kk, config = 512, 768, 3072, 27
    p1 = C.integer_probe(M, N, Kk)
    p2 = C.Probe("integer", p1.x.flip(0).contiguous(), p1.w.flip(0).contiguous(), p1.bias.flip(0).contiguous(),
                 p1.res.flip(0, 1).contiguous())
    wants, devs = [], []
    for p in (p1, p2):
        K.check_probe_preconditions(p, C.EPI_FULL)
        wants.append(K.expected_exact(p, C.EPI_FULL).to(DEV))
        devs.append(C.Probe(p.kind, *(t.to(DEV) for t in p[1:])))
    assert not torch.equal(wants[0], wants[1])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[_sentinel(M, N) for _ in range(20)] for _ in range(2)]
    torch.cuda.synchronize()
    for i in range(20):
        for s in range(2):
            with torch.cuda.stream(streams[s]):
                _gemm(devs[s], C.EPI_FULL, config, 2, out=outs[s][i])
    torch.cuda.synchronize()
    bad = [(s, i) for s in range(2) for i in range(20) if not torch.equal(outs[s][i], wants[s])]
    assert not bad, f"(stream, launch) with a wrong output: {bad}"


def test_tickets_after_the_pool_wraps():
    """About a hundred launches of 11 008 tiles (4096 x 4096, config 24, split-K 2) take the
    2^20-counter pool through one lap — every reservation inside it — and an exact split-K launch
    then lands on counters that were used and reset."""
    e = ops.ext()
    M = N = 4096
    Kk = 2 * C.tile(24)[2]
    x = torch.ones(M, Kk, dtype=BF, device=DEV)
    w = torch.ones(N, Kk, dtype=BF, device=DEV)
    out = torch.empty(M, N, dtype=BF, device=DEV)
    tiles = (M // 32) * -(-N // 48)
    start = prev = e._split_k_cursor(0)
    wrapped = False
    for _ in range(2 ** 20 // tiles + 2):
        e.gemm(x, w, None, None, 0, 1.0, out, 24, 2)
        cur = e._split_k_cursor(0)
        assert 0 < cur <= 2 ** 20 and _advance(prev, cur) >= tiles
        wrapped = wrapped or cur < prev
        prev = cur
        if wrapped and cur >= start:
            break
    assert wrapped, "the cursor never returned to the start of the pool"
    torch.cuda.synchronize()
    assert bool((out == Kk).all())
    M, N, Kk = C.shape(24, "seg")
    o = _sentinel(M, N)
    _gemm(_dev("integer", M, N, Kk), C.EPI_FULL, 24, 2, out=o)
    K.check_exact(o, _want("integer", M, N, Kk, C.EPI_FULL.name), "config 24 split-K 2 on reused counters")
