"""The wave-private-ring GEMM family (config ids 120..123, csrc/kernels/gemm_private.hip): 32 x 48
tiles whose W waves each multiply the whole tile over a K slice of their own from an LDS ring of
S slots of their own, with no barrier inside the K loop, and meet once, in the one-pass finish.

What this loop can get wrong is a wave reading a slot before its own DMA landed, refilling a slot
before its reads returned, taking a wrong K slice, or a finish that reads a region before the
barrier. The exact probes of gemm_cases.py (integer, scaled, selector: one right answer in every
summation order, compared with ``torch.equal``) show each as a wrong integer, at the smallest
shapes that reach every state of the ring:

* rows and columns: M = 32 + 5 (a second row tile of five rows), N = 48 + 24 (whole 16-byte
  segments) and 48 + 2 (unaligned rows: scalar stores, the bias read in place); NaN-padded operand
  buffers and a NaN-filled output buffer whose padding must stay NaN;
* K = W x 64 x t with t = 1 (the ring never advances), S (every slot once, no refill), S + 1 (the
  first refill of a slot: the WAR case) and 2 S + 1 (the ring wraps twice), plus the flagship
  K = 3072 / 768 at M = 64, N = 96;
* every exact probe runs 20 times, a 64 MB device fill between launches (operands from cold and
  warm caches): all 20 outputs are identical (the race screen of a new synchronisation structure).

Random operands are held to ``ops.ref_linear`` with the helper and bound test_gemm_onepass_gpu.py
applies to config 45. The family refuses — an error, nothing launched — what it does not attach.
"""
import functools

import pytest
import torch

import gemm_cases as gc
import gemm_checks as gk
from distributed_llm_scheduler_amd import ops
from test_gemm_onepass_gpu import TOL, _close

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

PRIVATE = {120: (8, 2), 121: (4, 3), 122: (6, 2), 123: (12, 1)}  # id -> (waves W, ring slots S)
BM, BN = 32, 48
# bias + residual + alpha 0.5 (the family takes no activation): half-integers, exact in bf16
EPI_BRH = gc.Epilogue("bias_res_half", True, True, None, 0.5)
REPS = 20


def _tsteps(S):
    return sorted({1, S, S + 1, 2 * S + 1})


def _ring_cases():
    return [(c, t) for c, (W, S) in sorted(PRIVATE.items()) for t in _tsteps(S)]


def _flagship_cases():
    return [(c, K) for c, (W, S) in sorted(PRIVATE.items()) for K in (768, 3072) if K % (64 * W) == 0]


@functools.lru_cache(maxsize=None)
def _flush():
    return torch.empty(64 << 20, dtype=torch.uint8, device=DEV)


def _gemm(config, x, w, bias=None, res=None, alpha=1.0, out=None, stats=None):
    return ops.ext().gemm(x, w, bias, res, 0, float(alpha), out, config, 1, None, 0, 1e-5, None, False, None, None, 1,
                          2, 0, stats, None)


@functools.lru_cache(maxsize=None)
def _probe_dev(kind, M, N, K):
    p = gc.probe(kind, M, N, K)
    return p, tuple(None if t is None else t.to(DEV) for t in (p.x, p.w, p.bias, p.res))


def _exact_probes(config, M, N, K, reps, poison):
    """Every exact probe of the shape on ``config``: contiguous operands ``reps`` times (cold and
    warm), then — ``poison`` — NaN-padded operands into a NaN-filled output buffer."""
    for kind, epis in (("integer", (gc.EPI_NONE, EPI_BRH)), ("scaled", (gc.EPI_NONE,)), ("selector", (gc.EPI_NONE,))):
        p, (x, w, b, r) = _probe_dev(kind, M, N, K)
        for epi in epis:
            gk.check_probe_preconditions(p, epi)
            want = gk.expected_exact(p, epi)
            what = f"config {config} {kind} {epi.name} ({M}, {N}, {K})"
            bias, res = (b if epi.bias else None), (r if epi.res else None)
            outs = []
            for i in range(reps):
                if i % 2 == 0:
                    _flush().fill_(i & 255)  # the operands leave the caches before every other launch
                outs.append(_gemm(config, x, w, bias, res, epi.alpha))
            torch.cuda.synchronize()
            gk.check_exact(outs[0], want, what)
            for i, o in enumerate(outs[1:], 1):
                assert torch.equal(o, outs[0]), f"{what}: run {i} differs from run 0"
            if poison:
                pd = gc.padded(p.x, p.w, p.res if epi.res else None, DEV)
                gk.check_poison_placement(pd, M, N, K)
                pd.obuf.fill_(float("nan"))
                _gemm(config, pd.a, pd.w, bias, pd.res, epi.alpha, out=pd.out)
                torch.cuda.synchronize()
                o = pd.obuf.cpu()
                gk.check_exact(o[:M, :N], want, what + " padded")
                assert bool(o[M:].isnan().all()) and bool(o[:M, N:].isnan().all()), f"{what}: the padding was written"
                if pd.rbuf is not None:
                    rb = pd.rbuf.cpu()
                    assert bool(rb[M:].isnan().all()) and bool(rb[:M, N:].isnan().all()) and torch.equal(rb[:M, :N], p.res)


@pytest.mark.parametrize("n_kind", gc.N_KINDS)
@pytest.mark.parametrize("config,t", _ring_cases())
def test_private_exact_probes_and_race_screen(config, t, n_kind):
    W, S = PRIVATE[config]
    assert ops.ext().gemm_private_waves(config) == W
    M, N, K = BM + 5, BN + (24 if n_kind == "seg" else 2), W * 64 * t
    _exact_probes(config, M, N, K, REPS, poison=True)


@pytest.mark.parametrize("config,K", _flagship_cases())
def test_private_exact_at_flagship_k(config, K):
    _exact_probes(config, 64, 96, K, 2, poison=False)


@functools.lru_cache(maxsize=None)
def _random(M, N, K):
    g = lambda seed, *shape, scale=1.0: (scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))).to(BF)  # noqa: E731
    cpu = {"x": g(400, M, K, scale=2.0) + 0.4, "w": g(401, N, K, scale=0.04), "bias": g(402, N, scale=0.2),
           "res": g(403, M, N)}
    ref = {
        "none": ops.ref_linear(cpu["x"], cpu["w"]),
        "bias": ops.ref_linear(cpu["x"], cpu["w"], cpu["bias"]),
        "bias_res_stats": ops.ref_linear(cpu["x"], cpu["w"], cpu["bias"], None, cpu["res"]),
        "alpha": ops.ref_linear(cpu["x"], cpu["w"], cpu["bias"], None, None, 0.37),
    }
    return {k: v.to(DEV) for k, v in cpu.items()}, ref


def _run_random(config, M, N, K, epi):
    d, _ = _random(M, N, K)
    if epi == "none":
        return _gemm(config, d["x"], d["w"]), None
    if epi == "bias":
        return _gemm(config, d["x"], d["w"], d["bias"]), None
    if epi == "alpha":
        return _gemm(config, d["x"], d["w"], d["bias"], None, 0.37), None
    st = torch.zeros(M, 2, dtype=torch.float32, device=DEV)
    return _gemm(config, d["x"], d["w"], d["bias"], d["res"], stats=st), st


def _check_stats(st, y):
    yf = y.cpu().float()
    ref = torch.stack([yf.sum(1), (yf * yf).sum(1)], 1)
    assert torch.allclose(st.cpu(), ref, rtol=1e-4, atol=1e-2), (st.cpu() - ref).abs().max()


@pytest.mark.parametrize("epi", ["none", "bias", "bias_res_stats", "alpha"])
@pytest.mark.parametrize("n_kind", gc.N_KINDS)
@pytest.mark.parametrize("config", sorted(PRIVATE))
def test_private_epilogues_random(config, n_kind, epi):
    """Random operands against ops.ref_linear in fp32 (the bound of test_gemm_onepass_gpu.py); the
    emitted statistics against fp32 row sums of the bf16 output."""
    W, S = PRIVATE[config]
    M, N, K = BM + 5, BN + (24 if n_kind == "seg" else 2), W * 64 * (S + 1)
    y, st = _run_random(config, M, N, K, epi)
    torch.cuda.synchronize()
    assert y.shape == (M, N)
    _close(y.cpu(), _random(M, N, K)[1][epi], TOL["bias_res_stats" if epi == "bias_res_stats" else "bias"])
    if st is not None:
        _check_stats(st, y)


@pytest.mark.parametrize("config", sorted(PRIVATE))
def test_private_is_deterministic(config):
    """The same launch twice: bit-identical C (the W regions are summed in ascending wave order);
    stats_out is atomics and is held to the statistics bound on both runs."""
    W, S = PRIVATE[config]
    M, N, K = 300, 144, W * 64 * (2 * S + 1)
    y1, s1 = _run_random(config, M, N, K, "bias_res_stats")
    y2, s2 = _run_random(config, M, N, K, "bias_res_stats")
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)
    _close(y1.cpu(), _random(M, N, K)[1]["bias_res_stats"], TOL["bias_res_stats"])
    _check_stats(s1, y1)
    _check_stats(s2, y2)


@pytest.mark.parametrize("config", sorted(PRIVATE))
def test_private_refuses_what_it_does_not_attach(config):
    """Each of these raises instead of launching: the output buffer keeps its fill."""
    W, S = PRIVATE[config]
    M, N, K = 40, 64, W * 64 * 2
    g = ops.ext().gemm
    x = torch.ones(M, K, dtype=BF, device=DEV)
    w = torch.ones(N, K, dtype=BF, device=DEV)
    out = torch.full((M, N), 7.0, dtype=BF, device=DEV)
    out_half = torch.full((M, N // 2), 7.0, dtype=BF, device=DEV)
    colsum = torch.zeros(N, dtype=torch.float32, device=DEV)
    ext_stats = torch.ones(M, 2, dtype=torch.float32, device=DEV)
    rows = torch.tensor([0, M], dtype=torch.int32, device=DEV)
    cos_t, sin_t = ops.rope_tables(M, 16, 10000.0, DEV)
    refused = {
        "k tiles not divisible by W": lambda: g(torch.ones(M, K + 64, dtype=BF, device=DEV),
                                                torch.ones(N, K + 64, dtype=BF, device=DEV), None, None, 0, 1.0, out,
                                                config, 1),
        "folded norm": lambda: g(x, w, None, None, 0, 1.0, out, config, 1, colsum, 1, 1e-5, None, False, None, None, 1, 2,
                                 0, None, ext_stats),
        "gelu": lambda: g(x, w, None, None, 1, 1.0, out, config, 1),
        "rope": lambda: g(x, w, None, None, 0, 1.0, out, config, 1, None, 0, 1e-5, None, False, cos_t, sin_t, M, 16, 16),
        "swiglu": lambda: g(x, w, None, None, 4, 1.0, out_half, config, 1),
        "split-K": lambda: g(x, w, None, None, 0, 1.0, out, config, 2),
        "row range": lambda: g(x, w, None, None, 0, 1.0, out, config, 1, None, 0, 1e-5, rows),
    }
    for what, launch in refused.items():
        with pytest.raises(RuntimeError):
            launch()
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((out_half == 7.0).all()), f"{what}: something was launched"
    # and the plain launch of the same operands is taken
    g(x, w, None, None, 0, 1.0, out, config, 1)
    torch.cuda.synchronize()
    assert bool((out == float(K)).all())
