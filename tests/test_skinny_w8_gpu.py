"""The skinny fp8-weight GEMM kernel (csrc/kernels/gemm_skinny_w8.hip) through
``ops.linear_skinny_w8`` over the cases of skinny_w8_cases.py, every W in {4, 8, 16}. The cases of a
kind run in one test, as in test_skinny_gpu.py (a case's message names it): the suite stays short."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import skinny_w8_cases as S  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
FN = ops.linear_skinny_w8


def test_bounded():
    for N, K in S.PLAIN + S.SWIGLU:
        for M in S.MS:
            (S.run_swiglu if (N, K) in S.SWIGLU else S.run_plain)(FN, DEV, M, N, K)
    S.run_plain(FN, DEV, 5, 272, 2112, arbitrary=True)


def test_exact():
    for M, N, K in S.EXACT_SHAPES:
        for kind in ("integer", "scaled"):
            S.run_exact(FN, DEV, kind, M, N, K)
    S.run_codes(FN, DEV, 160, list(range(160)), 4)  # every k: ten launches of 16 rows
    for W in S.WAVES:
        S.run_codes(FN, DEV, 2112, S.run_start_k(W), W)


def _families(M):
    c, q, s, _ = S.operands(M, 256, 2112)
    c = {k: v.to(DEV) for k, v in c.items()}
    q, s = q.to(DEV), s.to(DEV)
    return c["x"], [("gelu", dict(q=q, scale=s, bias=c["bias"], act="gelu", residual=c["res"], alpha=0.5)),
                    ("swiglu", dict(q=q, scale=s, act="swiglu", residual=c["res"][:, :128].contiguous()))]


def test_two_launches_and_row_invariance():
    x, fams = _families(16)
    for W, (name, kw) in ((W, f) for W in S.WAVES for f in fams):
        full = FN(x, waves=W, **kw)
        assert torch.equal(full, FN(x, waves=W, **kw)), f"{name} W {W}: two launches differ"
        for r in range(16):
            one = FN(x[r:r + 1], waves=W, **dict(kw, residual=kw["residual"][r:r + 1]))
            assert torch.equal(one[0], full[r]), f"{name} W {W}: row {r} of M = 16 differs from its M = 1 launch"


def test_graph_replay_after_x_rewritten():
    for fam in (0, 1):
        _graph_replay(fam)


def _graph_replay(fam):
    x, fams = _families(5)
    name, kw = fams[fam]
    x = x.clone()
    out = torch.empty(5, 128 if name == "swiglu" else 256, dtype=BF, device=DEV)
    FN(x, out=out, **kw)  # warm-up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        FN(x, out=out, **kw)
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        first = out.clone()
        assert torch.equal(first, FN(x, **kw))
    x.copy_(torch.flip(x, (0,)) * 0.5)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, FN(x, **kw)) and not torch.equal(out, first)


def test_auto_waves_is_the_host_rule_and_refusals():
    for act in (None, "swiglu"):
        for N in (32, 768, 2304, 6144, 28672, 128256):
            for K in (32, 160, 768, 4096, 14336):
                assert ops.ext().gemm_skinny_w8_waves(N, K, ops.ACT[act]) == ops.skinny_w8_waves(N, K, act)
    x, fams = _families(5)
    assert torch.equal(FN(x, **fams[0][1]), FN(x, waves=ops.skinny_w8_waves(256, 2112), **fams[0][1]))
    z = lambda *shp, dt=BF: torch.zeros(*shp, dtype=dt, device=DEV)  # noqa: E731
    q8 = lambda n, k: z(n, k, dt=torch.uint8).view(torch.float8_e4m3fn)  # noqa: E731
    x, q, s = z(2, 64), q8(32, 64), torch.ones(32, device=DEV)
    FN(x, q, s)
    for kw in (dict(x=z(17, 64)), dict(x=z(2, 48), q=q8(32, 48)), dict(q=q8(48, 64), scale=torch.ones(48, device=DEV), act="swiglu"),
               dict(q=z(32, 64)), dict(scale=torch.ones(31, device=DEV))):
        with pytest.raises(ValueError):
            FN(**dict(dict(x=x, q=q, scale=s), **kw))
    # the binding holds the same rules for a caller that goes round the wrapper
    e = ops.ext()
    assert e.gemm_skinny_w8_refusal(17, 32, 64, 64, 64) != "" and e.gemm_skinny_w8_refusal(16, 32, 64, 64, 64) == ""
    with pytest.raises(RuntimeError):
        e.gemm_skinny_w8(z(17, 64), q, s)
