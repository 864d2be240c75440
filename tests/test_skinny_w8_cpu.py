"""``ops.linear_skinny_w8`` and the plan option ``skinny_w8=True`` without a GPU: the CPU path over
the cases of skinny_w8_cases.py, the refusals, the plan option, and decode steps on the CPU executor
(which never dispatches to the kernel: the option must not change a CPU step)."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import skinny_w8_cases as S  # noqa: E402
from decode_checks import CAP, B, check_steps, stream  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402
from test_skinny_decode_cpu import _prog  # noqa: E402

KW = dict(world=1, batch=B, kv_cache=CAP, weight_dtype="fp8")
FN = ops.linear_skinny_w8


@pytest.mark.parametrize("N,K", S.PLAIN + S.SWIGLU)
def test_cpu_path_bounded(N, K):
    for M in S.MS:
        (S.run_swiglu if (N, K) in S.SWIGLU else S.run_plain)(FN, "cpu", M, N, K, waves=(None,))
    if (N, K) == (272, 2112):
        S.run_plain(FN, "cpu", 5, N, K, waves=(8,), arbitrary=True)


@pytest.mark.parametrize("M,N,K", S.EXACT_SHAPES)
def test_cpu_path_exact(M, N, K):
    for kind in ("integer", "scaled"):
        S.run_exact(FN, "cpu", kind, M, N, K, waves=(None,))
    S.run_codes(FN, "cpu", K, S.run_start_k(16, K) if K > 128 else list(range(K)), None)


def test_refusal_rules():
    ok = dict(M=16, N=48, K=160)
    assert ops.skinny_w8_refusal(**ok) is None and ops.skinny_w8_ok(**ok, act="gelu", waves=16, lda=168, ldw=176)
    for kw in (dict(M=17), dict(M=0), dict(N=0), dict(K=16), dict(K=48), dict(lda=164), dict(lda=152), dict(ldw=168),
               dict(ldw=144), dict(act="swiglu"), dict(act="tanh"), dict(waves=2)):
        assert isinstance(ops.skinny_w8_refusal(**dict(ok, **kw)), str), kw
    assert ops.skinny_w8_ok(16, 64, 160, "swiglu") and ops.SKINNY_W8_MAX_ROWS >= 1
    assert [ops.skinny_w8_waves(N, K, a) for N, K, a in ((128256, 4096, None), (4096, 14336, None), (28672, 8192, "swiglu"))] \
        == [4, 8, 4]
    x, q, s = torch.zeros(2, 64, dtype=torch.bfloat16), torch.zeros(32, 64, dtype=torch.float8_e4m3fn), torch.ones(32)
    assert FN(x, q, s).shape == (2, 32)
    for kw in (dict(x=x.float()), dict(q=q.view(torch.uint8)), dict(q=torch.zeros(32, 64, dtype=torch.bfloat16)),
               dict(scale=torch.ones(31)), dict(scale=s.double()), dict(bias=torch.zeros(32)),
               dict(residual=torch.zeros(2, 32)), dict(out=torch.zeros(2, 32))):
        with pytest.raises(ValueError):
            FN(**dict(dict(x=x, q=q, scale=s), **kw))


def test_plan_accepted_and_unchanged():
    for model, kw in (("tiny-gpt2", dict(seq=1)), ("tiny-llama", dict(seq=4)), ("tiny-gpt2", dict(seq=1, generate=True)),
                      ("tiny-llama", dict(seq=1, prefill_chunk=8)), ("tiny-llama", dict(seq=16, kv_dtype="fp8"))):
        p = runtime.plan(model, skinny_w8=True, **KW, **kw)
        plain = runtime.plan(model, **KW, **kw)
        assert p.completed == p.total and p.args["skinny_w8"] is True and "skinny_w8" not in plain.args
        assert _prog(p) == _prog(plain) and p.order == plain.order and p.placement == plain.placement
        assert p.stats["kernels_per_rank"] == plain.stats["kernels_per_rank"]


@pytest.mark.parametrize("match,kw", [
    ("skinny_w8=True needs a KV cache", dict(kv_cache=None)),
    ("skinny_w8=True takes weight_dtype='fp8' only", dict(weight_dtype="bf16")),
    ("skinny_w8=True does not combine with act_dtype='fp8'", dict(act_dtype="fp8")),
    ("skinny_w8=True does not combine with skinny_gemm=True", dict(skinny_gemm=True))])
def test_plan_refused(match, kw):
    with pytest.raises(ValueError, match=match):
        runtime.plan("tiny-llama", seq=1, skinny_w8=True, **dict(KW, **kw))


def test_saved_plan_resume_and_mismatch(tmp_path):
    a, b = str(tmp_path / "skinny.json"), str(tmp_path / "plain.json")
    p = runtime.plan("tiny-llama", seq=1, skinny_w8=True, **KW)
    plain = runtime.plan("tiny-llama", seq=1, **KW)
    runtime.save_plan(p, a)
    runtime.save_plan(plain, b)
    assert json.load(open(a))["args"]["skinny_w8"] is True and "skinny_w8" not in json.load(open(b))["args"]
    again = runtime.plan("tiny-llama", seq=1, skinny_w8=True, resume=a, **KW)
    assert again.order == p.order and again.args == p.args
    with pytest.raises(ValueError, match="different arguments.*skinny_w8"):
        runtime.plan("tiny-llama", seq=1, resume=a, **KW)
    with pytest.raises(ValueError, match="different arguments.*skinny_w8"):
        runtime.plan("tiny-llama", seq=1, skinny_w8=True, resume=b, **KW)


@pytest.mark.parametrize("model,T", [("tiny-gpt2", 1), ("tiny-llama", 4)])
def test_cpu_steps_are_those_without_the_option(monkeypatch, model, T):
    monkeypatch.setenv("DLS_SKINNY", "all")
    p, plain = runtime.plan(model, seq=T, skinny_w8=True, **KW), runtime.plan(model, seq=T, **KW)
    store = runtime.make_store(p)
    tokens = stream(p.cfg.vocab_size, seed=5)
    ex, ref = runtime.make_executor(p, 0, "cpu", store), runtime.make_executor(plain, 0, "cpu", store)
    assert ex.skinny_w8 and not ex._skinny_on and not ref.skinny_w8
    for e in (ex, ref):
        e.set_tokens("@tokens", tokens)
    check_steps(p, ex, store, tokens, T, steps=3)
    for _ in range(3):
        ref.step()
    assert torch.equal(ex.output("output_projection"), ref.output("output_projection")) and ex._skinny == {}
