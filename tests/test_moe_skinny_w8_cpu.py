"""``moe_skinny_w8=True`` and ``ops.gemm_grouped_skinny_w8`` without a GPU: the option, ``resume``, the
op's CPU path, all-k decode steps, and the clear rows of the fp8-experts top-2 reference."""
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import moe_decode_checks as M  # noqa: E402
from decode_checks import CAP, B, stream  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402

KW = dict(world=1, batch=B, kv_cache=CAP, moe_decode=True, moe_skinny_w8=True, weight_dtype="fp8-experts")


def test_accepted_and_refused():
    for kw in (dict(seq=1), dict(seq=16), dict(seq=1, generate=True), dict(seq=4, kv_dtype="fp8"),
               dict(seq=1, generate=True, kv_dtype="fp8"), dict(seq=4, placement="pipeline")):
        p = runtime.plan("tiny-mixtral", **KW, **kw)
        assert p.completed == p.total and p.args["moe_skinny_w8"] is True and p.kv_cache_bytes[0] > 0
    refused = [
        (dict(moe_decode=False), "needs moe_decode=True"),
        (dict(model="tiny-llama", weight_dtype="bf16"), "fp8-experts"),
        (dict(weight_dtype="bf16"), "weight_dtype='fp8-experts' only"),
        (dict(weight_dtype="mxfp4-experts", act_dtype="fp8"), "weight_dtype='fp8-experts' only"),
        (dict(act_dtype="fp8"), "act_dtype='fp8'"),
        # without the option the refusal of quantised experts stands; with it, every other rule of moe_decode
        (dict(moe_skinny_w8=False), "weight_dtype='bf16' only"),
        (dict(skinny_gemm=True), "skinny_gemm=True takes weight_dtype='bf16' only"),
        (dict(seq=1, prefill_chunk=8), "prefill_chunk"),
        (dict(tp=2), "tensor or sequence"),
        (dict(placement="expert"), "placement"),
        (dict(seq=17), "1 .. 16"),
    ]
    for kw, match in refused:
        args = dict(KW, model="tiny-mixtral", seq=4)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            runtime.plan(**args)


def test_option_unset_changes_nothing_and_resume(tmp_path):
    a, b = str(tmp_path / "w8.json"), str(tmp_path / "plain.json")
    plain = runtime.plan("tiny-mixtral", world=1, batch=B, seq=4, weight_dtype="fp8-experts")
    runtime.save_plan(plain, b)
    assert "moe_skinny_w8" not in plain.args and "moe_skinny_w8" not in json.load(open(b))["args"]
    p = runtime.plan("tiny-mixtral", seq=4, **KW)
    # the DAG and the program are those of the fp8-experts plan
    assert [(t.id, t.op.kind) for t in p.tasks] == [(t.id, t.op.kind) for t in plain.tasks]
    assert [(i.op, i.task) for i in p.programs[0].instrs] == [(i.op, i.task) for i in plain.programs[0].instrs]
    runtime.save_plan(p, a)
    assert json.load(open(a))["args"]["moe_skinny_w8"] is True
    again = runtime.plan("tiny-mixtral", seq=4, resume=a, **KW)
    assert again.order == p.order and again.args == p.args
    with pytest.raises(ValueError, match="different arguments.*moe_skinny_w8"):  # saved with, asked without
        runtime.plan("tiny-mixtral", world=1, batch=B, seq=4, weight_dtype="fp8-experts", resume=a)
    with pytest.raises(ValueError, match="different arguments.*moe_skinny_w8"):  # saved without, asked with
        runtime.plan("tiny-mixtral", seq=4, resume=b, **KW)


@pytest.mark.parametrize("act,N", [(None, 48), ("swiglu", 96)])
def test_cpu_path_is_gemm_grouped_w8(act, N):
    g = torch.Generator().manual_seed(5)
    K, counts = 160, (3, 0, 17, 2)
    qs, ss = zip(*(ops.quantize_fp8(torch.randn(N, K, generator=g).bfloat16() * 0.1) for _ in counts))
    x = torch.randn(2 * sum(counts), K, generator=g).bfloat16()
    rows = torch.randperm(x.shape[0], generator=g)[:sum(counts)].int()
    off = torch.tensor([0, 3, 3, 20, 22], dtype=torch.int32)
    NO = N // 2 if act else N
    for kw in (dict(out=True), dict(outs=True)):
        mk = lambda: ({"out": torch.zeros(sum(counts), NO, dtype=torch.bfloat16)} if "out" in kw else  # noqa: E731
                      {"outs": [torch.zeros(9, NO, dtype=torch.bfloat16) for _ in counts]})
        got, want = mk(), mk()
        ops.gemm_grouped_skinny_w8(x, qs, ss, off, act=act, a_rows=rows, **got)
        ops.gemm_grouped_w8(x, qs, ss, off, act=act, a_rows=rows, **want)
        pairs = list(zip(*(t["outs"] if "outs" in kw else [t["out"]] for t in (got, want))))
        assert all(torch.equal(u, v) for u, v in pairs) and all(bool(u.any()) == (n > 0) for (u, _), n in
                                                                   zip(pairs, counts if "outs" in kw else (1,)))
    assert ops.grouped_skinny_w8_ok(N, K, act) and not ops.grouped_skinny_w8_ok(N, K + 16, act)
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        ops.gemm_grouped_skinny_w8(x, [q.float().bfloat16() for q in qs], ss, off, act=act, a_rows=rows, **mk())


@pytest.mark.parametrize("T", [1, 4])
def test_all_k_steps_match_the_reference(monkeypatch, T):
    model = M.register_allk("tiny-mixtral", monkeypatch.setitem)
    p = runtime.plan(model, seq=T, **KW)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
    tokens = stream(p.cfg.vocab_size, seed=1)
    ex.set_tokens("@tokens", tokens)
    M.check_steps_allk(p, ex, store, tokens, T, steps=6)


@pytest.mark.parametrize("nb,n,clear", [(1, 32, 19), (2, 24, 28), (2, 64, 82)])
def test_the_fp8_experts_reference_keeps_half_its_rows_clear(nb, n, clear):
    """The near-tie measure needs clear rows to check: asserted on the reference alone."""
    p = runtime.plan("mini-mixtral", seq=1, **dict(KW, batch=nb))
    got = M.top2_reference(p, runtime.make_store(p), stream(p.cfg.vocab_size, seed=1)[:nb], n)[1]
    assert (got.numel(), int(got.sum())) == (nb * n, clear) and 2 * clear >= nb * n
