"""Decode steps of fp8-weight plans with ``skinny_w8=True`` on the GPU, under ``DLS_SKINNY=all``: one
eager step, then ONE captured hipGraph under torch's sync debug mode, held to decode_checks' margin
against the fp32 reference on the dequantised store, with ``ex._skinny`` saying that every dense GEMM
ran skinny (GPT-2's tied bf16 LM head on the bf16 kernel); the fallbacks; a ``prefill_chunk`` plan."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import decode_fp8_checks as D8  # noqa: E402
import generate_checks as G  # noqa: E402
import prefill_checks as P  # noqa: E402
from decode_checks import CAP, B, check_steps, stream  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402
from test_skinny_decode_gpu import _all_skinny, _dense_gemms, _each, _no_sync  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
sync = torch.cuda.synchronize
MODELS = ("mini-gpt2", "mini-llama")


def _executor(model, T, skinny=True, batch=B, graph=True, seed=3, store=None, **kw):
    p = runtime.plan(model, world=1, seq=T, batch=batch, kv_cache=CAP, weight_dtype="fp8",
                     **(dict(skinny_w8=True) if skinny else {}), **kw)
    store = store or runtime.make_store(p)
    tokens = stream(p.cfg.vocab_size, seed=seed)[:batch]
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=graph, autotune=False)
    ex.set_tokens("@tokens", tokens)
    return p, store, tokens, ex


def test_steps_one_eager_then_one_graph(monkeypatch):
    """Both models, T in {1, 4}, both kv_dtypes: eight plans in one test, as test_skinny_decode_gpu.py."""
    monkeypatch.setenv("DLS_SKINNY", "all")
    _each(_steps, *[(m, T, kv) for m in MODELS for T in (1, 4) for kv in ("bf16", "fp8")])


def _steps(model, T, kv_dtype):
    check = D8.check_steps_fp8 if kv_dtype == "fp8" else check_steps
    p, store, tokens, ex = _executor(model, T, kv_dtype=kv_dtype)
    check(p, ex, store, tokens, T, 1, sync=sync)  # eager (derives weights: may sync)
    _all_skinny(ex, p)
    assert ex.capture() and ex._graph is not None and not ex._segments
    check(p, ex, store, tokens, T, 5, start=T, sync=sync, step=_no_sync(ex.step))
    _all_skinny(ex, p)
    kinds = {ex._w(w).dtype for _, w in _dense_gemms(p)}  # the tied LM head of GPT-2 is a bf16 weight
    assert kinds == {torch.float8_e4m3fn} | ({torch.bfloat16} if model == "mini-gpt2" else set())
    last = ex.output("output_projection").clone()
    ex.kv_reset()  # the same graph from the same state: bit-identical (no unordered sum in the step)
    for _ in range(6):
        ex.step()
    sync()
    assert torch.equal(ex.output("output_projection"), last)
    plain = _executor(model, T, False, store=store, kv_dtype=kv_dtype)[3]  # the same step without the option
    plain.step()
    assert plain.capture() and 0 < ex.launches <= plain.launches, (ex.launches, plain.launches)


def test_fallbacks_switch_and_default_row_limit(monkeypatch):
    """32 rows fall back with the reason; DLS_SKINNY=0 turns the dispatch off (the plain plan's
    launches); without DLS_SKINNY the dispatch respects ops.SKINNY_W8_MAX_ROWS."""
    for mode, T, nb in (("all", 16, B), ("0", 1, B), (None, 1, 1), (None, 1, 2)):
        monkeypatch.delenv("DLS_SKINNY", raising=False) if mode is None else monkeypatch.setenv("DLS_SKINNY", mode)
        _each(_fallback, (mode, T, nb))


def _fallback(mode, T, nb):
    p, store, tokens, ex = _executor("mini-llama", T, batch=nb, graph=mode == "0", seed=5)
    check_steps(p, ex, store, tokens, T, 2, sync=sync)
    if mode == "0":
        plain = _executor("mini-llama", T, False, store=store)[3]
        plain.step()
        assert ex.capture() and plain.capture() and ex._skinny == {} and ex.launches == plain.launches
        return
    assert set(ex._skinny) >= _dense_gemms(p)
    rows, limit = nb * T, 16 if mode == "all" else ops.SKINNY_W8_MAX_ROWS
    for key, v in ex._skinny.items():
        assert v == "skinny" if rows <= limit else v.startswith(f"M = {rows} rows"), (key, v)


def test_prefill_chunk_generate_plan(monkeypatch):
    """Chunk steps keep the gemm_w8 tiles (nothing of them is recorded in ex._skinny), token steps
    run skinny, and the generation repeats bit for bit."""
    monkeypatch.setenv("DLS_SKINNY", "all")
    _each(_prefill_chunk, *[(m,) for m in MODELS])


def _prefill_chunk(model):
    p = runtime.plan(model, world=1, seq=1, batch=B, kv_cache=256, prefill_chunk=48, generate=True, weight_dtype="fp8",
                     skinny_w8=True)
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, DEV, store, use_graph=True, autotune=False)
    g = torch.Generator().manual_seed(11)
    prompts = tuple(torch.randint(0, p.cfg.vocab_size, (n + 1,), generator=g).tolist() for n in (200, 9))
    ex.set_sampling(**G.SAMPLING)
    ex.set_prompts("@tokens", prompts)
    assert ex.prefill() == 5 and ex._skinny == {}  # chunk steps only so far: tiles
    chunks, *eager = P.run_generate(ex, G.SAMPLING, prompts=prompts, sync=sync)  # eager: derives the weights
    _all_skinny(ex, p)
    P.check_generate(p, store, G.SAMPLING, *eager, prompts=prompts)
    assert chunks == 5 and ex.capture() and ex._chunk_graph is not None
    _, *first = P.run_generate(ex, G.SAMPLING, prompts=prompts, sync=sync, step=_no_sync(ex.step))
    _, *again = P.run_generate(ex, G.SAMPLING, prompts=prompts, sync=sync)
    assert torch.equal(again[2], first[2]) and all(torch.equal(a, b) for a, b in zip(again[0], first[0]))
    _all_skinny(ex, p)
