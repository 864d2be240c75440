"""Decode steps with an fp8 KV cache (runtime.plan kv_cache=C, kv_dtype="fp8") on the CPU backend:
the plan's byte accounting and the cap check for both cache dtypes, the interface (Plan.args, saved
plans, refusals, the CLI), incremental steps against the bound of decode_fp8_checks.py, restarts,
capacity, kv_randomize, and pipeline ranks of which some hold no cache.
"""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from decode_checks import CAP, B, MARGIN, stream  # noqa: E402
from decode_fp8_checks import check_steps_fp8, quant_shift  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402
from distributed_llm_scheduler_amd.models import reference, registry  # noqa: E402
from distributed_llm_scheduler_amd.parallel import runtime  # noqa: E402
from distributed_llm_scheduler_amd.parallel.executor import synthetic_tokens  # noqa: E402


# ------------------------------------------------------------------------------ accounting

@pytest.mark.parametrize("model", ["tiny-gpt2", "tiny-llama", "gpt2", "llama3-8b-1l"])
def test_cache_bytes_for_both_dtypes(model):
    T, C = 4, 64
    bf = runtime.plan(model, world=1, seq=T, batch=B, kv_cache=C)
    f8 = runtime.plan(model, world=1, seq=T, batch=B, kv_cache=C, kv_dtype="fp8")
    cfg = bf.cfg
    per_bf = 2 * B * C * cfg.kv_heads * cfg.head_dim * 2
    per_f8 = 2 * B * C * cfg.kv_heads * (cfg.head_dim + 4)
    assert bf.kv_cache_bytes == [cfg.n_layer * per_bf] and f8.kv_cache_bytes == [cfg.n_layer * per_f8]
    assert f8.stats["kv_cache_gb_per_rank"] == [cfg.n_layer * per_f8 / 1e9]
    mem_bf = {t.id: t.memory_required for t in bf.tasks}
    for t in f8.tasks:
        if t.op.kind == "attention":
            assert t.op.attrs["kv_dtype"] == "fp8" and registry.kv_cache_bytes(t.op) == per_f8
            assert t.memory_required == pytest.approx(mem_bf[t.id] - (per_bf - per_f8) / 1e9, rel=1e-9)
        else:
            assert "kv_dtype" not in t.op.attrs and t.memory_required == mem_bf[t.id]
    assert all("kv_dtype" not in t.op.attrs for t in bf.tasks)


@pytest.mark.parametrize("model", ["tiny-gpt2", "tiny-llama"])
def test_executor_holds_what_the_plan_counts(model):
    for kv_dtype in ("bf16", "fp8"):
        p = runtime.plan(model, world=1, seq=4, batch=B, kv_cache=CAP, kv_dtype=kv_dtype)
        ex = runtime.make_executor(p, 0, "cpu", runtime.make_store(p))
        assert ex.memory_bytes()["kv_cache"] == p.kv_cache_bytes[0] > 0
        for cs in ex._kv_cache.values():
            assert len(cs) == (4 if kv_dtype == "fp8" else 2)
            assert cs[0].dtype == (torch.uint8 if kv_dtype == "fp8" else torch.bfloat16)
            if kv_dtype == "fp8":
                nkv = p.cfg.kv_heads
                assert cs[2].dtype == torch.float32 and tuple(cs[2].shape) == (B, nkv, CAP) == tuple(cs[3].shape)


def test_a_cap_that_only_the_fp8_cache_fits():
    """The cap is derived from the two byte counts: just under the bf16 caches (which alone pass it:
    the three-figure ValueError) and above what the fp8 plan needs."""
    kw = dict(world=1, seq=4, batch=32, kv_cache=128)
    bf = runtime.plan("tiny-llama", **kw)
    f8 = runtime.plan("tiny-llama", kv_dtype="fp8", **kw)
    pr = f8.programs[0]
    need8 = pr.param_arena_bytes + pr.act_arena_bytes + f8.kv_cache_bytes[0]
    cap = bf.kv_cache_bytes[0] - 1000
    assert need8 < cap < bf.kv_cache_bytes[0], (need8, cap)
    with pytest.raises(ValueError, match=r"GPU 0: parameter arena 0\.\d+ GB \+ activation arena 0\.\d+ GB \+ "
                                         r"KV caches 0\.\d+ GB exceed its cap of 0\.\d+ GB"):
        runtime.plan("tiny-llama", cap_gb=cap / 1e9, **kw)
    ok = runtime.plan("tiny-llama", cap_gb=cap / 1e9, kv_dtype="fp8", **kw)
    assert ok.completed == ok.total and ok.kv_cache_bytes == f8.kv_cache_bytes
    pr = ok.programs[0]
    assert pr.param_arena_bytes + pr.act_arena_bytes + ok.kv_cache_bytes[0] <= cap


def test_second_placement_counts_fp8_bytes():
    """A cap below the unconstrained sum: the plan sets the (fp8) caches aside and re-fills parameters."""
    T = 4
    roomy = runtime.plan("tiny-llama", world=1, seq=T, batch=B, kv_cache=CAP, kv_dtype="fp8")
    pr = roomy.programs[0]
    cap = 0.8 * (pr.param_arena_bytes + pr.act_arena_bytes + roomy.kv_cache_bytes[0])
    p = runtime.plan("tiny-llama", world=1, seq=T, batch=B, kv_cache=CAP, kv_dtype="fp8", cap_gb=cap / 1e9)
    pr = p.programs[0]
    assert p.completed == p.total and pr.counts().get("evict", 0) > 0
    assert pr.param_arena_bytes + pr.act_arena_bytes + p.kv_cache_bytes[0] <= cap
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
    check_steps_fp8(p, ex, store, synthetic_tokens("@tokens", B * CAP, p.cfg.vocab_size).view(B, CAP), T, steps=3,
                    what="tiny-llama capped")


# ------------------------------------------------------------------------------ interface

def test_plan_args_saved_plans_and_refusals(tmp_path):
    base = runtime.plan("tiny-llama", world=1, seq=4, batch=B, kv_cache=CAP)
    same = runtime.plan("tiny-llama", world=1, seq=4, batch=B, kv_cache=CAP, kv_dtype="bf16")
    assert "kv_dtype" not in base.args and "kv_dtype" not in same.args and same.order == base.order
    p = runtime.plan("tiny-llama", world=1, seq=4, batch=B, kv_cache=CAP, kv_dtype="fp8")
    assert p.args["kv_dtype"] == "fp8"
    path, plain = str(tmp_path / "fp8.json"), str(tmp_path / "bf16.json")
    runtime.save_plan(p, path)
    runtime.save_plan(base, plain)
    assert json.load(open(path))["args"]["kv_dtype"] == "fp8" and "kv_dtype" not in json.load(open(plain))["args"]
    again = runtime.plan("tiny-llama", world=1, seq=4, batch=B, kv_cache=CAP, kv_dtype="fp8", resume=path)
    assert again.order == p.order and again.kv_cache_bytes == p.kv_cache_bytes
    with pytest.raises(ValueError, match="kv_dtype"):
        runtime.plan("tiny-llama", world=1, seq=4, batch=B, kv_cache=CAP, resume=path)
    with pytest.raises(ValueError, match="kv_dtype"):
        runtime.plan("tiny-llama", world=1, seq=4, batch=B, kv_cache=CAP, kv_dtype="fp8", resume=plain)
    with pytest.raises(ValueError, match="kv_dtype must be one of"):
        runtime.plan("tiny-llama", world=1, seq=4, batch=B, kv_cache=CAP, kv_dtype="int8")
    with pytest.raises(ValueError, match="needs a KV cache"):
        runtime.plan("tiny-llama", world=1, seq=4, batch=B, kv_dtype="fp8")
    with pytest.raises(ValueError, match="needs a KV cache"):
        registry.build("tiny-llama", batch=B, seq=4, kv_dtype="fp8")
    # every restriction of the cache stays
    for kw, match in ((dict(model="tiny-mixtral"), "MoE"), (dict(tp=2), "tensor or sequence"),
                      (dict(merge_mb=2, replicas=2), "merge_mb"), (dict(seq=17), "1 .. 16")):
        args = dict(model="tiny-llama", world=1, seq=4, batch=1, kv_cache=CAP, kv_dtype="fp8")
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            runtime.plan(**args)
    # independent of the weight / activation dtypes
    w8 = runtime.plan("tiny-llama", world=1, seq=4, batch=B, kv_cache=CAP, kv_dtype="fp8", weight_dtype="fp8",
                      act_dtype="fp8")
    assert w8.kv_cache_bytes == p.kv_cache_bytes


def test_reference_option():
    p = runtime.plan("tiny-llama", world=1, seq=4, batch=B)
    store = runtime.make_store(p)
    tok = stream(p.cfg.vocab_size, seed=1)[:1, :32]
    plain = reference.forward(p.cfg, store, tok)
    assert torch.equal(plain, reference.forward(p.cfg, store, tok, kv_dtype="bf16"))
    q8 = reference.forward(p.cfg, store, tok, kv_dtype="fp8")
    assert 0 < (q8 - plain).abs().max() < 0.1 * plain.abs().max()
    with pytest.raises(ValueError, match="kv_dtype"):
        reference.forward(p.cfg, store, tok, kv_dtype="fp4")


def test_cli_run_reports_the_dtype_and_the_bytes():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    docs = {}
    for dt in ("bf16", "fp8"):
        out = subprocess.run([sys.executable, "-m", "distributed_llm_scheduler_amd.cli", "run", "--model", "tiny-llama",
                              "--seq", "1", "--kv-cache", "64", "--past", "16", "--steps", "2", "--device", "cpu",
                              "--kv-dtype", dt], cwd=root, capture_output=True, text=True, timeout=240)
        assert out.returncode == 0, out.stderr[-2000:]
        docs[dt] = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
        assert docs[dt]["valid"] is True and docs[dt]["kv_dtype"] == dt
    D = 16
    assert docs["fp8"]["kv_cache_gb"] == pytest.approx(docs["bf16"]["kv_cache_gb"] * (D + 4) / (2 * D))


# ------------------------------------------------------------------------------ steps

@pytest.mark.parametrize("T", [1, 4])
@pytest.mark.parametrize("model", ["tiny-gpt2", "tiny-llama"])
def test_incremental_steps(model, T):
    p = runtime.plan(model, world=1, seq=T, batch=B, kv_cache=CAP, kv_dtype="fp8")
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
    tokens = synthetic_tokens("@tokens", B * CAP, p.cfg.vocab_size).view(B, CAP)
    check_steps_fp8(p, ex, store, tokens, T, steps=6)
    assert ex.kv_lengths() == [6 * T] * B
    ex.check_guards()
    # the cache rows written are the project's quantisation of bf16 rows: exactly bf16 when dequantised
    for k, v, ks, vs in ex._kv_cache.values():
        assert torch.isfinite(ops.kv_dequantize(k, ks)[:, :6 * T].float()).all()
        assert (torch.log2(ks[:, :, :6 * T]) % 1 == 0).all() and (torch.log2(vs[:, :, :6 * T]) % 1 == 0).all()


def test_the_wrong_layers_cache_misses_the_bound():
    """The bound is not vacuous: every layer on the first layer's cache (a plumbing error) exceeds it.
    (Swapped K and V scales would not: the rows of these random-init models nearly all share one
    scale. The kernel-level cases vary the scales per row for that reason.)"""
    T = 4
    p = runtime.plan("tiny-llama", world=1, seq=T, batch=B, kv_cache=CAP, kv_dtype="fp8")
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store)
    first = ex._kv_cache[sorted(ex._kv_cache)[0]]
    ex._kv_cache = {t: first for t in ex._kv_cache}
    tokens = synthetic_tokens("@tokens", B * CAP, p.cfg.vocab_size).view(B, CAP)
    with pytest.raises(AssertionError, match=">="):
        check_steps_fp8(p, ex, store, tokens, T, steps=6, what="mutant")


def test_restart_capacity_and_randomize():
    T = 4
    p = runtime.plan("tiny-llama", world=1, seq=T, batch=B, kv_cache=CAP, kv_dtype="fp8")
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
    check_steps_fp8(p, ex, store, synthetic_tokens("@tokens", B * CAP, p.cfg.vocab_size).view(B, CAP), T, steps=3)
    ex.kv_reset()
    other = stream(p.cfg.vocab_size, seed=77)
    ex.set_tokens("@tokens", other)
    check_steps_fp8(p, ex, store, other, T, steps=3, what="tiny-llama restart")
    ex.kv_reset([CAP - T - 1, 0])
    ex.step()
    before = ex.output("output_projection").clone()
    state = {t: [c.clone() for c in cs] for t, cs in ex._kv_cache.items()}
    with pytest.raises(RuntimeError, match="past the KV cache capacity"):
        ex.step()
    assert ex.kv_lengths() == [CAP - 1, T] and torch.equal(ex.output("output_projection"), before)
    assert all(torch.equal(a, b) for t, cs in state.items() for a, b in zip(cs, ex._kv_cache[t]))
    ex.kv_randomize(20, seed=3)
    assert ex.kv_lengths() == [20, 20]
    for k, v, ks, vs in ex._kv_cache.values():
        for c, s in ((k, ks), (v, vs)):
            x = ops.kv_dequantize(c, s).float()
            assert 0.8 < x.std() < 1.2 and abs(x.mean()) < 0.05  # quantised N(0,1) rows
            assert torch.isfinite(s).all() and (torch.log2(s) % 1 == 0).all() and len(s.unique()) > 1
    ex.step()
    assert torch.isfinite(ex.output("output_projection").float()).all() and ex.kv_lengths() == [24, 24]
    ex.check_guards()


# ------------------------------------------------------------------------------ ranks

WORLD, RT = 4, 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = runtime.plan("tiny-llama", world=world, seq=RT, batch=B, placement="pipeline", kv_cache=CAP,
                         kv_dtype="fp8")
        store = runtime.make_store(p)
        ex = runtime.make_executor(p, rank, "cpu", store, pg=dist.group.WORLD, debug=True)
        res = {"rank": rank, "planned": p.kv_cache_bytes[rank], "caches": len(ex._kv_cache), "errs": [],
               "bytes": ex.memory_bytes().get("kv_cache", 0)}
        ex.kv_randomize(8, seed=3)  # every rank, as the CLI and any SPMD caller do
        res["randomized"] = ex.kv_lengths()
        ex.kv_reset()
        tokens = stream(p.cfg.vocab_size, seed=5)
        ex.set_tokens("@tokens", tokens)
        last = p.placement["output_projection"] == rank
        if last:
            Q, ref = quant_shift(p, store, tokens, 3 * RT)
        for n in range(3):
            ex.step()
            if last:
                logits = ex.output("output_projection").float()
                want = ref[:, n * RT:(n + 1) * RT]
                res["errs"].append(((logits - want).abs().max().item(), MARGIN * want.abs().max().item() + 2 * Q))
        res["lengths"] = ex.kv_lengths()
        ex.kv_reset([CAP - RT + 1, 0])
        try:
            ex.step()
            res["raised"] = None
        except RuntimeError as e:
            res["raised"] = str(e)
        ex.check_guards()
        q.put(res)
    finally:
        dist.destroy_process_group()


def test_pipeline_ranks_some_without_a_cache_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(timeout=240)
    assert all(pr.exitcode == 0 for pr in procs), [pr.exitcode for pr in procs]
    results = sorted((q.get(timeout=5) for _ in range(WORLD)), key=lambda r: r["rank"])
    bare = [r["rank"] for r in results if r["planned"] == 0]
    assert bare and len(bare) < WORLD, results
    errs = [e for r in results for e in r["errs"]]
    assert len(errs) == 3 and all(err < bound for err, bound in errs), errs
    for r in results:
        assert (r["caches"] == 0) == (r["planned"] == 0) and r["bytes"] == r["planned"], r
        assert r["randomized"] == [8, 8] and r["lengths"] == [3 * RT] * B, r
        assert r["raised"] is not None and "past the KV cache capacity" in r["raised"], r
