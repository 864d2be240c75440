"""fp8 expert weights (weight_dtype="fp8-experts") on the CPU: what is marked and what it
weighs, the refusals, the grouped fp8-weight GEMM's reference path, the CPU executor against the
fp32 reference (uncapped, capped, expert-parallel over two ranks), the planner's metric on full
Mixtral under a cap, plans and the CLI."""
import json
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from distributed_llm_scheduler_amd import cli, ops
from distributed_llm_scheduler_amd.models import reference, registry
from distributed_llm_scheduler_amd.models.params import group_layout
from distributed_llm_scheduler_amd.parallel import runtime
from distributed_llm_scheduler_amd.parallel.executor import synthetic_tokens
from distributed_llm_scheduler_amd.parallel.program import steady_fill_bytes

WD = "fp8-experts"


def _check(p, ex, store, tol, rid=""):
    """The measure of tests/test_executor_gpu.py::_check."""
    out = ex.output(f"{rid}output_projection").float().cpu()
    B, S = out.shape[0], out.shape[1]
    tok = synthetic_tokens(f"{rid}@tokens", B * S, p.cfg.vocab_size).view(B, S)
    margins = []
    ref = reference.forward(p.cfg, store, tok, router_margins=margins)
    scale = ref.abs().max().item()
    assert margins  # an MoE model
    # ONLY rows whose router logits (nearly) tie may differ; they must stay a small minority
    row_err = (out - ref).abs().amax(-1)
    risky = torch.stack([m.abs() < 0.05 for m in margins]).any(0)
    bad = row_err > tol * scale
    assert bad.float().mean().item() < 0.1, (int(bad.sum()), int(risky.sum()), row_err.max().item(), scale)
    assert not (bad & ~risky).any(), (int((bad & ~risky).sum()), int(bad.sum()), row_err[~risky].max().item(), scale)


# --------------------------------------------------------------------------- marking, bytes
def test_weight_dtypes_lists_the_three_values():
    assert registry.WEIGHT_DTYPES == ("bf16", "fp8", "fp8-experts")


def test_mixtral_marks_exactly_the_expert_weights():
    _, g16, _ = registry.build("mixtral-8x7b")
    tasks, g8, cfg = registry.build("mixtral-8x7b", weight_dtype=WD)
    expert_groups = [pid for pid in g8 if "_expert_" in pid]
    assert len(expert_groups) == cfg.n_layer * cfg.n_experts == 256
    n_quant = 0
    for pid, grp in g8.items():
        for sp in grp.tensors:
            is_expert_w = ".moe.experts." in sp.name or sp.name.startswith("moe.experts.")
            assert sp.quant == (pid in expert_groups), (pid, sp.name)
            assert sp.quant == is_expert_w, sp.name
            n_quant += sp.quant
    assert n_quant == 2 * 256
    # every quantised tensor is read as an expert's w_gate_up / w_down and as nothing else
    readers = {}
    for t in tasks:
        for key, name in t.op.weights.items():
            readers.setdefault(name, set()).add((t.op.kind, key))
    quant = {sp.name for g in g8.values() for sp in g.tensors if sp.quant}
    for name, r in readers.items():
        assert (name in quant) == (r <= {("moe_expert", "w_gate_up"), ("moe_expert", "w_down")}), (name, r)
    gate = [sp for g in g8.values() for sp in g.tensors if sp.name.endswith("moe.gate")]
    assert len(gate) == cfg.n_layer and not any(sp.quant for sp in gate)
    assert not any(sp.quant for sp in g8["output_weights"].tensors)
    assert not any(sp.quant for pid, g in g8.items() if "attn" in pid for sp in g.tensors)
    b16 = sum(group_layout(g)[0] for g in g16.values())
    b8 = sum(group_layout(g)[0] for g in g8.values())
    F, H = cfg.ffn_dim, cfg.n_embd
    assert 256 * (2 * F * H + H * F) == 45_097_156_608
    assert b16 - b8 == 45_097_156_608 - 4 * (2 * F + H) * 256  # (every size here is a multiple of 256 B)
    assert abs((b16 - b8) / 1e9 - 45.0636) < 0.005
    # bf16 sizes are unchanged
    for pid, grp in g16.items():
        assert all(not s.quant for s in grp.tensors)
        assert group_layout(grp)[0] == sum((2 * s.numel + 255) // 256 * 256 for s in grp.tensors)
        if pid not in expert_groups:
            assert group_layout(g8[pid])[0] == group_layout(grp)[0]


@pytest.mark.parametrize("kw", [dict(model="tiny-llama"), dict(model="tiny-mixtral", tp=2, placement="tensor", world=2),
                                dict(model="tiny-mixtral", sp=2, placement="sequence", world=2)])
def test_fp8_experts_refused_where_it_is_not_built(kw):
    kw = dict(kw)
    model = kw.pop("model")
    with pytest.raises(ValueError):
        runtime.plan(model, seq=16, weight_dtype=WD, **kw)
    with pytest.raises(ValueError):
        registry.build(model, seq=16, weight_dtype=WD, tp=kw.get("tp", 1), sp=kw.get("sp", 1))


def test_fp8_still_refuses_moe_and_points_to_fp8_experts():
    with pytest.raises(ValueError, match="fp8-experts"):
        runtime.plan("tiny-mixtral", seq=16, weight_dtype="fp8")


def test_dense_fp8_marking_is_unchanged():
    _, g8, cfg = registry.build("llama3-8b", weight_dtype="fp8")
    assert sum(sp.quant for g in g8.values() for sp in g.tensors) == 4 * cfg.n_layer + 1


# --------------------------------------------------------------------- ops reference path
def _grouped_problem(seed, G, N, K, counts, swiglu):
    g = torch.Generator().manual_seed(seed)
    R = sum(counts)
    x = torch.randn(R, K, generator=g).to(torch.bfloat16)
    qs, ss = [], []
    for _ in range(G):
        w = (0.05 * torch.randn(N, K, generator=g)).to(torch.bfloat16)
        q, s = ops.quantize_fp8(w)
        if swiglu:
            q = ops.interleave_gate_up(q.view(torch.uint8)).view(torch.float8_e4m3fn)
            s = ops.interleave_gate_up(s)
        qs.append(q)
        ss.append(s * (1.0 + 0.37 * torch.rand(N, generator=g)))  # not powers of two
    off = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32)
    return x, qs, ss, off


@pytest.mark.parametrize("swiglu", [False, True])
@pytest.mark.parametrize("gather", [False, True])
def test_gemm_grouped_w8_cpu_equals_dequantised_gemm_grouped(swiglu, gather):
    counts = [3, 0, 7, 2]
    N, K = 64, 48
    x, qs, ss, off = _grouped_problem(11, 4, N, K, counts, swiglu)
    R, NO = sum(counts), N // 2 if swiglu else N
    act = "swiglu" if swiglu else None
    a_rows = None
    if gather:  # x is a token matrix, every token routed twice
        x = x[:R // 2]
        a_rows = torch.cat([torch.randperm(R // 2), torch.randperm(R // 2)])[torch.randperm(R)].to(torch.int32)
    deq = [ops.dequantize_fp8(q, s, torch.float32) for q, s in zip(qs, ss)]
    out, ref = torch.full((R, NO), 7.0, dtype=torch.bfloat16), torch.full((R, NO), 7.0, dtype=torch.bfloat16)
    ops.gemm_grouped_w8(x, qs, ss, off, act=act, out=out, a_rows=a_rows)
    ops.gemm_grouped(x, deq, off, act=act, out=ref, a_rows=a_rows)
    assert torch.equal(out, ref)
    # compact outputs shorter than the largest group's count: rows past the cap are dropped
    cap = 5
    outs = [torch.full((cap, NO), 7.0, dtype=torch.bfloat16) for _ in counts]
    refs = [torch.full((cap, NO), 7.0, dtype=torch.bfloat16) for _ in counts]
    ops.gemm_grouped_w8(x, qs, ss, off, act=act, outs=outs, a_rows=a_rows)
    ops.gemm_grouped(x, deq, off, act=act, outs=refs, a_rows=a_rows)
    for e, c in enumerate(counts):
        assert torch.equal(outs[e], refs[e])
        assert (outs[e][min(c, cap):] == 7.0).all()
        xs = x[a_rows.long()] if gather else x
        lo = int(off[e])
        assert torch.equal(outs[e][:min(c, cap)], out[lo:lo + min(c, cap)])
        assert torch.equal(out[lo:lo + c], ops.ref_linear(xs[lo:lo + c], deq[e], act=act))


def test_gemm_grouped_w8_wants_e4m3_weights():
    x, qs, ss, off = _grouped_problem(5, 2, 32, 32, [2, 2], False)
    with pytest.raises(TypeError):
        ops.gemm_grouped_w8(x, [q.float().to(torch.bfloat16) for q in qs], ss, off, out=torch.empty(4, 32))
    with pytest.raises((ValueError, RuntimeError)):  # K % 16 != 0
        ops.gemm_grouped_w8(x[:, :24].contiguous(), [q[:, :24].contiguous() for q in qs], ss, off,
                            out=torch.empty(4, 32, dtype=torch.bfloat16))


# ------------------------------------------------------------------------- CPU executor
def test_cpu_executor_fp8_experts_matches_reference():
    p = runtime.plan("tiny-mixtral", world=1, seq=16, batch=2, weight_dtype=WD)
    assert p.completed == p.total and p.args["weight_dtype"] == WD
    store = runtime.make_store(p)
    names = [s.name for g in p.groups.values() for s in g.tensors if s.quant]
    assert len(names) == 2 * p.cfg.n_layer * p.cfg.n_experts
    q, scale = store.quantized(names[0])
    assert q.dtype == torch.float8_e4m3fn and torch.equal(store.tensor(names[0]), ops.dequantize_fp8(q, scale))
    ex = runtime.make_executor(p, 0, "cpu", store)
    ex.step()
    _check(p, ex, store, 0.03)
    # the resident expert weights are fp8 views with their scales; the router weight is bf16
    w = ex._w(names[0])
    assert w.dtype == torch.float8_e4m3fn and ex._w(names[0] + "@scale").dtype == torch.float32
    assert ex._w("layers.0.moe.gate").dtype == torch.bfloat16


@pytest.mark.parametrize("sched", ["EFT", "MRU_spec"])
def test_cpu_executor_fp8_experts_under_cap(sched):
    """0.6 x the need: expert groups are evicted and re-filled as e4m3 + fp32 byte images, the
    SwiGLU interleave of (q, scale) persisted into the image."""
    need = sum(runtime.plan("tiny-mixtral", world=1, seq=16, batch=2, weight_dtype=WD).param_bytes.values()) / 1e9
    p = runtime.plan("tiny-mixtral", world=1, seq=16, batch=2, weight_dtype=WD, cap_gb=0.6 * need, scheduler=sched)
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
    for _ in range(2):
        st = ex.step()
    assert st.param_fills > 0
    _check(p, ex, store, 0.03)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p = runtime.plan("tiny-mixtral", world=world, seq=16, batch=2, placement="expert", weight_dtype=WD)
        store = runtime.make_store(p)
        ex = runtime.make_executor(p, rank, "cpu", store, pg=dist.group.WORLD)
        for _ in range(2):
            st = ex.step()
        while runtime.ep_widen_on_overflow(ex, dist.group.WORLD):  # capacity edges that overflowed
            st = ex.step()
        experts = sorted(t.id for t in p.tasks if t.op.kind == "moe_expert" and p.placement[t.id] == rank)
        ok = None
        if p.placement.get("output_projection") == rank:
            _check(p, ex, store, 0.03)
            ok = True
        q.put({"rank": rank, "sends": st.sends, "ok": ok, "experts": len(experts)})
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_expert_parallel_fp8_experts():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(timeout=240)
    assert all(pr.exitcode == 0 for pr in procs), [pr.exitcode for pr in procs]
    res = [q.get(timeout=5) for _ in range(world)]
    assert sum(r["ok"] is True for r in res) == 1 and sum(r["sends"] for r in res) > 0
    assert all(r["experts"] > 0 for r in res)  # both ranks ran fp8 experts


# --------------------------------------------------------------------- the project's metric
def test_mixtral_under_a_cap_of_0_7_of_the_bf16_parameters():
    bf16 = runtime.plan("mixtral-8x7b", world=1, cost_model="bytes")
    total16 = sum(bf16.param_bytes.values()) / 1e9
    cap = 0.7 * total16
    kw = dict(world=1, cap_gb=cap, cost_model="bytes")
    dfs16 = runtime.plan("mixtral-8x7b", scheduler="DFS", **kw)
    assert dfs16.total == 451 and dfs16.completed < 451
    for sched in ("DFS", "EFT"):
        p = runtime.plan("mixtral-8x7b", scheduler=sched, weight_dtype=WD, **kw)
        assert (p.completed, p.total) == (451, 451), sched
        assert sum(p.param_bytes.values()) / 1e9 < cap
        assert steady_fill_bytes(p.programs[0], p.param_bytes) == 0, sched
        assert p.stats["refill_gb_per_step_per_rank"][0] == 0.0, sched


# ---------------------------------------------------------------------------------- plans
def test_fp8_experts_plan_saves_and_resumes(tmp_path):
    path = str(tmp_path / "plan.json")
    p = runtime.plan("tiny-mixtral", world=1, seq=16, weight_dtype=WD)
    assert p.args["weight_dtype"] == WD
    runtime.save_plan(p, path)
    assert json.load(open(path))["args"]["weight_dtype"] == WD
    q = runtime.plan("tiny-mixtral", world=1, seq=16, weight_dtype=WD, resume=path)
    assert q.order == p.order and q.param_bytes == p.param_bytes
    with pytest.raises(ValueError):  # saved fp8-experts, resumed bf16
        runtime.plan("tiny-mixtral", world=1, seq=16, resume=path)
    path16 = str(tmp_path / "plan16.json")
    runtime.save_plan(runtime.plan("tiny-mixtral", world=1, seq=16), path16)
    with pytest.raises(ValueError):  # saved bf16, resumed fp8-experts
        runtime.plan("tiny-mixtral", world=1, seq=16, weight_dtype=WD, resume=path16)
    path8 = str(tmp_path / "plan8.json")
    runtime.save_plan(runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="fp8"), path8)
    with pytest.raises(ValueError):  # saved fp8 (dense), resumed bf16 — and the other way round
        runtime.plan("tiny-llama", world=1, seq=16, resume=path8)
    assert runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="fp8", resume=path8).args["weight_dtype"] == "fp8"


def test_cli_plan_and_run_fp8_experts(capsys):
    assert cli.main(["plan", "--model", "tiny-mixtral", "--seq", "16", "--weight-dtype", WD]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["weight_dtype"] == WD and out["tasks_completed"] == out["tasks_total"]
    assert cli.main(["plan", "--model", "tiny-mixtral", "--seq", "16"]) == 0
    out16 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out16["weight_dtype"] == "bf16" and out["param_gb"] < out16["param_gb"]
    assert cli.main(["run", "--device", "cpu", "--model", "tiny-mixtral", "--seq", "16", "--steps", "1", "--warmup", "0",
                     "--weight-dtype", WD]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["weight_dtype"] == WD and res["param_gb"] == out["param_gb"]
    assert res["tasks_completed"] == out["tasks_total"]
