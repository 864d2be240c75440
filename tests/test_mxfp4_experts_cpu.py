"""MXFP4 expert weights (weight_dtype="mxfp4-experts", act_dtype="fp8") on the CPU: what is marked
and what it weighs, the refusals, plans and the CLI, the grouped W4A8 GEMM's reference path, and
the CPU executor (uncapped, capped, expert-parallel over two ranks).

Executor rule (that of tests/test_mxfp4_cpu.py): the mode is held to 2 x what the CPU backend
measures against reference.forward(act_dtype="fp8") on the same store. Measured with the all-k
variant of tiny-mixtral (top_k = n_experts = 4: every expert takes every token, so routing cannot
differ and no row is exempt), batch 2 x 16, as (max-abs error / max |logit|, rms-relative error):
0.0065 and 0.0052. The ordinary top-2 tiny-mixtral takes the margin measure of
tests/test_w8_experts_cpu.py (a row may be over the tolerance only if one of its router margins is
below 0.05) with the tolerance by the same rule: over the rows whose margins are all >= 0.05 the
largest row error is 0.0050 of max |logit|, so the tolerance is 0.0100; no row is over it, capped
or not, and at most 5 % may be."""
import json
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from distributed_llm_scheduler_amd import cli, ops
from distributed_llm_scheduler_amd.models import config, reference, registry
from distributed_llm_scheduler_amd.models.params import group_layout
from distributed_llm_scheduler_amd.parallel import runtime
from distributed_llm_scheduler_amd.parallel.executor import DAGExecutor, synthetic_tokens

WD = "mxfp4-experts"
KW = dict(weight_dtype=WD, act_dtype="fp8")
ALLK = "tiny-mixtral-allk"
ALLK_CPU = (0.0065, 0.0052)  # CPU backend, all-k tiny-mixtral, batch 2 x 16 (the header)
TOP2_TOL = 2 * 0.0050       # CPU backend, top-2 tiny-mixtral, rows with every margin >= 0.05


def _register_allk():
    c = config.PRESETS["tiny-mixtral"]
    return c.with_(name=ALLK, top_k=c.n_experts)


@pytest.fixture
def allk(monkeypatch):
    monkeypatch.setitem(config.PRESETS, ALLK, _register_allk())
    return ALLK


def _check_allk(p, ex, store):
    out = ex.output("output_projection").float().cpu()
    B, S = out.shape[0], out.shape[1]
    tok = synthetic_tokens("@tokens", B * S, p.cfg.vocab_size).view(B, S)
    ref = reference.forward(p.cfg, store, tok, act_dtype="fp8")
    d = out - ref
    maxrel = d.abs().max().item() / ref.abs().max().item()
    rmsrel = (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
    print(f"{p.cfg.name}: max-abs / max-|logit| {maxrel:.4f}, rms-relative {rmsrel:.4f}")
    assert maxrel <= 2 * ALLK_CPU[0] and rmsrel <= 2 * ALLK_CPU[1], (maxrel, rmsrel)


def _check(p, ex, store, tol=TOP2_TOL):
    """The measure of tests/test_w8_experts_cpu.py::_check against the fp8-activation reference;
    the CPU backend itself stays at or below 5 % of rows over the tolerance."""
    out = ex.output("output_projection").float().cpu()
    B, S = out.shape[0], out.shape[1]
    tok = synthetic_tokens("@tokens", B * S, p.cfg.vocab_size).view(B, S)
    margins = []
    ref = reference.forward(p.cfg, store, tok, router_margins=margins, act_dtype="fp8")
    scale = ref.abs().max().item()
    assert margins
    row_err = (out - ref).abs().amax(-1)
    risky = torch.stack([m.abs() < 0.05 for m in margins]).any(0)
    bad = row_err > tol * scale
    print(f"{p.cfg.name}: bad rows {int(bad.sum())}/{bad.numel()}, risky {int(risky.sum())}, "
          f"max row err / scale {row_err.max().item() / scale:.4f}")
    assert bad.float().mean().item() <= 0.05, (int(bad.sum()), int(risky.sum()), row_err.max().item(), scale)
    assert not (bad & ~risky).any(), (int((bad & ~risky).sum()), int(bad.sum()), row_err[~risky].max().item(), scale)


# --------------------------------------------------------------------------- marking, bytes
def test_accepted_values():
    assert registry.MX_EXPERT_WEIGHT_DTYPES == ("mxfp4-experts",)
    assert registry.WEIGHT_DTYPES == ("bf16", "fp8", "fp8-experts") and registry.MX_WEIGHT_DTYPES == ("mxfp4",)


def test_mixtral_marks_what_fp8_experts_marks_and_weighs_by_hand():
    _, g16, cfg = registry.build("mixtral-8x7b")
    _, g8, _ = registry.build("mixtral-8x7b", weight_dtype="fp8-experts")
    _, g4, _ = registry.build("mixtral-8x7b", **KW)
    m8 = {sp.name for g in g8.values() for sp in g.tensors if sp.quant}
    m4 = {sp.name for g in g4.values() for sp in g.tensors if sp.quant}
    assert m4 == m8 and len(m4) == 2 * cfg.n_layer * cfg.n_experts == 512
    assert all(sp.qfmt == "mxfp4" for g in g4.values() for sp in g.tensors if sp.quant)
    gate = [sp for g in g4.values() for sp in g.tensors if sp.name.endswith("moe.gate")]
    assert len(gate) == cfg.n_layer and not any(sp.quant for sp in gate)
    assert not any(sp.quant for sp in g4["output_weights"].tensors)
    assert not any(sp.quant for pid, g in g4.items() if "attn" in pid for sp in g.tensors)
    # N K / 2 + N K / 32 bytes per expert tensor (both parts are multiples of 256 B here)
    F, H = cfg.ffn_dim, cfg.n_embd
    per_expert = (2 * F * H // 2 + 2 * F * H // 32) + (H * F // 2 + H * F // 32)
    assert per_expert % 256 == 0 and 256 * per_expert == 23_957_864_448
    b16 = sum(group_layout(g)[0] for g in g16.values())
    b4 = sum(group_layout(g)[0] for g in g4.values())
    assert b16 - b4 == 256 * (2 * 3 * F * H) - 256 * per_expert
    for pid, grp in g16.items():
        if "_expert_" not in pid:
            assert group_layout(g4[pid])[0] == group_layout(grp)[0]


def test_plan_bytes_of_tiny_mixtral_by_hand():
    """tiny-mixtral: 2 layers x 4 experts, hidden 64, ffn 96: gate_up [192, 64] and down [64, 96]
    per expert, each part rounded up to 256 B in the arena layout."""
    p = runtime.plan("tiny-mixtral", world=1, seq=16, **KW)
    pb = runtime.plan("tiny-mixtral", world=1, seq=16)
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    mx = (up(192 * 64 // 2) + up(192 * 64 // 32)) + (up(64 * 96 // 2) + up(64 * 96 // 32))
    bf = up(2 * 192 * 64) + up(2 * 64 * 96)
    assert sum(pb.param_bytes.values()) - sum(p.param_bytes.values()) == 8 * (bf - mx)
    assert p.args["weight_dtype"] == WD and p.args["act_dtype"] == "fp8"


def test_refusals():
    registry.build("tiny-mixtral", seq=16, **KW)
    registry.check_act_dtype("fp8", WD)
    with pytest.raises(ValueError, match="MoE model"):  # a model without experts
        registry.build("tiny-llama", seq=16, **KW)
    with pytest.raises(ValueError, match="parallelism"):
        registry.build("tiny-mixtral", seq=16, tp=2, **KW)
    with pytest.raises(ValueError, match="parallelism"):
        registry.build("tiny-mixtral", seq=16, sp=2, **KW)
    with pytest.raises(ValueError, match="W4A8"):
        registry.build("tiny-mixtral", seq=16, weight_dtype=WD, act_dtype="bf16")
    with pytest.raises(ValueError, match="W4A8"):
        runtime.plan("tiny-mixtral", seq=16, weight_dtype=WD)  # the default activations are bf16
    with pytest.raises(ValueError):
        runtime.plan("tiny-mixtral", seq=16, tp=2, placement="tensor", world=2, **KW)
    # the older refusals are intact
    with pytest.raises(ValueError, match="does not cover MoE"):
        registry.build("tiny-mixtral", seq=16, weight_dtype="mxfp4", act_dtype="fp8")
    with pytest.raises(ValueError, match="needs weight_dtype='fp8' or 'mxfp4'"):
        registry.build("tiny-mixtral", seq=16, weight_dtype="fp8-experts", act_dtype="fp8")
    with pytest.raises(ValueError, match="fp8-experts"):
        registry.build("tiny-mixtral", seq=16, weight_dtype="fp8")
    with pytest.raises(ValueError, match="weight_dtype"):
        registry.build("tiny-mixtral", seq=16, weight_dtype="mxfp6-experts", act_dtype="fp8")


def test_marked_k_must_be_a_multiple_of_32():
    """No registered MoE model has such a weight, so an expert's down projection is widened by 16."""
    tasks, groups, _ = registry.build("tiny-mixtral", seq=16)
    name = next(t.op.weights["w_down"] for t in tasks if t.op.kind == "moe_expert")
    sp = next(t for g in groups.values() for t in g.tensors if t.name == name)
    sp.shape = (sp.shape[0], sp.shape[1] + 16)
    with pytest.raises(ValueError, match="multiple of 32"):
        registry.mark_fp8(tasks, groups, registry._EXPERT_OPERANDS, fmt="mxfp4")


def test_executor_refuses_the_store_without_fp8_activations():
    p = runtime.plan("tiny-mixtral", world=1, seq=16, **KW)
    with pytest.raises(ValueError, match="act_dtype"):
        DAGExecutor(p.tasks, p.programs[0], runtime.make_store(p), "cpu", model_cfg=p.cfg)


# ---------------------------------------------------------------------------------- plans
def test_plan_saves_and_resumes(tmp_path):
    path = str(tmp_path / "plan.json")
    p = runtime.plan("tiny-mixtral", world=1, seq=16, **KW)
    runtime.save_plan(p, path)
    saved = json.load(open(path))["args"]
    assert saved["weight_dtype"] == WD and saved["act_dtype"] == "fp8"
    q = runtime.plan("tiny-mixtral", world=1, seq=16, resume=path, **KW)
    assert q.order == p.order and q.param_bytes == p.param_bytes
    with pytest.raises(ValueError):  # saved mxfp4-experts, resumed fp8-experts
        runtime.plan("tiny-mixtral", world=1, seq=16, weight_dtype="fp8-experts", resume=path)
    with pytest.raises(ValueError):  # ... resumed bf16
        runtime.plan("tiny-mixtral", world=1, seq=16, resume=path)
    path8 = str(tmp_path / "plan8.json")
    runtime.save_plan(runtime.plan("tiny-mixtral", world=1, seq=16, weight_dtype="fp8-experts"), path8)
    with pytest.raises(ValueError):  # saved fp8-experts, resumed mxfp4-experts
        runtime.plan("tiny-mixtral", world=1, seq=16, resume=path8, **KW)


def test_cli_plan_and_run(capsys):
    args = ["--model", "tiny-mixtral", "--seq", "16", "--weight-dtype", WD, "--act-dtype", "fp8"]
    assert cli.main(["plan"] + args) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["weight_dtype"] == WD and out["act_dtype"] == "fp8" and out["tasks_completed"] == out["tasks_total"]
    assert cli.main(["plan", "--model", "tiny-mixtral", "--seq", "16", "--weight-dtype", "fp8-experts"]) == 0
    out8 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["param_gb"] < out8["param_gb"]
    assert cli.main(["run", "--device", "cpu", "--steps", "1", "--warmup", "0"] + args) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["weight_dtype"] == WD and res["param_gb"] == out["param_gb"] and res["valid"]
    assert res["tasks_completed"] == out["tasks_total"]


# --------------------------------------------------------------------- ops reference path
def _grouped_problem(seed, G, N, K, T, swiglu):
    g = torch.Generator().manual_seed(seed)
    xq, _ = ops.quantize_fp8(torch.randn(T, K, generator=g).to(torch.bfloat16))
    xs = 2.0 ** torch.randint(-6, 4, (T,), generator=g).float() * (1.0 + 0.37 * torch.rand(T, generator=g))
    qs, ss = [], []
    for _ in range(G):
        q, s = ops.quantize_mxfp4((0.05 * torch.randn(N, K, generator=g)).to(torch.bfloat16))
        if swiglu:
            q, s = ops.interleave_gate_up(q), ops.interleave_gate_up(s)
        qs.append(q)
        ss.append(s)
    return xq, xs, qs, ss


@pytest.mark.parametrize("swiglu", [False, True])
@pytest.mark.parametrize("gather", [False, True])
def test_gemm_grouped_w4a8_cpu_equals_dequantised_gemm_grouped(swiglu, gather):
    counts = [3, 0, 7, 2]
    N, K = 64, 96
    R, NO = sum(counts), N // 2 if swiglu else N
    xq, xs, qs, ss = _grouped_problem(11, 4, N, K, R // 2 if gather else R, swiglu)
    off = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32)
    act = "swiglu" if swiglu else None
    a_rows = None
    if gather:  # xq is a token matrix, every token routed twice: rows AND scales are gathered
        a_rows = torch.cat([torch.randperm(R // 2), torch.randperm(R // 2)])[torch.randperm(R)].to(torch.int32)
    xd = ops.dequantize_fp8(xq, xs, torch.float32)
    deq = [ops.dequantize_mxfp4(q, s, torch.float32) for q, s in zip(qs, ss)]
    out, ref = torch.full((R, NO), 7.0, dtype=torch.bfloat16), torch.full((R, NO), 7.0, dtype=torch.bfloat16)
    ops.gemm_grouped_w4a8(xq, xs, qs, ss, off, act=act, out=out, a_rows=a_rows)
    ops.gemm_grouped(xd, deq, off, act=act, out=ref, a_rows=a_rows)
    assert torch.equal(out, ref)
    rows = a_rows.long() if gather else torch.arange(R)
    for e, c in enumerate(counts):  # the definition, with the scale of the SOURCE row
        lo = int(off[e])
        r = rows[lo:lo + c]
        want = ops.ref_linear(xq.float()[r] * xs[r][:, None], deq[e], act=act).to(torch.bfloat16)
        assert torch.equal(out[lo:lo + c], want)
    cap = 5
    outs = [torch.full((cap, NO), 7.0, dtype=torch.bfloat16) for _ in counts]
    ops.gemm_grouped_w4a8(xq, xs, qs, ss, off, act=act, outs=outs, a_rows=a_rows)
    for e, c in enumerate(counts):
        lo, n = int(off[e]), min(c, cap)
        assert torch.equal(outs[e][:n], out[lo:lo + n]) and (outs[e][n:] == 7.0).all()


def test_gemm_grouped_w4a8_refusals():
    xq, xs, qs, ss = _grouped_problem(5, 2, 32, 64, 4, False)
    off = torch.tensor([0, 2, 4], dtype=torch.int32)
    out = torch.empty(4, 32, dtype=torch.bfloat16)
    with pytest.raises(TypeError):
        ops.gemm_grouped_w4a8(xq.float().to(torch.bfloat16), xs, qs, ss, off, out=out)
    with pytest.raises(TypeError):
        ops.gemm_grouped_w4a8(xq, xs, [q.view(torch.float8_e4m3fn) for q in qs], ss, off, out=out)
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.gemm_grouped_w4a8(xq[:, :48].contiguous(), xs, [q[:, :24].contiguous() for q in qs], ss, off, out=out)
    with pytest.raises(ValueError, match="expected q"):
        ops.gemm_grouped_w4a8(xq, xs, qs, [s[:, :1] for s in ss], off, out=out)
    with pytest.raises(ValueError, match="xscale"):
        ops.gemm_grouped_w4a8(xq, xs[:3], qs, ss, off, out=out)
    with pytest.raises(ValueError, match="swiglu"):
        ops.gemm_grouped_w4a8(xq, xs, qs, ss, off, act="gelu", out=out)


# ------------------------------------------------------------------------- CPU executor
def test_cpu_executor_matches_reference(allk):
    for model, check in ((allk, _check_allk), ("tiny-mixtral", _check)):
        p = runtime.plan(model, world=1, seq=16, batch=2, **KW)
        assert p.completed == p.total
        store = runtime.make_store(p)
        names = [s.name for g in p.groups.values() for s in g.tensors if s.quant]
        assert len(names) == 2 * p.cfg.n_layer * p.cfg.n_experts
        q, s = store.quantized(names[0])
        assert q.dtype == torch.uint8 and torch.equal(store.tensor(names[0]), ops.dequantize_mxfp4(q, s))
        ex = runtime.make_executor(p, 0, "cpu", store)
        ex.step()
        check(p, ex, store)
        assert ex._w(names[0]).dtype == torch.uint8 and ex._w(names[0] + "@scale").dtype == torch.uint8
        assert ex._w("layers.0.moe.gate").dtype == torch.bfloat16


@pytest.mark.parametrize("sched", ["EFT", "MRU_spec"])
def test_cpu_executor_under_cap(allk, sched):
    """0.6 x the need: expert groups are evicted and re-filled as MXFP4 byte images, the SwiGLU
    interleave of (q, s) persisted into the image."""
    for model, check in ((allk, _check_allk), ("tiny-mixtral", _check)):
        need = sum(runtime.plan(model, world=1, seq=16, batch=2, **KW).param_bytes.values()) / 1e9
        p = runtime.plan(model, world=1, seq=16, batch=2, cap_gb=0.6 * need, scheduler=sched, **KW)
        assert p.completed == p.total
        store = runtime.make_store(p)
        ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
        for _ in range(2):
            st = ex.step()
        assert st.param_fills > 0
        check(p, ex, store)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    import os
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    config.PRESETS[ALLK] = _register_allk()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        res = {"rank": rank, "sends": 0, "ok": 0, "experts": 0}
        for model, check in ((ALLK, _check_allk), ("tiny-mixtral", _check)):
            p = runtime.plan(model, world=world, seq=16, batch=2, placement="expert", **KW)
            store = runtime.make_store(p)
            ex = runtime.make_executor(p, rank, "cpu", store, pg=dist.group.WORLD)
            for _ in range(2):
                st = ex.step()
            while runtime.ep_widen_on_overflow(ex, dist.group.WORLD):  # capacity edges that overflowed
                st = ex.step()
            res["experts"] += sum(t.op.kind == "moe_expert" and p.placement[t.id] == rank for t in p.tasks)
            res["sends"] += st.sends
            if p.placement.get("output_projection") == rank:
                check(p, ex, store)
                res["ok"] += 1
        q.put(res)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_expert_parallel():
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
    assert sum(r["ok"] for r in res) == 2 and sum(r["sends"] for r in res) > 0  # both models were checked
    assert all(r["experts"] > 0 for r in res)  # both ranks ran MXFP4 experts
