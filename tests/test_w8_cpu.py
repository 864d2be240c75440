"""fp8 weight storage (weight_dtype="fp8") on the CPU: the quantiser, the byte accounting, the
planner's metric under a cap, the CPU executor against the fp32 reference, plans and the CLI."""
import json
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from distributed_llm_scheduler_amd import cli, ops
from distributed_llm_scheduler_amd.models import reference, registry
from distributed_llm_scheduler_amd.models.params import ParamStore, group_layout
from distributed_llm_scheduler_amd.parallel import runtime
from distributed_llm_scheduler_amd.parallel.executor import synthetic_tokens

E4M3_MAX = 448.0


def _weights():
    g = torch.Generator().manual_seed(7)
    w = (0.02 * torch.randn(96, 160, generator=g)).to(torch.bfloat16)
    w[5] = 0                                   # an all-zero row
    w[6] = w[6] * 1e-6                         # a tiny row
    w[7] = (w[7].float() * 3e4).to(torch.bfloat16)  # a large row
    w[8, :] = 0
    w[8, 3] = 448.0                            # amax exactly at the format's maximum
    w[9, :] = 0
    w[9, 4] = -449.0 * 2 ** -10                # just past a power-of-two boundary, negative
    return w


# ---------------------------------------------------------------------------- quantiser
def test_quantizer_scales_are_powers_of_two_and_rows_in_range():
    w = _weights()
    q, scale = ops.quantize_fp8(w)
    assert q.dtype == torch.float8_e4m3fn and q.shape == w.shape
    assert scale.dtype == torch.float32 and scale.shape == (w.shape[0],)
    m, _ = torch.frexp(scale)
    assert torch.equal(m, torch.full_like(m, 0.5)) and (scale > 0).all()
    qf = q.float()
    assert torch.isfinite(qf).all()  # no NaN code
    assert (q.view(torch.uint8) & 0x7F != 0x7F).all()
    assert qf.abs().max() <= E4M3_MAX
    # the smallest power of two that brings the row's amax within range
    amax = w.float().abs().amax(1)
    nz = amax > 0
    assert (amax[nz] / scale[nz] <= E4M3_MAX).all() and (amax[nz] / (scale[nz] / 2) > E4M3_MAX).all()
    # +-amax maps within range and keeps its sign
    i = w.float().abs().argmax(1)
    rows = torch.arange(w.shape[0])
    assert torch.equal(torch.sign(qf[rows, i]), torch.sign(w.float()[rows, i]))


def test_quantizer_zero_row():
    q, scale = ops.quantize_fp8(_weights())
    assert scale[5].item() == 1.0 and (q[5].float() == 0).all()
    assert (ops.dequantize_fp8(q, scale)[5] == 0).all()


def test_quantizer_round_trip_and_error_bound():
    w = _weights()
    q, scale = ops.quantize_fp8(w)
    dq32 = q.float() * scale[:, None]
    dq = ops.dequantize_fp8(q, scale)
    assert dq.dtype == torch.bfloat16
    assert torch.equal(dq.float(), dq32)  # the dequantised weight is exactly a bf16 tensor
    # 3 mantissa bits -> relative 2^-4; subnormal step 2^-9 -> absolute scale * 2^-10
    err = (w.float() - dq32).abs()
    bound = torch.maximum(2.0 ** -4 * w.float().abs(), scale[:, None] * 2.0 ** -10)
    assert (err <= bound).all()
    # quantising the dequantised weight again changes nothing
    q2, s2 = ops.quantize_fp8(dq)
    assert torch.equal(ops.dequantize_fp8(q2, s2), dq)


def test_every_code_times_a_power_of_two_is_bf16():
    codes = torch.arange(256, dtype=torch.uint8)
    codes = codes[(codes & 0x7F) != 0x7F]
    assert codes.numel() == 254
    v = codes.view(torch.float8_e4m3fn).float()
    for e in (-8, 0, 4):
        x = v * 2.0 ** e
        assert torch.equal(x.to(torch.bfloat16).float(), x)


def test_linear_w8_cpu_matches_reference_on_dequantised_weight():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(10, 64, generator=g).to(torch.bfloat16)
    w = (0.05 * torch.randn(64, 64, generator=g)).to(torch.bfloat16)
    b = torch.randn(64, generator=g).to(torch.bfloat16)
    r = torch.randn(10, 64, generator=g).to(torch.bfloat16)
    q, s = ops.quantize_fp8(w)
    for act in (None, "gelu", "silu", "relu"):
        y = ops.linear_w8(x, q, s, b, act=act, residual=r, alpha=0.5)
        assert torch.equal(y, ops.ref_linear(x, ops.dequantize_fp8(q, s), b, act, r, 0.5))
    qi, si = ops.interleave_gate_up(q.view(torch.uint8)).view(torch.float8_e4m3fn), ops.interleave_gate_up(s)
    y = ops.linear_w8(x, qi, si, act="swiglu")
    assert y.shape == (10, 32)
    assert torch.equal(y, ops.ref_linear(x, ops.interleave_gate_up(ops.dequantize_fp8(q, s)), act="swiglu"))
    with pytest.raises((ValueError, RuntimeError)):
        ops.linear_w8(x[:, :40], q[:, :40].contiguous(), s)  # K % 16 != 0


# --------------------------------------------------------------------------------- bytes
def _al(n):
    return (n + 255) // 256 * 256


def test_llama3_8b_fp8_bytes():
    _, g16, _ = registry.build("llama3-8b")
    tasks, g8, cfg = registry.build("llama3-8b", weight_dtype="fp8")
    b16 = {k: group_layout(g)[0] for k, g in g16.items()}
    b8 = {k: group_layout(g)[0] for k, g in g8.items()}
    assert 0.50 < sum(b8.values()) / sum(b16.values()) < 0.54
    assert abs(sum(b8.values()) / 1e9 - 8.56) < 0.01
    quantised = 0
    for pid, grp in g8.items():
        want, offs = 0, []
        for sp in grp.tensors:
            offs.append(want)
            if sp.quant:
                N, K = sp.shape
                want += _al(N * K) + _al(4 * N)
                quantised += 1
            else:
                want += _al(2 * sp.numel)
        assert b8[pid] == want, pid
        assert [o for _, o in group_layout(grp)[1]] == offs
        assert ParamStore(g8).nbytes(pid) == want
        assert grp.nbytes() == sum(s.numel + 4 * s.shape[0] if s.quant else 2 * s.numel for s in grp.tensors)
    # qkv, o, gate_up, down of every layer + the LM head; embedding and norms stay bf16
    assert quantised == 4 * cfg.n_layer + 1
    assert b8["embedding_weights"] == b16["embedding_weights"]
    assert not g8["embedding_weights"].tensors[0].quant and g8["output_weights"].tensors[0].quant
    assert all(not s.quant for pid, g in g8.items() if "norm" in pid for s in g.tensors)


def test_gpt2_tied_wte_and_biases_stay_bf16():
    _, g16, _ = registry.build("gpt2")
    _, g8, cfg = registry.build("gpt2", weight_dtype="fp8")
    for pid in ("embedding_weights", "position_weights", "final_ln_weights", "layer_0_ln1_weights"):
        assert group_layout(g8[pid])[0] == group_layout(g16[pid])[0]
        assert all(not s.quant for s in g8[pid].tensors)
    for pid, g in g8.items():
        for s in g.tensors:
            assert s.quant == (len(s.shape) == 2 and s.name not in ("wte", "wpe")), s.name
    H = cfg.n_embd
    assert group_layout(g8["layer_0_attn_qkv_weights"])[0] == _al(3 * H * H) + _al(4 * 3 * H) + _al(2 * 3 * H)
    assert abs(sum(group_layout(g)[0] for g in g8.values()) / 1e9 - 0.164) < 0.001


@pytest.mark.parametrize("model", ["gpt2", "llama3-8b", "mixtral-8x7b", "tiny-gpt2", "mini-llama"])
def test_bf16_sizes_unchanged(model):
    _, g, _ = registry.build(model, weight_dtype="bf16")
    _, g0, _ = registry.build(model)
    for pid, grp in g.items():
        assert all(not s.quant for s in grp.tensors)
        want = sum(_al(2 * s.numel) for s in grp.tensors)  # the layout before fp8 storage existed
        assert group_layout(grp)[0] == group_layout(g0[pid])[0] == want
        assert grp.nbytes() == 2 * sum(s.numel for s in grp.tensors)


# --------------------------------------------------------------------- the project's metric
def test_llama3_8b_under_a_10_3_gb_cap():
    kw = dict(world=1, cap_gb=10.3, cost_model="bytes")
    dfs16 = runtime.plan("llama3-8b", scheduler="DFS", **kw)
    eft16 = runtime.plan("llama3-8b", scheduler="EFT", **kw)
    assert (dfs16.completed, dfs16.total) == (128, 195)
    assert (eft16.completed, eft16.total) == (195, 195)
    assert abs(eft16.stats["refill_gb_per_step_per_rank"][0] - 6.04) < 0.01
    dfs8 = runtime.plan("llama3-8b", scheduler="DFS", weight_dtype="fp8", **kw)
    eft8 = runtime.plan("llama3-8b", scheduler="EFT", weight_dtype="fp8", **kw)
    assert (dfs8.completed, dfs8.total) == (195, 195)
    assert (eft8.completed, eft8.total) == (195, 195)
    assert eft8.stats["refill_gb_per_step_per_rank"][0] == 0.0
    assert dfs8.stats["refill_gb_per_step_per_rank"][0] == 0.0


# ------------------------------------------------------------------------- CPU executor
def _ref_check(p, ex, store, rid=""):
    out = ex.output(f"{rid}output_projection").float()
    B, S = out.shape[0], out.shape[1]
    tok = synthetic_tokens(f"{rid}@tokens", B * S, p.cfg.vocab_size).view(B, S)
    ref = reference.forward(p.cfg, store, tok)
    return (out - ref).abs().max().item(), ref.abs().max().item()


MODELS = ["tiny-gpt2", "tiny-llama", "mini-gpt2", "mini-llama"]


@pytest.mark.parametrize("model", MODELS)
def test_cpu_executor_fp8_matches_reference(model):
    p = runtime.plan(model, world=1, seq=32, batch=2, weight_dtype="fp8")
    assert p.completed == p.total
    store = runtime.make_store(p)
    names = [s.name for g in p.groups.values() for s in g.tensors if s.quant]
    assert names
    q, scale = store.quantized(names[0])
    assert q.dtype == torch.float8_e4m3fn
    assert torch.equal(store.tensor(names[0]), ops.dequantize_fp8(q, scale))
    ex = runtime.make_executor(p, 0, "cpu", store)
    ex.step()
    err, scale_ = _ref_check(p, ex, store)
    assert err < 0.02 * scale_
    # no folded norm, no row statistics, no post-norm around an fp8 GEMM
    assert not ex._post_norm and not ex._stats_out


@pytest.mark.parametrize("sched", ["EFT", "MRU_spec"])
@pytest.mark.parametrize("model", MODELS)
def test_cpu_executor_fp8_under_cap(model, sched):
    """0.6 x the fp8 need: groups are evicted and re-filled as mixed bf16 / e4m3 / fp32 byte
    images, the SwiGLU interleave of (q, scale) persisted into the image."""
    need = sum(runtime.plan(model, world=1, seq=16, weight_dtype="fp8").param_bytes.values()) / 1e9
    p = runtime.plan(model, world=1, seq=16, weight_dtype="fp8", cap_gb=0.6 * need, scheduler=sched)
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
    for _ in range(3):
        st = ex.step()
    assert st.param_fills > 0
    err, scale = _ref_check(p, ex, store)
    assert err < 0.02 * scale


def test_set_tensor_quantises():
    p = runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="fp8")
    store = runtime.make_store(p)
    name = "layers.0.attention.wo"
    w = (0.05 * torch.randn(store._spec(name).shape)).to(torch.bfloat16)
    store.set_tensor(name, w)
    q, s = ops.quantize_fp8(w)
    assert torch.equal(store.quantized(name)[0].view(torch.uint8), q.view(torch.uint8))
    assert torch.equal(store.tensor(name), ops.dequantize_fp8(q, s))
    ex = runtime.make_executor(p, 0, "cpu", store)
    ex.step()
    err, scale = _ref_check(p, ex, store)
    assert err < 0.02 * scale


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
        p = runtime.plan("tiny-llama", world=world, seq=16, replicas=2, placement="pipeline", weight_dtype="fp8")
        store = runtime.make_store(p)
        ex = runtime.make_executor(p, rank, "cpu", store, pg=dist.group.WORLD)
        for _ in range(2):
            st = ex.step()
        errs = [_ref_check(p, ex, store, rid) for rid in ("r0/", "r1/")
                if p.placement.get(f"{rid}output_projection") == rank]
        q.put({"rank": rank, "sends": st.sends, "errs": errs})
    finally:
        dist.destroy_process_group()


def test_two_rank_pipeline_fp8():
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
    errs = [e for r in res for e in r["errs"]]
    assert len(errs) == 2 and sum(r["sends"] for r in res) > 0
    for err, scale in errs:
        assert err < 0.02 * scale


# ---------------------------------------------------------------------------------- plans
def test_fp8_plan_saves_and_resumes(tmp_path):
    path = str(tmp_path / "plan.json")
    p = runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="fp8")
    assert p.args["weight_dtype"] == "fp8"
    runtime.save_plan(p, path)
    q = runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="fp8", resume=path)
    assert q.order == p.order and q.param_bytes == p.param_bytes
    with pytest.raises(ValueError):  # saved fp8, resumed bf16
        runtime.plan("tiny-llama", world=1, seq=16, resume=path)


def test_plan_saved_without_the_key_resumes_with_the_default(tmp_path):
    path = str(tmp_path / "plan.json")
    p = runtime.plan("tiny-llama", world=1, seq=16)
    assert "weight_dtype" not in p.args  # as sp / merge_mb: only when not the default
    runtime.save_plan(p, path)
    assert "weight_dtype" not in json.load(open(path))["args"]
    q = runtime.plan("tiny-llama", world=1, seq=16, resume=path)
    assert q.order == p.order
    q = runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="bf16", resume=path)
    assert q.order == p.order
    with pytest.raises(ValueError):  # saved bf16, resumed fp8
        runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="fp8", resume=path)


@pytest.mark.parametrize("kw", [dict(model="tiny-mixtral"), dict(model="tiny-llama", tp=2, placement="tensor", world=2),
                                dict(model="tiny-llama", sp=2, placement="sequence", world=2)])
def test_fp8_refused_where_it_is_not_built(kw):
    kw = dict(kw)
    model = kw.pop("model")
    runtime.plan(model, seq=16, **kw)  # the same plan in bf16 is fine
    with pytest.raises(ValueError):
        runtime.plan(model, seq=16, weight_dtype="fp8", **kw)
    with pytest.raises(ValueError):
        runtime.plan("tiny-gpt2", seq=16, weight_dtype="int8")


def test_cli_plan_and_run_fp8(capsys):
    assert cli.main(["plan", "--model", "tiny-gpt2", "--seq", "16", "--weight-dtype", "fp8"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["weight_dtype"] == "fp8" and out["tasks_completed"] == out["tasks_total"] == 19
    assert cli.main(["plan", "--model", "tiny-gpt2", "--seq", "16"]) == 0
    out16 = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out16["weight_dtype"] == "bf16" and out["param_gb"] < out16["param_gb"]
    assert cli.main(["run", "--device", "cpu", "--model", "tiny-gpt2", "--seq", "16", "--steps", "1", "--warmup", "0",
                     "--weight-dtype", "fp8"]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["weight_dtype"] == "fp8" and res["tasks_completed"] == 19 and res["param_gb"] == out["param_gb"]
