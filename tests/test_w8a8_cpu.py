"""fp8 activations (act_dtype="fp8") on the CPU: plan / build / CLI arguments, the reference
forward, the CPU paths of the new ops, and the CPU executor backend in the new mode."""
import json

import pytest
import torch
import torch.nn.functional as F

from distributed_llm_scheduler_amd import cli, ops
from distributed_llm_scheduler_amd.models import reference, registry
from distributed_llm_scheduler_amd.parallel import runtime
from distributed_llm_scheduler_amd.parallel.executor import synthetic_tokens

F8 = torch.float8_e4m3fn


# ------------------------------------------------------------------------ plan, build, CLI
@pytest.mark.parametrize("wd", ["bf16", "fp8-experts"])
def test_act_fp8_needs_fp8_weights(wd):
    model = "tiny-mixtral" if wd == "fp8-experts" else "tiny-gpt2"
    runtime.plan(model, seq=16, weight_dtype=wd)  # fine without fp8 activations
    with pytest.raises(ValueError, match="act_dtype"):
        runtime.plan(model, seq=16, weight_dtype=wd, act_dtype="fp8")
    with pytest.raises(ValueError, match="act_dtype"):
        registry.build(model, seq=16, weight_dtype=wd, act_dtype="fp8")


def test_unknown_act_dtype_is_refused():
    with pytest.raises(ValueError, match="act_dtype"):
        runtime.plan("tiny-gpt2", seq=16, weight_dtype="fp8", act_dtype="int8")
    with pytest.raises(ValueError, match="act_dtype"):
        registry.build("tiny-gpt2", seq=16, weight_dtype="fp8", act_dtype="fp16")
    registry.build("tiny-gpt2", seq=16, weight_dtype="fp8", act_dtype="fp8")


def test_plan_args_save_and_resume(tmp_path):
    p0 = runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="fp8")
    assert "act_dtype" not in p0.args  # only when not the default
    p = runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="fp8", act_dtype="fp8")
    assert p.args["act_dtype"] == "fp8"
    # the DAG, the bytes and the placement are those of fp8 storage
    assert p.order == p0.order and p.param_bytes == p0.param_bytes
    path, path0 = str(tmp_path / "a8.json"), str(tmp_path / "a16.json")
    runtime.save_plan(p, path)
    runtime.save_plan(p0, path0)
    assert json.load(open(path))["args"]["act_dtype"] == "fp8"
    assert "act_dtype" not in json.load(open(path0))["args"]
    q = runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="fp8", act_dtype="fp8", resume=path)
    assert q.order == p.order and q.args["act_dtype"] == "fp8"
    with pytest.raises(ValueError):  # saved fp8 activations, resumed bf16
        runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="fp8", resume=path)
    with pytest.raises(ValueError):  # saved bf16 activations, resumed fp8
        runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="fp8", act_dtype="fp8", resume=path0)
    q0 = runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="fp8", act_dtype="bf16", resume=path0)
    assert q0.order == p0.order


def test_cli_plan_and_run_carry_act_dtype(capsys):
    assert cli.main(["plan", "--model", "tiny-gpt2", "--seq", "16", "--weight-dtype", "fp8", "--act-dtype", "fp8"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["act_dtype"] == "fp8" and out["weight_dtype"] == "fp8" and out["tasks_completed"] == out["tasks_total"]
    assert cli.main(["plan", "--model", "tiny-gpt2", "--seq", "16", "--weight-dtype", "fp8"]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["act_dtype"] == "bf16"
    with pytest.raises(ValueError, match="act_dtype"):
        cli.main(["plan", "--model", "tiny-gpt2", "--seq", "16", "--act-dtype", "fp8"])
    assert cli.main(["run", "--device", "cpu", "--model", "tiny-gpt2", "--seq", "16", "--steps", "1", "--warmup", "0",
                     "--weight-dtype", "fp8", "--act-dtype", "fp8"]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["act_dtype"] == "fp8" and res["valid"]


# ------------------------------------------------------------------------------ reference
def _qdq(x):
    q, s = ops.quantize_fp8(x.reshape(-1, x.shape[-1]))
    return ops.dequantize_fp8(q, s, torch.float32).reshape(x.shape)


def _gpt2_by_hand(cfg, store, tok):
    """GPT-2 forward with every GEMM input on a quantised weight quantise-dequantised per row
    (the tied LM head's wte is stored bf16: its input stays as it is)."""
    w = lambda n: store.tensor(n).float()
    B, S = tok.shape
    H, nh, D = cfg.n_embd, cfg.n_head, cfg.head_dim
    x = w("wte")[tok.long()] + w("wpe")[:S][None]
    for i in range(cfg.n_layer):
        p = f"h.{i}."
        h = F.layer_norm(x, (H,), w(p + "ln_1.weight"), w(p + "ln_1.bias"), cfg.norm_eps)
        qkv = _qdq(h) @ w(p + "attn.c_attn.weight").t() + w(p + "attn.c_attn.bias")
        a = reference._attn(qkv[..., :H], qkv[..., H:2 * H], qkv[..., 2 * H:], nh, nh, D)
        x = x + _qdq(a) @ w(p + "attn.c_proj.weight").t() + w(p + "attn.c_proj.bias")
        h = F.layer_norm(x, (H,), w(p + "ln_2.weight"), w(p + "ln_2.bias"), cfg.norm_eps)
        h = F.gelu(_qdq(h) @ w(p + "mlp.c_fc.weight").t() + w(p + "mlp.c_fc.bias"), approximate="tanh")
        x = x + _qdq(h) @ w(p + "mlp.c_proj.weight").t() + w(p + "mlp.c_proj.bias")
    x = F.layer_norm(x, (H,), w("ln_f.weight"), w("ln_f.bias"), cfg.norm_eps)
    return x @ w("wte").t()


def test_reference_fp8_activations_by_hand():
    p = runtime.plan("mini-gpt2", world=1, seq=32, batch=2, weight_dtype="fp8")
    store = runtime.make_store(p)
    assert not store.is_quantized("wte") and store.is_quantized("h.0.attn.c_attn.weight")
    tok = synthetic_tokens("@tokens", 64, p.cfg.vocab_size).view(2, 32)
    got = reference.forward(p.cfg, store, tok, act_dtype="fp8")
    assert torch.equal(got, _gpt2_by_hand(p.cfg, store, tok))
    base = reference.forward(p.cfg, store, tok)
    assert torch.equal(base, reference.forward(p.cfg, store, tok, act_dtype="bf16"))
    assert not torch.equal(got, base)
    with pytest.raises(ValueError):
        reference.forward(p.cfg, store, tok, act_dtype="int8")


@pytest.mark.parametrize("model", ["mini-gpt2", "mini-llama"])
def test_reference_default_is_unchanged_and_bf16_store_ignores_the_mode(model):
    """The default output is the straight-line forward's; with a store that holds nothing
    quantised the fp8 mode has nothing to act on."""
    p = runtime.plan(model, world=1, seq=16)
    store = runtime.make_store(p)
    tok = synthetic_tokens("@tokens", 16, p.cfg.vocab_size).view(1, 16)
    base = reference.forward(p.cfg, store, tok)
    fam = reference.gpt2_forward if p.cfg.family == "gpt2" else reference.llama_forward
    assert torch.equal(base, fam(p.cfg, store, tok))
    assert torch.equal(base, reference.forward(p.cfg, store, tok, act_dtype="fp8"))


# -------------------------------------------------------------------------------- CPU ops
def _crafted_rows():
    """Rows at scale 1 (one element is 448) unless said otherwise; every value is a bf16 value."""
    K = 32
    rows, want_scale = [], []

    def row(vals, scale=1.0, anchor=True):
        r = torch.zeros(K)
        r[:len(vals)] = torch.tensor(vals, dtype=torch.float32)
        if anchor:
            r[K - 1] = 448.0
        rows.append(r)
        want_scale.append(scale)

    row([], anchor=False)
    row([448.0 * 2 ** 5], scale=2.0 ** 5, anchor=False)
    row([450.0 * 2 ** 5], scale=2.0 ** 6, anchor=False)
    row([-448.0 * 2 ** -20], scale=2.0 ** -20, anchor=False)
    row([17.0, 19.0, -17.0, -19.0, 21.0, 23.0])
    row([0.0009765625 * k for k in range(1, 17)])
    row([2.0 ** -11, -(2.0 ** -11), 2.0 ** -12, 2.0 ** -10 * 0.9921875, 2.0 ** -10 * 1.0078125, -(2.0 ** -30)])
    x = torch.stack(rows).to(torch.bfloat16)
    assert torch.equal(x.float(), torch.stack(rows))
    return x, torch.tensor(want_scale)


def test_quantize_rows_cpu_crafted():
    x, want_scale = _crafted_rows()
    q, s = ops.quantize_rows_fp8(x)
    qh, sh = ops.quantize_fp8(x)
    assert q.dtype == F8 and torch.equal(q.view(torch.uint8), qh.view(torch.uint8)) and torch.equal(s, sh)
    assert torch.equal(s, want_scale)
    v = q.float()
    assert (v[0] == 0).all()
    assert v[1, 0] == 448.0 and v[2, 0] == 224.0 and v[3, 0] == -448.0
    assert v[4, :6].tolist() == [16.0, 20.0, -16.0, -20.0, 20.0, 24.0]  # ties to even
    assert v[5, :16].tolist() == [round(k / 2) * 2.0 ** -9 for k in range(1, 17)]  # subnormal ties
    assert v[6, :6].tolist() == [0.0, 0.0, 0.0, 0.0, 2.0 ** -9, 0.0]
    # caller's outputs (uint8 scratch as the executor passes it), and a 3-D input
    oq, osc = torch.zeros(x.shape, dtype=torch.uint8), torch.zeros(x.shape[0])
    q2, s2 = ops.quantize_rows_fp8(x, oq, osc)
    assert q2.dtype == F8 and q2.data_ptr() == oq.data_ptr() and s2 is osc
    assert torch.equal(oq, qh.view(torch.uint8)) and torch.equal(osc, sh)
    x3 = x[:6].reshape(2, 3, -1)
    q3, s3 = ops.quantize_rows_fp8(x3)
    assert q3.shape == x3.shape and s3.shape == (6,)
    assert torch.equal(q3.view(torch.uint8).reshape(6, -1), qh[:6].view(torch.uint8))


@pytest.mark.parametrize("kind", ["layernorm", "rmsnorm"])
def test_norm_q8_cpu_is_the_composition(kind):
    g = torch.Generator().manual_seed(1)
    x, r = torch.randn(9, 64, generator=g).bfloat16(), torch.randn(9, 64, generator=g).bfloat16()
    w, b = torch.randn(64, generator=g).bfloat16(), torch.randn(64, generator=g).bfloat16()
    if kind == "layernorm":
        norm = lambda **kw: ops.layernorm(x, w, b, 1e-5, **kw)
        fused = lambda **kw: ops.layernorm_q8(x, w, b, 1e-5, **kw)
    else:
        norm = lambda **kw: ops.rmsnorm(x, w, 1e-5, **kw)
        fused = lambda **kw: ops.rmsnorm_q8(x, w, 1e-5, **kw)
    q, s = fused()
    qh, sh = ops.quantize_fp8(norm())
    assert torch.equal(q.view(torch.uint8), qh.view(torch.uint8)) and torch.equal(s, sh)
    y, sm = norm(residual=r)
    so = torch.empty_like(x)
    q, s, sm2 = fused(residual=r, sum_out=so)
    qh, sh = ops.quantize_fp8(y)
    assert torch.equal(q.view(torch.uint8), qh.view(torch.uint8)) and torch.equal(s, sh)
    assert torch.equal(sm2, sm) and torch.equal(so, sm)


def test_linear_w8a8_cpu_follows_the_definition():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(10, 64, generator=g).to(torch.bfloat16)
    w = (0.05 * torch.randn(64, 64, generator=g)).to(torch.bfloat16)
    b = torch.randn(64, generator=g).to(torch.bfloat16)
    r = torch.randn(10, 64, generator=g).to(torch.bfloat16)
    q, s = ops.quantize_fp8(w)
    xq, xs = ops.quantize_rows_fp8(x)
    xs = xs * 3.0  # any positive scales
    xd, wd = xq.float() * xs[:, None], q.float() * s[:, None]
    for act in (None, "gelu", "silu", "relu"):
        y = ops.linear_w8a8(xq, xs, q, s, b, act=act, residual=r, alpha=0.5)
        assert y.dtype == torch.bfloat16
        assert torch.equal(y, ops.ref_linear(xd, wd, b, act, r, 0.5).to(torch.bfloat16))
    qi, si = ops.interleave_gate_up(q.view(torch.uint8)).view(F8), ops.interleave_gate_up(s)
    y = ops.linear_w8a8(xq, xs, qi, si, act="swiglu")
    assert y.shape == (10, 32)
    assert torch.equal(y, ops.ref_linear(xd, ops.interleave_gate_up(wd), act="swiglu").to(torch.bfloat16))
    out = torch.zeros(10, 80, dtype=torch.bfloat16)[:, 8:72]
    assert ops.linear_w8a8(xq, xs, q, s, out=out) is out
    assert torch.equal(out, (xd @ wd.t()).to(torch.bfloat16))
    with pytest.raises((ValueError, RuntimeError), match="16"):
        ops.linear_w8a8(xq[:, :40].contiguous(), xs, q[:, :40].contiguous(), s)
    with pytest.raises(TypeError):
        ops.linear_w8a8(x, xs, q, s)
    with pytest.raises(TypeError):
        ops.linear_w8a8(xq, xs, w, s)


# --------------------------------------------------------------------------- CPU executor
# (max-abs error / max |logit|, rms-relative error) of the CPU executor backend with
# act_dtype="fp8" against reference.forward(act_dtype="fp8") at seq=64, batch=2, as measured:
# an activation that differs by one bf16 step upstream (the executor keeps activations in bf16,
# the reference in fp32) can flip an e4m3 rounding by a whole fp8 step, so this is far noisier
# than the W8A16 comparison (0.005 on the same models). Both backends are held to 2 x these.
EXEC_CPU = {"mini-gpt2": (0.0595, 0.0528), "mini-llama": (0.0711, 0.0605)}


def _measures(out, ref):
    d = out - ref
    return d.abs().max().item() / ref.abs().max().item(), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


@pytest.mark.parametrize("model", ["mini-gpt2", "mini-llama"])
def test_cpu_executor_fp8_activations(model, capsys):
    p = runtime.plan(model, world=1, seq=64, batch=2, weight_dtype="fp8", act_dtype="fp8")
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store)
    ex.step()
    out = ex.output("output_projection").float()
    tok = synthetic_tokens("@tokens", 128, p.cfg.vocab_size).view(2, 64)
    ref8 = reference.forward(p.cfg, store, tok, act_dtype="fp8")
    maxrel, rmsrel = _measures(out, ref8)
    # reported, not gated: what fp8 activations cost against the W8A16 reference
    ref16 = reference.forward(p.cfg, store, tok)
    d = ref8 - ref16
    top1 = (ref8.argmax(-1) == ref16.argmax(-1)).float().mean().item()
    with capsys.disabled():
        print(f"\n{model}: executor vs fp8-activation reference: max {maxrel:.4f} rms {rmsrel:.4f}; "
              f"fp8-activation vs W8A16 reference: max logit diff {d.abs().max().item():.4f}, "
              f"rms-relative {_measures(ref8, ref16)[1]:.4f}, top-1 agreement {top1:.3f}")
    cmax, crms = EXEC_CPU[model]
    assert maxrel <= 2 * cmax and rmsrel <= 2 * crms
    # the mode is on: the W8A16 executor lands elsewhere (close to ITS reference)
    ex16 = runtime.make_executor(runtime.plan(model, world=1, seq=64, batch=2, weight_dtype="fp8"), 0, "cpu", store)
    ex16.step()
    out16 = ex16.output("output_projection").float()
    assert _measures(out16, ref16)[0] < 0.02 and not torch.equal(out16, out)


def test_cpu_executor_fp8_activations_under_cap():
    need = sum(runtime.plan("mini-llama", world=1, seq=64, batch=2, weight_dtype="fp8").param_bytes.values()) / 1e9
    p = runtime.plan("mini-llama", world=1, seq=64, batch=2, weight_dtype="fp8", act_dtype="fp8", cap_gb=0.6 * need)
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
    for _ in range(3):
        st = ex.step()
    assert st.param_fills > 0
    tok = synthetic_tokens("@tokens", 128, p.cfg.vocab_size).view(2, 64)
    maxrel, rmsrel = _measures(ex.output("output_projection").float(), reference.forward(p.cfg, store, tok, act_dtype="fp8"))
    cmax, crms = EXEC_CPU["mini-llama"]
    assert maxrel <= 2 * cmax and rmsrel <= 2 * crms


def test_executor_refuses_fp8_activations_without_fp8_weights():
    p = runtime.plan("tiny-gpt2", world=1, seq=16)
    from distributed_llm_scheduler_amd.parallel.executor import DAGExecutor

    with pytest.raises(ValueError, match="act_dtype"):
        DAGExecutor(p.tasks, p.programs[0], runtime.make_store(p), "cpu", model_cfg=p.cfg, act_dtype="fp8")
