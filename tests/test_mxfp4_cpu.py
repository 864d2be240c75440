"""MXFP4 weight storage without a GPU: the host quantiser on crafted blocks, the packing, the
group layout, the argument checks, ``ops.linear_w4a8`` on CPU and the CPU-backend executor with
``weight_dtype="mxfp4", act_dtype="fp8"``."""
import json

import pytest
import torch
import torch.nn.functional as F

from distributed_llm_scheduler_amd import cli, ops
from distributed_llm_scheduler_amd.models import reference, registry
from distributed_llm_scheduler_amd.models.params import (ParamGroup, ParamStore, TensorSpec, group_layout,
                                                          quant_parts)
from distributed_llm_scheduler_amd.parallel import runtime
from distributed_llm_scheduler_amd.parallel.executor import DAGExecutor, synthetic_tokens

BF = torch.bfloat16
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _nib(q, k):
    """e2m1 code of element k of every row of packed bytes q [N, K/2]."""
    return (q[:, k // 2] >> (4 * (k % 2))) & 15


def _block(vals, fill=0.0):
    """One row of one 32-element block starting with ``vals``."""
    return torch.tensor([list(vals) + [fill] * (32 - len(vals))], dtype=torch.float32).to(BF)


# ------------------------------------------------------------------------ crafted blocks
def test_all_zero_block():
    q, s = ops.quantize_mxfp4(torch.zeros(3, 64, dtype=BF))
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8 and q.shape == (3, 32) and s.shape == (3, 2)
    assert (s == 127).all() and (q == 0).all()


@pytest.mark.parametrize("e", [-20, -3, 0, 1, 10])
def test_amax_at_and_just_above_six(e):
    """amax = 6 * 2^e takes scale 2^e and code 7; one bf16 step above (6 * (1 + 2^-7)) no longer
    fits and doubles the scale (3.02 rounds to 3: code 5)."""
    at = _block([6.0 * 2.0 ** e])
    q, s = ops.quantize_mxfp4(at)
    assert s[0, 0].item() == 127 + e and _nib(q, 0).item() == 7
    above = _block([6.0 * 2.0 ** e * (1 + 2.0 ** -7)])
    assert above[0, 0].float().item() > at[0, 0].float().item()
    q, s = ops.quantize_mxfp4(above)
    assert s[0, 0].item() == 127 + e + 1 and _nib(q, 0).item() == 5


def test_ties_to_even_signs_and_saturation():
    """Under a 6.0 anchor (scale 2^0) the midpoints go to the even code: 0.25 -> 0, 0.75 -> 1,
    1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4; negative values mirror them with bit 3."""
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    # the last two: one bf16 step above a tie
    w = _block([6.0] + ties + [-t for t in ties] + [-6.0, 0.5, -0.5, 3.0, -3.0, 0.251953125, 5.03125])
    q, s = ops.quantize_mxfp4(w)
    assert s[0, 0].item() == 127
    d = ops.dequantize_mxfp4(q, s, torch.float32)[0]
    assert d[:22].tolist() == [6.0] + want + [-v for v in want] + [-6.0, 0.5, -0.5, 3.0, -3.0, 0.5, 6.0]
    for i in range(7):  # the sign is bit 3 of the code
        assert _nib(q, 8 + i).item() == _nib(q, 1 + i).item() | 8
    assert _nib(q, 15).item() == 15 and _nib(q, 0).item() == 7


def test_blocks_of_one_row_span_2_to_the_minus_20_to_10():
    """Every block has its own scale: a row whose 31 blocks have amax 1.5 * 2^-20 .. 1.5 * 2^10."""
    es = list(range(-20, 11))
    w = torch.cat([_block([1.5 * 2.0 ** e, -0.5 * 2.0 ** e]) for e in es], 1)
    q, s = ops.quantize_mxfp4(w)
    # 1.5 = 0.75 * 2^1: e = ex - 3 = -2, i.e. 1.5 * 2^e is stored as 6 * 2^(e - 2)
    assert s[0].tolist() == [127 + e - 2 for e in es]
    assert all(_nib(q, 32 * b).item() == 7 and _nib(q, 32 * b + 1).item() == 8 + 4 for b in range(len(es)))
    assert torch.equal(ops.dequantize_mxfp4(q, s), w)  # all of it representable


def test_exponent_clamp():
    """e is clamped to [-127, 127] (codes 0..254; 255 is never written). bf16's smallest values
    need e below -127: the clamp keeps code 0 and the values round on its grid; its largest need
    no more than 125."""
    tiny = 2.0 ** -133  # the smallest bf16 subnormal: amax / 2^e <= 6 would want e = -135
    w = _block([tiny, 2.0 ** -128, -(2.0 ** -127)])
    q, s = ops.quantize_mxfp4(w)
    assert s[0, 0].item() == 0
    assert ops.dequantize_mxfp4(q, s, torch.float32)[0, :3].tolist() == [0.0, 2.0 ** -128, -(2.0 ** -127)]
    big = _block([torch.finfo(BF).max, -1.0])
    q, s = ops.quantize_mxfp4(big)
    # 3.39e38 = 0.996 * 2^128: e = 128 - 2 = 126 and 3.98 rounds to 4 (code 6)
    assert s[0, 0].item() == 127 + 126 and (s < 255).all() and _nib(q, 0).item() == 6


# ------------------------------------------------------------------------------- round trip
def _weights(N=96, K=416, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (0.02 * torch.randn(N, K, generator=g)).to(BF)


def test_round_trip():
    """dequantize(quantize(w)) is exactly bf16 (the fp32 and the bf16 result agree), within half
    a grid step of w, and a fixed point of the quantiser's VALUES. The bytes repeat for every
    block whose largest code is 4 or 6; a block whose amax rounded down to 3 * 2^e is, by the
    scale rule (the smallest 2^e with amax / 2^e <= 6), re-quantised as 6 * 2^(e - 1): the same
    values, one scale code lower with doubled elements."""
    w = _weights()
    q, s = ops.quantize_mxfp4(w)
    d32, d16 = ops.dequantize_mxfp4(q, s, torch.float32), ops.dequantize_mxfp4(q, s)
    assert d16.dtype == BF and torch.equal(d16.float(), d32)
    step = torch.ldexp(torch.ones(s.shape), (s.int() - 127)).repeat_interleave(32, 1)  # 2^e; grid step <= 2 * 2^e
    assert ((d32 - w.float()).abs() <= step).all()
    q2, s2 = ops.quantize_mxfp4(d16)
    assert torch.equal(ops.dequantize_mxfp4(q2, s2), d16)
    top = (torch.maximum(q & 7, (q >> 4) & 7)).reshape(q.shape[0], -1, 16).amax(2)  # largest |code| per block
    keep = top >= 6  # codes 6, 7: values 4 and 6
    assert keep.any() and (~keep).any()
    assert torch.equal(s2[keep], s[keep])
    assert torch.equal(q2.reshape(q.shape[0], -1, 16)[keep], q.reshape(q.shape[0], -1, 16)[keep])
    assert torch.equal(s2[~keep & (top > 0)], s[~keep & (top > 0)] - 1)
    q3, s3 = ops.quantize_mxfp4(ops.dequantize_mxfp4(q2, s2))  # from there on the bytes repeat
    assert torch.equal(q3, q2) and torch.equal(s3, s2)


def test_packing_and_scale_index():
    """Element k of a row is the low nibble of byte k/2 for even k, the high nibble for odd k;
    block b of row n scales elements 32b .. 32b+31 of that row."""
    codes = (torch.arange(4)[:, None] * 5 + torch.arange(64)[None, :] * 3) % 16
    q = (codes[:, 0::2] | (codes[:, 1::2] << 4)).to(torch.uint8)
    s = torch.tensor([[127, 130], [120, 127], [126, 128], [127, 127]], dtype=torch.uint8)
    d = ops.dequantize_mxfp4(q, s, torch.float32)
    for n in range(4):
        for k in range(64):
            c = codes[n, k].item()
            want = (-1.0 if c & 8 else 1.0) * E2M1[c & 7] * 2.0 ** (s[n, k // 32].item() - 127)
            assert d[n, k].item() == want, (n, k)
    w = torch.zeros(1, 64, dtype=BF)
    w[0, 0], w[0, 1], w[0, 33] = 1.0, -3.0, 0.5
    q, s = ops.quantize_mxfp4(w)
    assert q[0, 0].item() == (4 | ((8 | 7) << 4))  # scale 2^-1: 1 -> 2 (code 4), -3 -> -6 (code 15)
    # block 1: 0.5 = 4 * 2^-3 (2^-4 would need 8), element 33 is the high nibble of byte 16
    assert s[0].tolist() == [126, 124] and q[0, 16].item() == 6 << 4 and (q[0, 1:16] == 0).all()
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.quantize_mxfp4(torch.zeros(2, 48, dtype=BF))


# ----------------------------------------------------------------------------------- layout
def _mixed_store():
    specs = [TensorSpec("g.bias", (48,), init="bias"),
             TensorSpec("g.w8", (48, 80), quant=True),
             TensorSpec("g.w4", (40, 96), quant=True, qfmt="mxfp4"),
             TensorSpec("g.ln", (96,), init="ln")]
    grp = ParamGroup("g", specs)
    return grp, ParamStore({"g": grp}, pin=False)


def test_layout_of_a_mixed_group():
    grp, store = _mixed_store()
    assert quant_parts(grp.tensors[1]) == (48 * 80, 3840, 4 * 48)
    assert quant_parts(grp.tensors[2]) == (40 * 96 // 2, 2048, 40 * 96 // 32)  # 1920 data bytes, scales at 2048
    assert grp.nbytes() == 48 * 2 + (48 * 80 + 4 * 48) + (1920 + 120) + 96 * 2
    total, layout = group_layout(grp)
    assert [off for _, off in layout] == [0, 256, 256 + 3840 + 256, 256 + 3840 + 256 + 2048 + 256]
    assert total == layout[-1][1] + 256 and store.nbytes("g") == total
    assert all(sp.quant for sp in grp.tensors[1:3]) and store.quant_format("g.w4") == "mxfp4"
    assert store.quant_format("g.w8") == "fp8" and store.quant_format("g.ln") is None


def test_group_image_and_set_tensor():
    grp, store = _mixed_store()
    q, s = store.quantized("g.w4")
    assert q.dtype == torch.uint8 and q.shape == (40, 48) and s.shape == (40, 3)
    assert torch.equal(store.tensor("g.w4"), ops.dequantize_mxfp4(q, s)) and store.tensor("g.w4").dtype == BF
    img = store.group_image("g")
    off = dict((sp.name, o) for sp, o in group_layout(grp)[1])["g.w4"]
    assert torch.equal(img[off:off + 1920], q.reshape(-1))
    assert torch.equal(img[off + 2048:off + 2048 + 120], s.reshape(-1))
    assert (img[off + 1920:off + 2048] == 0).all()
    q8, s8 = store.quantized("g.w8")
    off8 = dict((sp.name, o) for sp, o in group_layout(grp)[1])["g.w8"]
    assert torch.equal(img[off8:off8 + 3840], q8.view(torch.uint8).reshape(-1))
    new = _weights(40, 96, seed=3)
    store.set_tensor("g.w4", new)
    qn, sn = ops.quantize_mxfp4(new)
    assert torch.equal(store.quantized("g.w4")[0], qn) and torch.equal(store.quantized("g.w4")[1], sn)
    img2 = store.group_image("g")  # the old image was dropped
    assert img2 is not img and torch.equal(img2[off:off + 1920], qn.reshape(-1))
    out_q, out_s = torch.empty(40, 48, dtype=torch.uint8), torch.empty(40, 3, dtype=torch.uint8)
    store.fill("g.w4", out_q, out_s)
    assert torch.equal(out_q, qn) and torch.equal(out_s, sn)


# ---------------------------------------------------------------------------- argument checks
def test_value_errors():
    registry.build("tiny-gpt2", seq=16, weight_dtype="mxfp4", act_dtype="fp8")
    with pytest.raises(ValueError, match="MoE"):
        registry.build("tiny-mixtral", seq=16, weight_dtype="mxfp4", act_dtype="fp8")
    with pytest.raises(ValueError, match="parallelism"):
        registry.build("tiny-gpt2", seq=16, weight_dtype="mxfp4", act_dtype="fp8", tp=2)
    with pytest.raises(ValueError, match="parallelism"):
        registry.build("tiny-gpt2", seq=16, weight_dtype="mxfp4", act_dtype="fp8", sp=2)
    with pytest.raises(ValueError, match="W4A8"):
        registry.build("tiny-gpt2", seq=16, weight_dtype="mxfp4", act_dtype="bf16")
    with pytest.raises(ValueError, match="W4A8"):
        runtime.plan("tiny-gpt2", seq=16, weight_dtype="mxfp4", act_dtype="bf16")
    with pytest.raises(ValueError, match="W4A8"):
        runtime.plan("tiny-gpt2", seq=16, weight_dtype="mxfp4")  # the default activations are bf16
    registry.check_act_dtype("fp8", "fp8")
    registry.check_act_dtype("fp8", "mxfp4")
    with pytest.raises(ValueError, match="weight_dtype"):
        runtime.plan("tiny-gpt2", seq=16, weight_dtype="mxfp6", act_dtype="fp8")
    # the accepted values: the earlier three, unchanged, and the block-scaled format next to them
    assert registry.MX_WEIGHT_DTYPES == ("mxfp4",) and "mxfp4" not in registry.WEIGHT_DTYPES


def test_marked_k_must_be_a_multiple_of_32():
    """No registered model has such a weight, so one of tiny-gpt2's GEMM weights is widened by 16."""
    tasks, groups, _ = registry.build("tiny-gpt2", seq=16, weight_dtype="fp8")
    sp = next(sp for g in groups.values() for sp in g.tensors if sp.quant)
    tasks, groups, _ = registry.build("tiny-gpt2", seq=16)
    sp = next(t for g in groups.values() for t in g.tensors if t.name == sp.name)
    sp.shape = (sp.shape[0], sp.shape[1] + 16)
    with pytest.raises(ValueError, match="multiple of 32"):
        registry.mark_fp8(tasks, groups, fmt="mxfp4")
    assert not any(t.quant for g in groups.values() for t in g.tensors if t.name == sp.name)


def test_marks_what_fp8_marks():
    for model in ("tiny-gpt2", "tiny-llama"):
        _, g8, _ = registry.build(model, seq=16, weight_dtype="fp8")
        _, g4, _ = registry.build(model, seq=16, weight_dtype="mxfp4", act_dtype="fp8")
        m8 = {sp.name for g in g8.values() for sp in g.tensors if sp.quant}
        m4 = {sp.name for g in g4.values() for sp in g.tensors if sp.quant}
        assert m8 == m4 and m4
        assert all(sp.qfmt == "mxfp4" for g in g4.values() for sp in g.tensors if sp.quant)
        assert all(sp.qfmt == "fp8" for g in g8.values() for sp in g.tensors if sp.quant)
    _, g4, _ = registry.build("tiny-gpt2", seq=16, weight_dtype="mxfp4", act_dtype="fp8")
    by_name = {sp.name: sp for g in g4.values() for sp in g.tensors}
    assert not by_name["wte"].quant  # GPT-2's tied embedding stays bf16, as do norms and biases
    assert not any(sp.quant for sp in by_name.values() if len(sp.shape) == 1)


def test_plan_bytes_of_mini_llama_by_hand():
    """mini-llama: 2 layers, hidden 256, 4 heads / 2 kv heads of 64, ffn 512, vocab 1024. Marked
    per layer: qkv [512, 256], o [256, 256], gate_up [1024, 256], down [256, 512]; and the LM head
    [1024, 256]. Every marked tensor is its own 256-B multiple in both parts here."""
    p = runtime.plan("mini-llama", world=1, seq=64, batch=2, weight_dtype="mxfp4", act_dtype="fp8")
    pb = runtime.plan("mini-llama", world=1, seq=64, batch=2)
    marked = 2 * (512 * 256 + 256 * 256 + 1024 * 256 + 256 * 512) + 1024 * 256
    total_b, total_4 = sum(pb.param_bytes.values()), sum(p.param_bytes.values())
    assert total_b - total_4 == 2 * marked - (marked // 2 + marked // 32)
    assert total_4 == 1292800


def test_save_resume_and_cli(tmp_path, capsys):
    p = runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="mxfp4", act_dtype="fp8")
    assert p.args["weight_dtype"] == "mxfp4" and p.args["act_dtype"] == "fp8"
    path = str(tmp_path / "mx.json")
    runtime.save_plan(p, path)
    assert json.load(open(path))["args"]["weight_dtype"] == "mxfp4"
    q = runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="mxfp4", act_dtype="fp8", resume=path)
    assert q.order == p.order and q.param_bytes == p.param_bytes
    with pytest.raises(ValueError):  # saved mxfp4, resumed fp8
        runtime.plan("tiny-llama", world=1, seq=16, weight_dtype="fp8", act_dtype="fp8", resume=path)
    assert cli.main(["plan", "--model", "tiny-gpt2", "--seq", "16", "--weight-dtype", "mxfp4", "--act-dtype", "fp8"]) == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert out["weight_dtype"] == "mxfp4" and out["act_dtype"] == "fp8" and out["tasks_completed"] == out["tasks_total"]
    assert cli.main(["run", "--device", "cpu", "--model", "tiny-gpt2", "--seq", "16", "--steps", "1", "--warmup", "0",
                     "--weight-dtype", "mxfp4", "--act-dtype", "fp8"]) == 0
    res = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["weight_dtype"] == "mxfp4" and res["valid"]


def test_executor_refuses_mxfp4_weights_without_fp8_activations():
    p = runtime.plan("tiny-gpt2", world=1, seq=16, weight_dtype="mxfp4", act_dtype="fp8")
    with pytest.raises(ValueError, match="W4A8"):
        DAGExecutor(p.tasks, p.programs[0], runtime.make_store(p), "cpu", model_cfg=p.cfg)


# ------------------------------------------------------------------------- ops.linear_w4a8
def test_linear_w4a8_cpu_follows_the_definition():
    g = torch.Generator().manual_seed(1)
    M, N, K = 37, 64, 160
    xq, xs = ops.quantize_rows_fp8(torch.randn(M, K, generator=g).to(BF))
    q, s = ops.quantize_mxfp4(_weights(N, K, seed=2))
    bias = (0.1 * torch.randn(N, generator=g)).to(BF)
    res = torch.randn(M, N, generator=g).to(BF)
    prod = (xq.float() * xs[:, None]) @ ops.dequantize_mxfp4(q, s, torch.float32).t()
    assert torch.equal(ops.linear_w4a8(xq, xs, q, s), prod.to(BF))
    for act, fn in [("gelu", lambda v: F.gelu(v, approximate="tanh")), ("silu", F.silu), ("relu", torch.relu)]:
        want = fn(0.5 * prod + bias.float()) + res.float()
        got = ops.linear_w4a8(xq, xs, q, s, bias, act=act, residual=res, alpha=0.5)
        assert got.dtype == BF and torch.allclose(got.float(), want, atol=2e-2, rtol=1e-2), act
    y = prod + bias.float()
    want = F.silu(y[:, :N // 2]) * y[:, N // 2:]
    got = ops.linear_w4a8(xq, xs, ops.interleave_gate_up(q), ops.interleave_gate_up(s), ops.interleave_gate_up(bias),
                          act="swiglu")
    assert got.shape == (M, N // 2) and torch.allclose(got.float(), want, atol=1e-2, rtol=1e-2)
    out = torch.zeros(M, N + 8, dtype=BF)
    ops.linear_w4a8(xq, xs, q, s, out=out[:, 4:4 + N])
    assert torch.equal(out[:, 4:4 + N], prod.to(BF)) and (out[:, :4] == 0).all()
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.linear_w4a8(xq[:, :48].contiguous(), xs, q[:, :24].contiguous(), s)
    with pytest.raises(TypeError):
        ops.linear_w4a8(xq.float().to(BF), xs, q, s)
    with pytest.raises(TypeError):
        ops.linear_w4a8(xq, xs, q.view(torch.float8_e4m3fn), s)


# --------------------------------------------------------------------------------- executor
# Measured here (this executor against reference.forward(act_dtype="fp8") on the same mxfp4
# store, seq=64, batch=2), as (max-abs error / max |logit|, rms-relative error): mini-gpt2 0.0599
# and 0.0507, mini-llama 0.0614 and 0.0592. Both backends are held to 2 x these (the margin of
# the W8A8 tests: an upstream bf16 step can flip an e4m3 rounding): plumbing, not arithmetic.
EXEC_CPU = {"mini-gpt2": (0.0599, 0.0507), "mini-llama": (0.0614, 0.0592)}


def _measures(out, ref):
    d = out - ref
    return d.abs().max().item() / ref.abs().max().item(), (d.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


@pytest.mark.parametrize("model", ["mini-gpt2", "mini-llama"])
def test_cpu_executor_mxfp4(model, capsys):
    p = runtime.plan(model, world=1, seq=64, batch=2, weight_dtype="mxfp4", act_dtype="fp8")
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store)
    ex.step()
    out = ex.output("output_projection").float()
    tok = synthetic_tokens("@tokens", 128, p.cfg.vocab_size).view(2, 64)
    ref = reference.forward(p.cfg, store, tok, act_dtype="fp8")
    maxrel, rmsrel = _measures(out, ref)
    # the reference's mode covers the new format: without the input quantise-dequantise it lands elsewhere
    ref16 = reference.forward(p.cfg, store, tok)
    assert not torch.equal(ref, ref16) and _measures(out, ref16)[1] > 0
    # reported, not gated: what MXFP4 storage costs on random-init weights
    lines = []
    for other in ("bf16", "fp8"):
        po = runtime.plan(model, world=1, seq=64, batch=2, weight_dtype=other)
        ro = reference.forward(po.cfg, runtime.make_store(po), tok)
        d = ref16 - ro
        top1 = (ref16.argmax(-1) == ro.argmax(-1)).float().mean().item()
        lines.append(f"mxfp4 store vs {other} store: max logit diff {d.abs().max().item():.4f}, rms-relative "
                     f"{_measures(ref16, ro)[1]:.4f}, top-1 agreement {top1:.3f}")
    with capsys.disabled():
        print(f"\n{model}: executor vs reference: max {maxrel:.4f} rms {rmsrel:.4f}; " + "; ".join(lines))
    cmax, crms = EXEC_CPU[model]
    assert maxrel <= 2 * cmax and rmsrel <= 2 * crms


def test_cpu_executor_mxfp4_under_cap():
    need = sum(runtime.plan("mini-llama", world=1, seq=64, batch=2, weight_dtype="mxfp4",
                            act_dtype="fp8").param_bytes.values()) / 1e9
    p = runtime.plan("mini-llama", world=1, seq=64, batch=2, weight_dtype="mxfp4", act_dtype="fp8", cap_gb=0.6 * need)
    assert p.completed == p.total
    store = runtime.make_store(p)
    ex = runtime.make_executor(p, 0, "cpu", store, debug=True)
    for _ in range(3):
        st = ex.step()
    assert st.param_fills > 0
    tok = synthetic_tokens("@tokens", 128, p.cfg.vocab_size).view(2, 64)
    maxrel, rmsrel = _measures(ex.output("output_projection").float(),
                               reference.forward(p.cfg, store, tok, act_dtype="fp8"))
    cmax, crms = EXEC_CPU["mini-llama"]
    assert maxrel <= 2 * cmax and rmsrel <= 2 * crms
