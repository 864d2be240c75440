"""What the CPU and GPU tests of decode steps with an fp8 KV cache (test_decode_fp8_cpu.py,
test_decode_fp8_gpu.py) share: the end-to-end bound and the check of a step's logits against it.

decode_checks.MARGIN (0.03 x max|ref| against the fp32 reference) does not carry over: e4m3 K/V
quantisation alone moves the logits of these random-init models by about that much. The bound is
computed from the reference, never from the code under test:

    Q = max|forward(kv_dtype="fp8") - forward()| over the test's own token streams,
    a step's logits are within MARGIN x max|ref| + 2 x Q of the UNQUANTISED reference forward().

The first term is the project's allowance for bf16 arithmetic. The executor quantises bf16-rounded
rows where the reference quantises fp32 rows: another realisation of the same rounding noise, which
a CPU probe put 0.8 Q from the reference's; the factor 2 covers that. The sharp checks are the
kernel-level ones (test_attn_decode_fp8_gpu.py); this one catches plumbing errors — the wrong scale
tensor, the wrong layer's cache, scales not advanced with pos.
"""
import torch

from decode_checks import MARGIN, full_reference
from distributed_llm_scheduler_amd.models import reference

observed = {}  # what -> (worst error / bound, Q / max|ref|): printed by the tests, quoted in the README


def quant_shift(p, store, tokens, n):
    """Q over the first n tokens of every sequence, and the unquantised reference [B][n][V]."""
    ref = full_reference(p, store, tokens, n)
    tok = tokens[:, :n].contiguous().cpu()
    q8 = torch.stack([reference.forward(p.cfg, store, tok[b].view(1, -1), kv_dtype="fp8")[0]
                      for b in range(tok.shape[0])])
    return (q8 - ref).abs().max().item(), ref


def check_steps_fp8(p, ex, store, tokens, T, steps, start=0, tid="output_projection", sync=None, step=None,
                    what=None):
    """``steps`` steps from length ``start``: after each, the T logits rows of every sequence are
    within MARGIN x max|ref| + 2 Q of the unquantised reference rows, and kv_lengths() advanced."""
    Q, ref = quant_shift(p, store, tokens, start + steps * T)
    worst = 0.0
    for n in range(steps):
        (step or ex.step)()
        if sync is not None:
            sync()
        lo = start + n * T
        logits = ex.output(tid).float().cpu()
        assert logits.shape[:2] == (tokens.shape[0], T)
        want = ref[:, lo:lo + T]
        err, scale = (logits - want).abs().max().item(), want.abs().max().item()
        bound = MARGIN * scale + 2 * Q
        worst = max(worst, err / bound)
        assert err < bound, (f"step {n} (positions {lo} .. {lo + T - 1}): {err:.4g} >= {MARGIN} x {scale:.4g} + "
                             f"2 x {Q:.4g}")
        lens = ex.kv_lengths()
        assert lens == [lo + T] * tokens.shape[0], lens
    what = what or f"{p.cfg.name} T={T}"
    frac = Q / ref.abs().max().item()
    print(f"fp8 KV cache, {what}: Q = {Q:.4g} ({frac:.4f} of max|ref|), worst step error {worst:.3f} of the bound")
    observed[what] = (worst, frac)
    return worst
