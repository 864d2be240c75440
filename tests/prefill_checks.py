"""What the CPU and GPU tests of chunked prompt prefill (test_prefill_cpu.py, test_prefill_gpu.py)
share: NaN-filled caches to start from, token steps checked at RAGGED positions against the fp32
reference forward over each sequence's own stream, and the trajectory of a generating plan after a
chunked prefill with generate_checks' acceptance test at every draw.
"""
import math

import torch

import decode_checks as DC
import decode_fp8_checks as D8
import generate_checks as G
import sample_cases as S
from distributed_llm_scheduler_amd.models import reference

MARGIN = DC.MARGIN


def poison_caches(ex):
    """Every cache row NaN (fp8: the e4m3 NaN byte and NaN scales): a prefill that reads a row it
    did not write, or leaves one unwritten below a sequence's length, shows in the logits."""
    for cs in ex._kv_cache.values():
        if len(cs) == 2:
            cs[0].fill_(math.nan)
            cs[1].fill_(math.nan)
        else:
            cs[0].fill_(0x7F)
            cs[1].fill_(0x7F)
            cs[2].fill_(math.nan)
            cs[3].fill_(math.nan)


def lengths(ex, prefix=""):
    lens = ex.kv_lengths()
    return lens[prefix] if isinstance(lens, dict) else lens


def check_token_steps(p, ex, store, tokens, steps, kv_dtype="bf16", tid="output_projection", prefix="", sync=None,
                      step=None, what=""):
    """``steps`` token steps from the present (ragged) lengths: after each, sequence b's logits row is
    within the bound of the reference row at ITS position, finite, and its length advanced by one.
    bf16 caches: decode_checks.MARGIN x max|ref|; fp8: decode_fp8_checks' MARGIN x max|ref| + 2 Q."""
    start = lengths(ex, prefix)
    n = max(start) + steps
    if kv_dtype == "fp8":
        Q, ref = D8.quant_shift(p, store, tokens, n)
    else:
        Q, ref = 0.0, DC.full_reference(p, store, tokens, n)
    worst = 0.0
    for s in range(steps):
        (step or ex.step)()
        if sync is not None:
            sync()
        logits = ex.output(tid).float().cpu()[:, 0]
        assert torch.isfinite(logits).all(), f"{what} step {s}: logits are not finite"
        for b, n0 in enumerate(start):
            want = ref[b, n0 + s]
            err, scale = (logits[b] - want).abs().max().item(), ref[b].abs().max().item()
            bound = MARGIN * scale + 2 * Q
            worst = max(worst, err / bound)
            assert err < bound, f"{what} step {s} sequence {b} (position {n0 + s}): {err:.4g} >= {bound:.4g}"
        assert lengths(ex, prefix) == [n0 + s + 1 for n0 in start]
    print(f"prefill {p.cfg.name} kv {kv_dtype} {what}: worst token-step error {worst:.3f} of the bound")
    return worst


def run_generate(ex, sampling, prompts=G.PROMPTS, new=G.NEW, name="@tokens", tid="output_projection", prefix="",
                 step=None, sync=None):
    """set_sampling, set_prompts, prefill() in chunk steps, then ``new`` token steps keeping each
    step's logits [B][V] and sampler statistics [B][4]. Returns (chunk steps, logits, stats, stream)."""
    ex.set_sampling(**sampling)
    ex.set_prompts(name, prompts)
    chunks = ex.prefill()
    assert lengths(ex, prefix) == [len(pr) - 1 for pr in prompts]
    logits, stats = [], []
    for s in range(new):
        (step or ex.step)()
        if sync is not None:
            sync()
        logits.append(ex.output(tid).float().cpu()[:, 0].clone())
        stats.append(G.state(ex, prefix)["stats"].cpu().clone())
    return chunks, logits, stats, G.state(ex, prefix)["tokens"].cpu().clone()


def check_generate(p, store, sampling, logits, stats, stream, prompts=G.PROMPTS, request=0, kv_dtype="bf16"):
    """generate_checks.check for ragged positions: token step s finds sequence b at position
    len(prompt_b) - 1 + s; its logits are held to the reference over the FINAL stream and the token
    it wrote to sample_cases.accept at the draw of (seed, request, b, that position + 1)."""
    new = len(logits)
    for b, pr in enumerate(prompts):
        assert stream[b, :len(pr)].tolist() == list(pr), f"prompt {b} changed: {stream[b, :len(pr)].tolist()}"
    kw = {} if kv_dtype == "bf16" else {"kv_dtype": kv_dtype}
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
    tau, k, pp, seed = (sampling[x] for x in ("temperature", "top_k", "top_p", "seed"))
    worst = 0.0
    for b, pr in enumerate(prompts):
        n = len(pr) - 1 + new
        ref = reference.forward(p.cfg, store, stream[b, :n].view(1, -1), **kw)[0]  # [n][V]
        scale = ref.abs().max().item()
        for s in range(new):
            pos = len(pr) - 1 + s
            err = (logits[s][b] - ref[pos]).abs().max().item()
            worst = max(worst, err / (MARGIN * scale))
            assert err < MARGIN * scale, f"sequence {b} step {s}: logits {err:.4g} >= {MARGIN} x {scale:.4g}"
            l = logits[s][b].double()
            tok = int(stream[b, pos + 1])
            what = f"{p.cfg.name} sequence {b} token step {s} (position {pos})"
            if not tau > 0:
                assert tok == S.first_argmax(l), f"{what}: token {tok}, lowest argmax {S.first_argmax(l)}"
            S.accept(l, f32(tau), k, f32(pp), S.uniform(seed, request, b, pos + 1), tok, stats[s][b], S.EPS, what)
    print(f"generate after prefill {p.cfg.name} kv {kv_dtype}: worst logits error {worst:.3f} of the bound")
