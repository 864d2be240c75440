"""What the CPU and GPU tests of MoE decode steps (test_moe_decode_cpu.py, test_moe_decode_gpu.py)
share: the all-k variant of a Mixtral preset, where routing cannot flip and decode_checks.check_steps
holds every row, and the near-tie measure of test_executor_gpu._check for top-2 routing, applied
per step and accumulated over every checked row:

* a row is CLEAR when every layer's reference router margin (k-th against (k+1)-th logit) is at
  least 0.05; a bf16 router may pick another expert only on the other rows;
* no clear row may exceed decode_checks.MARGIN x max|ref|;
* rows that exceed it stay below 10 % of the checked rows;
* clear rows are at least half of the checked rows (or the test checks too little).

With ``decode_checks.stream(vocab, seed=1)`` the fp32 reference of mini-mixtral has 84 clear rows
of 128 over all 64 positions and 29 of 48 over the first 24.
"""
import torch

from decode_checks import MARGIN
from distributed_llm_scheduler_amd.models import config, reference

RISK = 0.05
BAD_SHARE = 0.1
_top2 = {}


def allk_name(model):
    return model + "-allk"


def register_allk(model, setitem):
    """``setitem(mapping, key, value)``: monkeypatch.setitem in a test, dict.__setitem__ in a child process."""
    c = config.PRESETS[model]
    setitem(config.PRESETS, allk_name(model), c.with_(name=allk_name(model), top_k=c.n_experts))
    return allk_name(model)


_allk = {}


def check_steps_allk(p, ex, store, tokens, T, steps, step=None, sync=None, kv_dtype="bf16", tid="output_projection"):
    """decode_checks.check_steps against ``reference.forward`` with the plan's ``kv_dtype``: every
    logits row of every step within MARGIN x max|ref|. Returns the worst error / bound."""
    tok = tokens[:, :steps * T].contiguous().cpu()
    key = (p.cfg.name, kv_dtype, tuple(tok.flatten().tolist()), tuple(tok.shape), id(store))
    if key not in _allk:
        kw = {} if kv_dtype == "bf16" else {"kv_dtype": kv_dtype}
        _allk[key] = (store, torch.stack([reference.forward(p.cfg, store, tok[b].view(1, -1), **kw)[0]
                                          for b in range(tok.shape[0])]))
    ref = _allk[key][1]
    worst = 0.0
    for n in range(steps):
        (step or ex.step)()
        if sync is not None:
            sync()
        lo = n * T
        logits = ex.output(tid).float().cpu()
        assert logits.shape[:2] == (tokens.shape[0], T)
        want = ref[:, lo:lo + T]
        err, scale = (logits - want).abs().max().item(), want.abs().max().item()
        worst = max(worst, err / (MARGIN * scale))
        assert err < MARGIN * scale, f"step {n} (positions {lo} .. {lo + T - 1}): {err:.4g} >= {MARGIN} x {scale:.4g}"
        assert ex.kv_lengths() == [lo + T] * tokens.shape[0]
    print(f"moe decode {p.cfg.name} kv {kv_dtype} T={T}: worst row error {worst:.3f} of the bound")
    return worst


def top2_reference(p, store, tokens, n, kv_dtype="bf16"):
    """([B][n][V] reference logits, [B][n] bool: clear rows), once per (model, store, tokens)."""
    tok = tokens[:, :n].contiguous().cpu()
    key = (p.cfg.name, kv_dtype, tuple(tok.flatten().tolist()), tuple(tok.shape), id(store))
    if key not in _top2:
        refs, clear = [], []
        kw = {} if kv_dtype == "bf16" else {"kv_dtype": kv_dtype}
        for b in range(tok.shape[0]):
            margins = []
            refs.append(reference.forward(p.cfg, store, tok[b].view(1, -1), router_margins=margins, **kw)[0])
            assert margins, "not an MoE model"
            clear.append(~torch.stack([m.abs() < RISK for m in margins]).any(0).view(-1))
        _top2[key] = (store, torch.stack(refs), torch.stack(clear))
    return _top2[key][1], _top2[key][2]


def check_steps_top2(p, ex, store, tokens, T, steps, step=None, sync=None, kv_dtype="bf16", tid="output_projection"):
    """``steps`` steps from empty caches under the near-tie measure; returns (checked, clear, bad) rows."""
    ref, clear = top2_reference(p, store, tokens, steps * T, kv_dtype)
    checked = n_clear = n_bad = 0
    for n in range(steps):
        (step or ex.step)()
        if sync is not None:
            sync()
        lo = n * T
        logits = ex.output(tid).float().cpu()
        assert logits.shape[:2] == (tokens.shape[0], T)
        want = ref[:, lo:lo + T]
        row_err, scale = (logits - want).abs().amax(-1), want.abs().max().item()
        bad = row_err > MARGIN * scale
        c = clear[:, lo:lo + T]
        assert not (bad & c).any(), (f"step {n}: {int((bad & c).sum())} clear rows off by up to "
                                     f"{row_err[c].max().item():.4g} > {MARGIN} x {scale:.4g}")
        checked += bad.numel()
        n_clear += int(c.sum())
        n_bad += int(bad.sum())
        assert ex.kv_lengths() == [lo + T] * tokens.shape[0]
    print(f"moe decode {p.cfg.name} T={T}: {checked} rows, {n_clear} clear, {n_bad} past the margin")
    assert n_bad < BAD_SHARE * checked, (n_bad, checked)
    assert 2 * n_clear >= checked, (n_clear, checked)
    return checked, n_clear, n_bad
