"""Dispatch of the wave-private rings on 64-row tiles (config ids tuning.PRIVATE_WIDE ..):
``ops.linear_norm`` hands the native GEMM a family id if and only if the tuning table names one for
the shape AND the family takes the launch — a folded norm with handed-over row statistics, no
activation or GeLU, no RoPE or residual, a K whose 64-deep tiles divide by the config's waves.
Every other launch of such a shape, ``ops.linear`` included, gets the 64 x 64 K-grouped config the
table held before. The native library is replaced by a recorder, so this runs without a GPU.
"""
import json
import os
import re

import pytest
import torch

from distributed_llm_scheduler_amd import ops
from distributed_llm_scheduler_amd.ops import tuning

FLAGSHIP = [(512, 2304, 768), (512, 3072, 768)]
BF = torch.bfloat16


class _Recorder:
    """Stands in for the op library: records (config, splitk) of every gemm call."""

    def __init__(self):
        self.calls = []

    def gemm(self, x, w, bias, residual, act, alpha, out, config, splitk, *rest, **kw):
        self.calls.append((int(config), int(splitk)))
        return torch.empty(x.numel() // x.shape[-1], w.shape[0] // (2 if act == ops.SWIGLU else 1), dtype=x.dtype)


@pytest.fixture
def recorder(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(ops, "_gpu", lambda t: True)
    monkeypatch.setattr(ops, "ext", lambda: rec)
    monkeypatch.setattr(tuning, "_model", None)
    return rec


def _use_table(monkeypatch, tmp_path, gemm):
    path = tmp_path / "t.json"
    path.write_text(json.dumps({"gemm": gemm, "candidates": {}, "refined": {}}))
    monkeypatch.setattr(tuning, "_PATH", str(path))
    monkeypatch.setattr(tuning, "_table", None)
    monkeypatch.setattr(tuning, "_overrides", {})
    monkeypatch.setattr(tuning, "_cands", {})
    monkeypatch.setattr(tuning, "_refined", {})
    monkeypatch.setattr(tuning, "_col_splits", {})


def _norm(rec, M, N, K, stats=True, **kw):
    rec.calls.clear()
    ops.linear_norm(torch.zeros(M, K, dtype=BF), torch.zeros(N, K, dtype=BF), torch.zeros(N), torch.zeros(N, dtype=BF),
                    kw.pop("mode", "layernorm"), ext_stats=torch.zeros(M, 2) if stats else None, **kw)
    assert len(rec.calls) == 1
    return rec.calls[0]


def _linear(rec, M, N, K, **kw):
    rec.calls.clear()
    ops.linear(torch.zeros(M, K, dtype=BF), torch.zeros(N, K, dtype=BF), **kw)
    assert len(rec.calls) == 1
    return rec.calls[0]


def test_shipped_table_choice_reaches_the_kernel(recorder):
    """The QKV and fc1 shapes launch exactly what the shipped table names with the step's operands;
    where that is a family id the family takes the shape, and a plain ``ops.linear`` of the shape
    or a launch without handed-over statistics gets the fallback."""
    for (M, N, K), act in zip(FLAGSHIP, (None, "gelu")):
        choice = tuple(tuning.table()[f"{M}x{N}x{K}"])
        assert _norm(recorder, M, N, K, act=act) == choice
        if choice[0] in tuning.PRIVATE_WIDE_CFGS:
            assert tuning.private_wide_takes(choice[0], K, folded=True, ext_stats=True, act=ops.ACT[act])
            assert _linear(recorder, M, N, K) == tuning.PRIVATE_WIDE_FALLBACK
            # (in-loop statistics need one K group: the fallback's own replacement, never a family id)
            assert _norm(recorder, M, N, K, stats=False)[0] not in tuning.PRIVATE_WIDE_CFGS
        else:
            assert _linear(recorder, M, N, K) == choice


def test_no_other_shipped_entry_names_the_family():
    named = {k for k, v in tuning.table().items() if v[0] in tuning.PRIVATE_WIDE_CFGS}
    assert named <= {f"{M}x{N}x{K}" for M, N, K in FLAGSHIP}
    for m, t in tuning._overrides.items():
        assert all(v[0] not in tuning.PRIVATE_WIDE_CFGS for v in t.values()), m
    assert not any(c in tuning.PRIVATE_WIDE_CFGS for v in tuning._col_splits.values() for _, _, c, _ in v)


@pytest.mark.parametrize("cfg", sorted(tuning.PRIVATE_WIDE_CFGS))
def test_family_id_if_and_only_if_table_and_rule_say_so(cfg, recorder, monkeypatch, tmp_path):
    BM, BN, W, S = tuning.PRIVATE_WIDE_CFGS[cfg]
    K_ok, K_bad = 64 * W * 3, 64 * W * 3 + 64
    _use_table(monkeypatch, tmp_path, {f"512x3072x{K_ok}": [cfg, 1], f"512x3072x{K_bad}": [cfg, 1],
                                       f"256x3072x{K_ok}": [17, 1]})
    fb = tuning.PRIVATE_WIDE_FALLBACK
    for mode in ("layernorm", "rmsnorm"):
        assert _norm(recorder, 512, 3072, K_ok, mode=mode) == (cfg, 1)
        assert _norm(recorder, 512, 3072, K_ok, mode=mode, act="gelu") == (cfg, 1)
    # the table names another config, or knows nothing of the shape: never a family id
    assert _norm(recorder, 256, 3072, K_ok) == (17, 1)
    assert _norm(recorder, 128, 3072, K_ok)[0] not in tuning.PRIVATE_WIDE_CFGS
    # launches the family refuses
    assert _norm(recorder, 512, 3072, K_bad) == fb  # K-tiles do not divide by W
    # in-loop statistics (they need one K group: linear_norm replaces the two-group fallback)
    assert _norm(recorder, 512, 3072, K_ok, stats=False)[0] not in tuning.PRIVATE_WIDE_CFGS
    for act in ("silu", "relu"):
        assert _norm(recorder, 512, 3072, K_ok, act=act) == fb
    assert _norm(recorder, 512, 3072, K_ok, act="swiglu")[0] not in tuning.PRIVATE_WIDE_CFGS  # (its own table key)
    rope = (torch.zeros(512, 8), torch.zeros(512, 8), 512, 16, 64)
    assert _norm(recorder, 512, 3072, K_ok, rope=rope) == fb
    assert _norm(recorder, 512, 3072, K_ok, residual=torch.zeros(512, 3072, dtype=BF)) == fb
    # ops.linear has no folded norm: always the fallback, whatever it attaches
    assert _linear(recorder, 512, 3072, K_ok) == fb
    assert _linear(recorder, 512, 3072, K_ok, act="gelu", bias=torch.zeros(3072, dtype=BF)) == fb
    rows = torch.tensor([0, 512], dtype=torch.int32)
    assert _linear(recorder, 512, 3072, K_ok, rows=rows, rows_hint=512)[0] not in tuning.PRIVATE_WIDE_CFGS


def test_private_wide_takes_matches_the_native_rule():
    """tuning.PRIVATE_WIDE_CFGS / private_wide_takes against the table of csrc/kernels/kernels.h, the
    instances gemm_private.hip launches and the refusals of gemm_glds_impl.h."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "csrc", "kernels", "kernels.h")).read()
    src = open(os.path.join(root, "csrc", "kernels", "gemm_private.hip")).read()
    impl = open(os.path.join(root, "csrc", "kernels", "gemm_glds_impl.h")).read()
    first, count = (int(v) for v in re.search(r"kGemmPrivateWide = (\d+), kGemmPrivateWideCount = (\d+);", hdr).groups())
    rows = re.search(r"kGemmPrivateWideCfgs\[kGemmPrivateWideCount\] = \{(.*)\};", hdr).group(1)
    cfgs = [tuple(int(v) for v in r.split(",")) for r in re.findall(r"\{([^{}]*)\}", rows)]
    assert first == tuning.PRIVATE_WIDE and count == len(cfgs)
    assert {first + i: c for i, c in enumerate(cfgs)} == tuning.PRIVATE_WIDE_CFGS
    launched = [tuple(int(v) for v in m) for m in re.findall(r"launch_private_wide<(\d+), (\d+), (\d+), (\d+)>", src)]
    assert launched == cfgs
    # ids apart from the register-staged kernel, the 32 x 48 family and the vendor library
    ids = set(tuning.PRIVATE_WIDE_CFGS)
    assert min(ids) >= tuning.REGSTAGE + 4 and max(ids) < tuning.LIB and not ids & set(tuning.PRIVATE_WAVES)
    rule = re.search(r"inline bool private_wide_takes\(.*?\n\}", impl, re.S).group(0)
    for term in ("a.K % (64 * waves) == 0", "splitk <= 1", "ln_mode == 1 || ln_mode == 2", "a.ext_stats", "!ranged",
                 "a.act == ACT_NONE || a.act == ACT_GELU_TANH", "a.rope.cols == 0", "!a.R", "!a.stats_out"):
        assert term in rule, term
    ok = dict(folded=True, ext_stats=True)
    for cfg, (BM, BN, w, S) in tuning.PRIVATE_WIDE_CFGS.items():
        assert 12 % w == 0 and w * S * (BM + BN) * 128 <= 160 * 1024  # K = 768 divides; the rings fit in LDS
        assert tuning.private_wide_takes(cfg, 64 * w, **ok) and tuning.private_wide_takes(cfg, 64 * w * 7, act=1, **ok)
        assert not tuning.private_wide_takes(cfg, 64 * w + 64, **ok) and not tuning.private_wide_takes(cfg, 0, **ok)
        assert not tuning.private_wide_takes(cfg, 64 * w * 2, sk=2, **ok)
        assert not tuning.private_wide_takes(cfg, 64 * w * 2) and not tuning.private_wide_takes(cfg, 64 * w, folded=True)
        for kw in ({"act": 2}, {"act": 3}, {"act": 4}, {"ranged": True}, {"rope": True}, {"residual": True},
                   {"stats_out": True}):
            assert not tuning.private_wide_takes(cfg, 64 * w * 2, **ok, **kw), kw
    assert not tuning.private_wide_takes(17, 768, **ok) and not tuning.private_wide_takes(122, 768, **ok)
    assert tuning.resolve_private_wide((17, 1), 768, **ok) == (17, 1)
