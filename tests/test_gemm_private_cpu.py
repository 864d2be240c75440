"""Dispatch of the wave-private-ring GEMM family (config ids tuning.PRIVATE ..): ``ops.linear``
hands the native GEMM a family id if and only if the tuning table names one for the shape, and
never for a launch the family refuses (an activation, RoPE, a row range, a K whose 64-deep tiles
do not divide by the config's waves) — that launch gets the K-grouped config of the same tile.
The native library is replaced by a recorder, so this runs without a GPU.
"""
import json

import pytest
import torch

from distributed_llm_scheduler_amd import ops
from distributed_llm_scheduler_amd.ops import tuning

FLAGSHIP = [(512, 768, 3072), (512, 768, 768)]


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


def _linear(rec, M, N, K, **kw):
    rec.calls.clear()
    ops.linear(torch.zeros(M, K, dtype=torch.bfloat16), torch.zeros(N, K, dtype=torch.bfloat16), **kw)
    assert len(rec.calls) == 1
    return rec.calls[0]


def test_shipped_table_choice_reaches_the_kernel(recorder):
    """The two GPT-2 N = 768 shapes launch exactly what the shipped table names; where that is a
    family id, the family takes the shape, and an epilogue it refuses gets the fallback."""
    for M, N, K in FLAGSHIP:
        choice = tuning.table()[f"{M}x{N}x{K}"]
        assert _linear(recorder, M, N, K) == tuple(choice)
        res = torch.zeros(M, N, dtype=torch.bfloat16)
        assert _linear(recorder, M, N, K, bias=torch.zeros(N, dtype=torch.bfloat16), residual=res) == tuple(choice)
        if choice[0] in tuning.PRIVATE_WAVES:
            assert tuning.private_takes(choice[0], K)
            assert _linear(recorder, M, N, K, act="gelu") == tuning.PRIVATE_FALLBACK
        else:
            assert _linear(recorder, M, N, K, act="gelu")[0] not in tuning.PRIVATE_WAVES


def test_no_other_shipped_entry_names_the_family():
    named = {k for k, v in tuning.table().items() if v[0] in tuning.PRIVATE_WAVES}
    assert named <= {f"{M}x{N}x{K}" for M, N, K in FLAGSHIP}
    for m, t in tuning._overrides.items():
        assert all(v[0] not in tuning.PRIVATE_WAVES for v in t.values()), m


@pytest.mark.parametrize("cfg", sorted(tuning.PRIVATE_WAVES))
def test_family_id_if_and_only_if_the_table_says_so(cfg, recorder, monkeypatch, tmp_path):
    W = tuning.PRIVATE_WAVES[cfg]
    K_ok, K_bad = 64 * W * 4, 64 * W * 4 + 64
    _use_table(monkeypatch, tmp_path, {f"512x768x{K_ok}": [cfg, 1], f"512x768x{K_bad}": [cfg, 1],
                                       f"256x768x{K_ok}": [45, 1]})
    assert _linear(recorder, 512, 768, K_ok) == (cfg, 1)
    assert _linear(recorder, 512, 768, K_ok, alpha=0.5, residual=torch.zeros(512, 768, dtype=torch.bfloat16)) == (cfg, 1)
    # the table names another config, or knows nothing of the shape: never a family id
    assert _linear(recorder, 256, 768, K_ok) == (45, 1)
    assert _linear(recorder, 128, 768, K_ok)[0] not in tuning.PRIVATE_WAVES
    # launches the family refuses
    assert _linear(recorder, 512, 768, K_bad) == tuning.PRIVATE_FALLBACK  # K-tiles do not divide by W
    for act in ("gelu", "silu", "relu"):
        assert _linear(recorder, 512, 768, K_ok, act=act) == tuning.PRIVATE_FALLBACK
    rope = (torch.zeros(512, 8), torch.zeros(512, 8), 512, 16, 64)
    assert _linear(recorder, 512, 768, K_ok, rope=rope) == tuning.PRIVATE_FALLBACK
    rows = torch.tensor([0, 512], dtype=torch.int32)
    assert _linear(recorder, 512, 768, K_ok, rows=rows, rows_hint=512)[0] not in tuning.PRIVATE_WAVES
    assert _linear(recorder, 512, 768, K_ok, act="swiglu")[0] not in tuning.PRIVATE_WAVES


def test_private_takes_matches_the_native_rule():
    """tuning.private_takes against the wave counts and the refusals of csrc/kernels/gemm_private.hip."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "csrc", "kernels", "gemm_private.hip")).read()
    hdr = open(os.path.join(root, "csrc", "kernels", "kernels.h")).read()
    waves = [int(v) for v in re.search(r"kWaves\[kGemmPrivateCount\] = \{([^}]*)\}", src).group(1).split(",")]
    first, count = (int(v) for v in re.search(r"kGemmPrivate = (\d+), kGemmPrivateCount = (\d+);", hdr).groups())
    assert first == tuning.PRIVATE and count == len(waves)
    assert {first + i: w for i, w in enumerate(waves)} == tuning.PRIVATE_WAVES
    assert tuning.PRIVATE >= tuning.REGSTAGE + 4 and max(tuning.PRIVATE_WAVES) < tuning.LIB
    for cfg, w in tuning.PRIVATE_WAVES.items():
        assert tuning.private_takes(cfg, 64 * w) and tuning.private_takes(cfg, 64 * w * 7)
        assert not tuning.private_takes(cfg, 64 * w + 64) and not tuning.private_takes(cfg, 0)
        assert not tuning.private_takes(cfg, 64 * w * 2, sk=2)
        for kw in ({"act": 1}, {"act": 4}, {"ranged": True}, {"rope": True}, {"folded": True}):
            assert not tuning.private_takes(cfg, 64 * w * 2, **kw), kw
    assert not tuning.private_takes(45, 3072)
