"""Token sampling without a GPU: the Philox vectors, the CPU path of ``ops.sample_tokens`` on every
case of sample_cases.py against the independent float64 oracle, the stream rule, the argument
refusals, and mutants that the acceptance must reject.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sample_cases as S  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402


@pytest.mark.parametrize("fn", [S.philox, ops.philox4x32_10], ids=["oracle", "ops"])
def test_philox_vectors(fn):
    for counter, key, want in S.PHILOX_VECTORS:
        assert tuple(fn(counter, key)) == want, [hex(x) for x in fn(counter, key)]


def test_uniform_is_24_bits_of_word_0():
    seed = 0xA4093822_299F31D0
    u = S.uniform(seed, 2, 1, 5)
    assert u == (S.philox((5, 1, 2, 0), (0x299F31D0, 0xA4093822))[0] >> 8) * 2.0 ** -24
    assert u == ops.sample_uniform(seed, 2, 1, 5) and 0.0 <= u < 1.0
    assert S.uniform(-1, 0, 0, 0) == S.uniform((1 << 64) - 1, 0, 0, 0)  # a negative int64 seed is its bit pattern


@pytest.mark.parametrize("name", S.CASES)
def test_cpu_path(name):
    c = S.case(name)
    nxt, stats, stream = S.run(ops, c, "cpu")
    S.check(c, nxt, stats, stream)


def test_stream_rule():
    S.check_stream_rule(ops, "cpu")


def test_same_launch_twice_is_identical():
    c = S.case("draws_v333_k50")
    a, b = S.run(ops, c, "cpu"), S.run(ops, c, "cpu")
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_draw_depends_on_seed_request_sequence_and_position_only():
    us = {S.uniform(1, 0, 0, 4), S.uniform(2, 0, 0, 4), S.uniform(1, 1, 0, 4), S.uniform(1, 0, 1, 4),
          S.uniform(1, 0, 0, 5)}
    assert len(us) == 5


def test_acceptance_rejects_mutants():
    """A sampler that walks the candidates in logit order, one whose top-k threshold is a class
    off, and a greedy that takes the last maximum all fail the acceptance."""
    c = S.case("draws_v333_k50")
    l = c.rows[0]
    nxt, stats, _ = S.run(ops, c, "cpu")
    order = l.sort(descending=True, stable=True).indices
    rejected = 0
    for b in range(c.B):
        theta = float(stats[b, 0])
        kept = order[l[order] >= theta]
        w = torch.exp(l[kept] - l.max())
        u = S.uniform(c.seed, c.request, b, c.n(b))
        tok = int(kept[int((w.cumsum(0) > u * w.sum()).nonzero()[0])])
        try:
            S.accept(l, 1.0, 50, 0.9, u, tok, stats[b], S.EPS)
        except AssertionError:
            rejected += 1
    assert rejected >= c.B * 3 // 4, rejected
    c = S.case("tie_at_theta_k_v50257")
    nxt, stats, _ = S.run(ops, c, "cpu")
    off = stats[0].clone()
    vals = c.rows[0].unique()
    off[0] = vals[int((vals == float(off[0])).nonzero()[0]) + 1]  # the next class up
    with pytest.raises(AssertionError, match="theta"):
        S.accept(c.rows[0], 1.0, 50, 1.0, S.uniform(c.seed, 0, 0, c.n(0)), int(nxt[0]), off, S.EPS)
    c = S.case("ties_v50257_greedy")
    with pytest.raises(AssertionError, match="greedy"):
        S.accept(c.rows[0], 0.0, 0, 1.0, 0.5, c.V - 1, torch.tensor([float(c.rows[0].max()), 1.0, 0.0, 1.0]), S.EPS)


def _args(B=2, V=40, T=1, C=8):
    return dict(logits=torch.zeros(B * T, 64, dtype=torch.bfloat16), V=V, T=T,
                pos=torch.zeros(B, dtype=torch.int32), tokens=torch.zeros(B, C, dtype=torch.int32), C=C,
                temperature=torch.zeros(B), top_k=torch.zeros(B, dtype=torch.int32), top_p=torch.ones(B), seed=0)


@pytest.mark.parametrize("change, match", [
    (dict(V=0), "V"),
    (dict(V=(1 << 20) + 1), "V"),
    (dict(logits=torch.zeros(2, 64)), "bf16"),
    (dict(logits=torch.zeros(3, 64, dtype=torch.bfloat16)), r"\[B\*T\]"),
    (dict(V=65), ">= V"),
    (dict(logits=torch.zeros(2, 60, dtype=torch.bfloat16)), "stride"),
    (dict(pos=torch.zeros(2, dtype=torch.int64)), "pos"),
    (dict(tokens=torch.zeros(2, 7, dtype=torch.int32)), "tokens"),
    (dict(temperature=torch.zeros(2, dtype=torch.float64)), "temperature"),
    (dict(top_k=torch.zeros(3, dtype=torch.int32)), "top_k"),
    (dict(top_p=torch.ones(1)), "top_p"),
    (dict(seed=1.5), "seed"),
    (dict(seed=torch.zeros(1, dtype=torch.int32)), "seed"),
    (dict(eos=torch.zeros(1, dtype=torch.int64)), "eos"),
    (dict(prompt_len=torch.zeros(2)), "prompt_len"),
    (dict(done=torch.zeros(1, dtype=torch.int32)), "done"),
    (dict(request=-1), "request"),
    (dict(stats=torch.zeros(2, 3)), "stats"),
])
def test_refusals(change, match):
    with pytest.raises(ValueError, match=match):
        ops.sample_tokens(**{**_args(), **change})


def test_defaults_allocate_outputs():
    a = _args()
    a["logits"][:, 3] = 1.0
    nxt, stats = ops.sample_tokens(**a)
    assert nxt.tolist() == [3, 3] and stats.shape == (2, 4) and a["tokens"][:, 1].tolist() == [3, 3]
    assert ops.sample_workspace(2, 40, "cpu") is None
