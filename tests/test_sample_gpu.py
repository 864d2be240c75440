"""The sampling kernel (csrc/kernels/sample.hip) on every case of sample_cases.py against the
independent float64 oracle: exact greedy tokens and top-k thresholds, the top-p and draw windows
of ``sample_cases.EPS``, poisoned pad columns and rows, ties across the workgroup slices, the
stream rule and bit-identical repeats. Prints the measured error that EPS is made from.
test_sample_cpu.py shows that the acceptance rejects mutants.
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sample_cases as S  # noqa: E402
from distributed_llm_scheduler_amd import ops  # noqa: E402
from distributed_llm_scheduler_amd.models import registry  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_measured = {}


@pytest.mark.parametrize("B, V", [(1, 1), (1, 8192), (1, 8193), (3, 50257), (1, 128256), (32, 128256), (96, 128256),
                                  (600, 128256), (1, 1 << 20)])
def test_slices_are_the_cases_slices(B, V):
    n, length = ops.sample_slices(B, V)
    assert (n, length) == S.slices(B, V) and length % 8 == 0 and (n - 1) * length < V <= n * length
    assert registry.sample_slices(B, V) == (n, length)  # what the plan sizes the sampler's workspace by


def _kernel(name):
    if name in _measured:
        return
    c = S.case(name)
    ws = ops.sample_workspace(c.B, c.V, DEV)
    nxt, stats, stream = S.run(ops, c, DEV, ws)
    # measured under the widest window a sampler may have here (2^-14), then held to EPS
    err = S.check(c, nxt, stats, stream, eps=2.0 ** -14)
    print(f"\n[sample] {name}: max(|Z - Z_ref|, |c - c_ref|) / Z_ref = {err:.3e}")
    S.check(c, nxt, stats, stream)
    assert int(ws[1].abs().sum()) == 0, "a ticket was not reset"
    _measured[name] = err


@pytest.mark.parametrize("name", S.CASES)
def test_kernel(name):
    _kernel(name)


def test_measured_error_is_what_eps_was_made_from():
    for name in S.CASES:  # (already measured when the whole file runs)
        _kernel(name)
    worst = max(_measured.values())
    print(f"\n[sample] measured error over {len(_measured)} cases: {worst:.3e} "
          f"(sample_cases.MEASURED_ERR {S.MEASURED_ERR:.3e}, EPS 2^{torch.tensor(S.EPS).log2().item():.0f})")
    assert 3 * worst <= S.EPS <= 2.0 ** -14


def test_stream_rule():
    S.check_stream_rule(ops, DEV)


@pytest.mark.parametrize("name", S.DETERMINISM_CASES)
def test_same_launch_twice_is_bit_identical(name):
    c = S.case(name)
    ws = ops.sample_workspace(c.B, c.V, DEV)
    first = S.run(ops, c, DEV, ws)
    for _ in range(3):
        again = S.run(ops, c, DEV, ws)
        assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(first, again))


def test_two_cases_on_one_workspace():
    """The second launch has other logits and greedy rows only: stale partials are not merged."""
    a, b = S.case("ties_v128256_k1"), S.case("ties_v128256_greedy")
    ws = ops.sample_workspace(a.B, a.V, DEV)
    for c in (a, b, a):
        S.check(c, *S.run(ops, c, DEV, ws))
    assert int(ws[1].abs().sum()) == 0


def test_parameters_are_read_from_the_device_every_launch():
    """Device-resident seed and eos: a launch follows what the tensors hold (what a captured
    graph relies on)."""
    c = S.case("draws_v50257_k50")
    B = c.B
    seed = torch.tensor([c.seed], dtype=torch.int64, device=DEV)
    args = (c.logits.to(DEV), c.V, c.T, torch.tensor(c.pos, dtype=torch.int32, device=DEV))
    par = (torch.tensor(c.tau, device=DEV), torch.tensor(c.k, dtype=torch.int32, device=DEV),
           torch.tensor(c.p, device=DEV))
    ws = ops.sample_workspace(B, c.V, DEV)

    def go():
        stream = torch.full((B, S.CAP), S.SENTINEL, dtype=torch.int32, device=DEV)
        nxt, stats = ops.sample_tokens(*args, stream, S.CAP, *par, seed, request=c.request, workspace=ws)
        return nxt.cpu(), stats.cpu(), stream.cpu()

    first = go()
    S.check(c, *first)
    seed += 1
    second = go()
    assert not torch.equal(first[0], second[0])
    c2 = S.dataclasses.replace(c, seed=c.seed + 1)
    S.check(c2, *second)


def test_refusals():
    c = S.case("distinct_v333_b3_t4")
    dev = torch.device(DEV)
    a = dict(logits=c.logits.to(dev), V=c.V, T=c.T, pos=torch.zeros(3, dtype=torch.int32, device=dev),
             tokens=torch.zeros(3, 8, dtype=torch.int32, device=dev), C=8, temperature=torch.zeros(3, device=dev),
             top_k=torch.zeros(3, dtype=torch.int32, device=dev), top_p=torch.ones(3, device=dev), seed=0)
    with pytest.raises(ValueError, match="workspace"):
        ops.sample_tokens(**a)
    ws = ops.sample_workspace(3, c.V, dev)
    with pytest.raises(ValueError, match="top_k"):
        ops.sample_tokens(**{**a, "top_k": torch.zeros(3, dtype=torch.int32)}, workspace=ws)
    big = S.case("distinct_v50257_b3_t4")
    with pytest.raises(RuntimeError, match="partials"):
        ops.sample_tokens(**{**a, "logits": big.logits.to(dev), "V": big.V}, workspace=ws)
