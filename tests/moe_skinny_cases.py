"""Cases and checks of ``ops.gemm_grouped_skinny``, shared by test_moe_skinny_cpu.py and
test_moe_skinny_gpu.py. A case is (act, (N, K), group counts); it runs with and without ``a_rows``
and with ``out`` and compact ``outs``. References are ``gemm_checks.ref64`` / ``ref64_swiglu``,
computed once per case on the CPU and never written again.

Bounded cases hold every element to ``gemm_checks.derived_bound`` with C = 2: the output is rounded
once and has no residual, the family ``C_BOUND["swiglu"]`` covers. Worst err / derived bound on an
MI355X over all cases of this file: see MEASURED below (the GPU test prints every figure).

Exact probes: x and w in {-1, 0, 1} as ``gemm_cases.integer_probe`` builds them; every partial sum
in any order is an integer below 2^24 and every output is an integer of magnitude <= 256, which
bf16 holds: ``torch.equal``. They run without activation (SiLU is not exact) and at K <= 256
(beyond it a ternary sum can pass 256).

Poison: every row of x that no group owns is NaN, every output element is NaN before the launch,
and the outputs sit inside canary rows (``out``: canary columns too). An element no group owns
must still be NaN afterwards, every owned one finite, every canary untouched.
"""
import functools
from collections import namedtuple

import torch

import gemm_cases as gc
import gemm_checks as gk

BF = torch.bfloat16
C = 2.0
assert C == gk.C_BOUND["swiglu"]
FAMILY = "moe_skinny"
# worst err / derived bound measured on an MI355X (test_moe_skinny_gpu.py prints each case's)
MEASURED = {"none": 0.9866, "swiglu": 0.984}  # (16, 32) counts (17, 0, 33, 5); (512, 256) counts (1, 0, 16, 7)

PLAIN_NK = ((16, 32), (48, 96), (256, 256), (256, 14336))
SWIGLU_NK = ((32, 32), (96, 160), (512, 256), (512, 4096))
COUNTS = ((0, 0, 0, 2), (1, 0, 16, 7), (16, 16, 16, 16), (0,) * 7 + (1,), (17, 0, 33, 5))
CASES = [("none", nk, c) for nk in PLAIN_NK for c in COUNTS] + [("swiglu", nk, c) for nk in SWIGLU_NK for c in COUNTS]
EXACT_CASES = [("none", nk, c) for nk in PLAIN_NK if nk[1] <= 256 for c in COUNTS]
LEAD, TAIL = 2, 3  # rows of x (no a_rows) before the first and after the last group: owned by nobody
CAP_BELOW = 20     # compact capacity of the multi-pass case: below its count of 33


def case_id(case):
    act, (N, K), counts = case
    return f"{act}-{N}x{K}-" + "_".join(str(c) for c in counts)


Case = namedtuple("Case", "act N K NO counts weights rows refs pres aps")


@functools.lru_cache(maxsize=None)
def build(act, nk, counts, kind="random"):
    """Weights, the R sorted rows (row r belongs to the group whose range holds it) and, per group,
    the float64 reference of its rows (out, pre-activation magnitude terms)."""
    N, K = nk
    E, R = len(counts), sum(counts)
    if kind == "integer":
        p = gc.integer_probe(max(R, 1), N * E, K)
        rows, wall = p.x[:R], p.w
    else:
        s = 9100 + N + 3 * K + 7 * R + E
        rows = gc._rand(R, K, scale=2.0, seed=s) + 0.4
        wall = gc._rand(N * E, K, scale=0.04 if act == "none" else 2.0 / K ** 0.5, seed=s + 1)
    weights = tuple(wall[e * N:(e + 1) * N].contiguous() for e in range(E))
    refs, pres, aps = [], [], []
    r = 0
    for e, c in enumerate(counts):
        x = rows[r:r + c]
        r += c
        if act == "swiglu":
            ref, ap = gk.ref64_swiglu(x, weights[e])
            pre = ref
        else:
            pre, ref = gk.ref64(x, weights[e])
            ap = gk.absprod64(x, weights[e])
        if kind == "integer" and c > 0:
            assert torch.equal((x.float() @ weights[e].float().T).double(), ref) and gk.absprod64(x, weights[e]).max() < 2 ** 24
            assert c == 0 or ref.abs().max().item() <= 256, "an output bf16 cannot hold"
        refs.append(ref)
        pres.append(pre)
        aps.append(ap)
    return Case(act, N, K, N // 2 if act == "swiglu" else N, counts, weights, rows, tuple(refs), tuple(pres), tuple(aps))


Run = namedtuple("Run", "x offsets a_rows out outs obuf cap mode")


def make_run(c, use_a_rows, mode, device):
    """Device buffers of one launch. ``mode``: "out" or "outs"."""
    E, R = len(c.counts), sum(c.counts)
    nan = float("nan")
    if use_a_rows:
        # token matrix: the R sorted rows scattered among as many NaN rows
        T = 2 * R + TAIL
        perm = torch.randperm(T, generator=gc._gen(9300 + R + c.K))[:R]
        x = torch.full((T, c.K), nan, dtype=BF)
        x[perm] = c.rows
        a_rows = perm.to(torch.int32).to(device)
        first = 0
    else:
        x = torch.full((LEAD + R + TAIL, c.K), nan, dtype=BF)
        x[LEAD:LEAD + R] = c.rows
        a_rows = None
        first = LEAD
    offs = [first]
    for n in c.counts:
        offs.append(offs[-1] + n)
    offsets = torch.tensor(offs, dtype=torch.int32, device=device)
    out_rows = R if use_a_rows else x.shape[0]
    if mode == "out":
        obuf = torch.full((out_rows + gc.PAD_ROWS, c.NO + 8), gc.CANARY, dtype=BF, device=device)
        out = obuf[:out_rows, :c.NO]
        out.fill_(nan)
        return Run(x.to(device), offsets, a_rows, out, None, obuf, 0, mode)
    cap = CAP_BELOW if max(c.counts) > CAP_BELOW else max(c.counts) + 1
    assert cap > max(c.counts) or c.counts == (17, 0, 33, 5)  # the multi-pass case alone is cut by its capacity
    obuf = torch.full((E * (cap + 1) + 1, c.NO), gc.CANARY, dtype=BF, device=device)
    outs = [obuf[1 + e * (cap + 1):1 + e * (cap + 1) + cap] for e in range(E)]
    for o in outs:
        o.fill_(nan)
    return Run(x.to(device), offsets, a_rows, None, outs, obuf, cap, mode)


_dev_weights = {}


def weights_on(c, device):
    key = (id(c.weights), str(device))
    if key not in _dev_weights:
        _dev_weights.clear()  # one case's weights at a time
        _dev_weights[key] = [w.to(device) for w in c.weights]
    return _dev_weights[key]


def launch(fn, c, run):
    fn(run.x, weights_on(c, run.x.device), run.offsets, act=None if c.act == "none" else c.act,
       out=run.out, outs=run.outs, a_rows=run.a_rows)


def group_outputs(c, run):
    """Per group: (its written rows as a CPU tensor, the rows of the reference they stand for)."""
    first = int(run.offsets[0])
    res = []
    r = first
    for e, n in enumerate(c.counts):
        if run.mode == "out":
            res.append((run.out[r:r + n].cpu(), n))
        else:
            res.append((run.outs[e][:min(n, run.cap)].cpu(), min(n, run.cap)))
        r += n
    return res


def verify(c, run, what, exact=False):
    """Every check of one finished launch; returns the worst err / derived bound (0 for exact)."""
    worst = 0.0
    for e, (got, n) in enumerate(group_outputs(c, run)):
        if n == 0:
            continue
        ref, pre, ap = c.refs[e][:n], c.pres[e][:n], c.aps[e][:n]
        if exact:
            gk.check_exact(got, ref.to(BF), f"{what} group {e}")
        else:
            worst = max(worst, gk.check_bound(got, pre, ref, ap, c.K, FAMILY, f"{what} group {e}", C=C))
    # what nobody owns is still NaN, the canaries are whole
    ob = run.obuf.cpu()
    if run.mode == "out":
        o = run.out.cpu()
        first, R = int(run.offsets[0]), sum(c.counts)
        assert bool(o[:first].isnan().all()) and bool(o[first + R:].isnan().all()), f"{what}: a row no group owns was written"
        assert bool((ob[o.shape[0]:] == gc.CANARY).all()), f"{what}: rows past the output were written"
        assert bool((ob[:o.shape[0], c.NO:] == gc.CANARY).all()), f"{what}: columns past N' were written"
    else:
        keep = torch.ones(ob.shape[0], dtype=torch.bool)
        for e, n in enumerate(c.counts):
            base = 1 + e * (run.cap + 1)
            keep[base:base + run.cap] = False
            tail = run.outs[e][min(n, run.cap):].cpu()
            assert bool(tail.isnan().all()), f"{what}: group {e} wrote past its min(count, capacity) rows"
        assert bool((ob[keep] == gc.CANARY).all()), f"{what}: a canary row between the compact outputs was written"
    return worst


def bits(run):
    return run.obuf.cpu().view(torch.int16)


VARIANTS = [(a, m) for a in (False, True) for m in ("out", "outs")]


def run_case(fn, case, device, exact=False):
    """All four variants of a case through ``fn`` (the signature of ops.gemm_grouped_skinny), each
    launched twice into fresh buffers: checked, and bit-identical."""
    act, nk, counts = case
    c = build(act, nk, counts, "integer" if exact else "random")
    worst = 0.0
    for use_a_rows, mode in VARIANTS:
        what = f"{case_id(case)} a_rows={int(use_a_rows)} {mode}"
        r1 = make_run(c, use_a_rows, mode, device)
        launch(fn, c, r1)
        worst = max(worst, verify(c, r1, what, exact))
        r2 = make_run(c, use_a_rows, mode, device)
        launch(fn, c, r2)
        assert torch.equal(bits(r1), bits(r2)), f"{what}: two launches differ"
    print(f"moe_skinny worst ratio {case_id(case)}: {worst:.4g}")
    return worst


# ---------------------------------------------------------------------------------------------
# What subtly wrong kernels would return (the oracle self-check of test_moe_skinny_cpu.py)

WAVES, SLICE = 4, 64


def mutant(name):
    """A CPU stand-in with the op's signature and one defect: "first_wave_only" sums only the first
    wave's run of K slices; "gate_up_off_by_one" pairs gate block c with up block c + 1."""
    from distributed_llm_scheduler_amd import ops

    def fn(x, weights, offsets, act=None, out=None, outs=None, a_rows=None):
        N, K = weights[0].shape
        ws = list(weights)
        if name == "first_wave_only":
            nk = -(-K // SLICE)
            k1 = min(K, -(-nk // WAVES) * SLICE)
            if k1 < K:
                ws = [torch.cat([w[:, :k1], torch.zeros_like(w[:, k1:])], 1) for w in ws]
        elif name == "gate_up_off_by_one" and act == "swiglu":
            ws = []
            for w in weights:
                v = w.reshape(N // 32, 2, 16, K).clone()
                v[:, 1] = torch.roll(v[:, 1], -1, 0)
                ws.append(v.reshape(N, K))
        return ops.gemm_grouped_skinny(x, ws, offsets, act=act, out=out, outs=outs, a_rows=a_rows)
    return fn
