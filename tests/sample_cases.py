"""Inputs and the oracle shared by the CPU and GPU tests of token sampling (test_sample_cpu.py,
test_sample_gpu.py; test_generate_*.py use the acceptance on the executor's own logits), built on
the CPU from fixed seeds, once per process.

A case is one launch of ``ops.sample_tokens``: B sequences, T logits rows each of which only row
``b*T + T-1`` may be read, V valid columns of a padded row, per-sequence (temperature, top_k,
top_p), a seed, a request ordinal, and a sentinel-filled token stream [B][C]. Pad columns and the
rows that must not be read hold +inf: a kernel that reads one as a candidate picks it.

The oracle is float64 and independent of ``ops``: its own Philox4x32-10 (held to three published
vectors by test_sample_cpu.py), theta_k by sorting, weights by ``exp``. A result is never compared
with an fp64 draw for equality: with thousands of kept tokens the cumulative boundaries lie closer
than fp32 resolves. ``accept`` asks instead, at the implementation's own threshold stats[0]:

* greedy: the token is the lowest index of the maximum and stats == (l_max, 1, 0, 1), exactly;
* p >= 1: theta == theta_k exactly; p < 1: theta is a value of the row that is >= theta_k (top-k is
  integer counting, so exact), the weight strictly above its class is < p Z1 + eps Z1 and the
  weight including its class is >= p Z1 - eps Z1;
* the token is kept and its fp64 cumulative interval [c, c + w] under that theta meets
  [u Z - eps Z, u Z + eps Z]; the reported Z, c and w are within eps Z of the fp64 ones.
"""
import dataclasses
import functools
import itertools
import math

import torch

SENTINEL = -7  # fills the token streams
CAP = 16  # stream capacity C of the cases

# The window. On an MI355X test_sample_gpu.py prints max(|Z - Z_ref|, |c - c_ref|) / Z_ref over every
# row of every case, references taken at the kernel's own theta and token. EPS is three times the
# measured figure rounded up to a power of two and may not exceed 2^-14: above that the
# arithmetic is to be fixed, not the window. Measured: 1.059e-7 in tie_at_theta_k_v50257 over
# the 33 cases (the kernel sums 2^-40 fixed-point weights exactly; what is left is the fp32 exp
# and the fp32 rounding of the reported sums), so EPS is 2^-21.
MEASURED_ERR = 1.059e-7
EPS = 2.0 ** math.ceil(math.log2(3 * MEASURED_ERR))
assert EPS <= 2.0 ** -14

TAUS = (0.0, 0.25, 1.0, 4.0)
PS = (1e-6, 0.5, 0.9, 1.0)
VS = (1, 7, 333, 50257, 128256)


def top_ks(V):
    return (0, 1, 2, 50, V, V + 5)


# ---------------------------------------------------------------- Philox4x32-10 (Salmon et al. 2011)
def _mulhilo(a, b):
    p = a * b
    return p >> 32, p & 0xFFFFFFFF


def philox(counter, key):
    c = [x & 0xFFFFFFFF for x in counter]
    k = [x & 0xFFFFFFFF for x in key]
    for _ in range(10):
        h0, l0 = _mulhilo(0xD2511F53, c[0])
        h1, l1 = _mulhilo(0xCD9E8D57, c[2])
        c = [h1 ^ c[1] ^ k[0], l1, h0 ^ c[3] ^ k[1], l0]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return tuple(c)


PHILOX_VECTORS = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)


def uniform(seed, request, b, n):
    seed &= (1 << 64) - 1
    return (philox((n, b, request, 0), (seed & 0xFFFFFFFF, seed >> 32))[0] >> 8) / float(1 << 24)


# ---------------------------------------------------------------- the kernel's slicing
def slices(B, V):
    """(workgroups per row, elements per workgroup) of csrc/kernels/sample.hip; the GPU test
    holds this to ``ops.sample_slices``. The tie cases put equal maxima on both sides of every
    boundary."""
    S = max(1, min(64, -(-V // 8192), 512 // max(B, 1)))
    length = -(-(-(-V // 8)) // S) * 8
    return -(-V // length), length


# ---------------------------------------------------------------- cases
@dataclasses.dataclass(eq=False)
class Case:
    name: str
    logits: torch.Tensor  # bf16 [B*T][ld], poisoned outside the valid rows and columns
    V: int
    T: int
    src: tuple  # per sequence: its row in ``rows`` (identical sequences share one)
    rows: tuple  # the distinct logits rows, float64 [V]
    pos: tuple
    tau: tuple
    k: tuple
    p: tuple
    seed: int
    request: int = 0

    @property
    def B(self):
        return len(self.src)

    def n(self, b):
        return self.pos[b] + self.T


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn_row(V, g, scale=3.0):
    return (torch.randn(V, generator=g) * scale).to(torch.bfloat16)


def _make(name, rows, src, T, tau, k, p, seed, request=0, pos=None):
    """rows: distinct bf16 [V] rows; src[b]: the row of sequence b."""
    V = rows[0].numel()
    B = len(src)
    ld = -(-V // 64) * 64
    logits = torch.full((B * T, ld), math.inf, dtype=torch.bfloat16)
    for b, r in enumerate(src):
        logits[b * T + T - 1, :V] = rows[r]
    pos = tuple(pos) if pos is not None else tuple((5 * b + 3) % (CAP - T) for b in range(B))

    def per(x):
        return tuple(x) if isinstance(x, (tuple, list)) else (x,) * B

    return Case(name, logits, V, T, tuple(src), tuple(r.double() for r in rows), pos, per(tau), per(k), per(p), seed,
                request)


def _grid(V):
    """One row, every (tau, k, p) of the issue's product, one sequence each."""
    combos = list(itertools.product(TAUS, top_ks(V), PS))
    row = _randn_row(V, _gen(100 + V))
    return _make(f"grid_v{V}", [row], [0] * len(combos), 1, [c[0] for c in combos], [c[1] for c in combos],
                 [c[2] for c in combos], seed=0x1234567 + V, request=V % 3)


def _draws(V, tau, k, p, T, tag):
    """64 identical rows that differ in (b, n): 64 draws of one distribution per launch."""
    row = _randn_row(V, _gen(200 + V))
    return _make(f"draws_v{V}_{tag}", [row], [0] * 64, T, tau, k, p, seed=(0xDEADBEEF << 20) + V,
                 pos=[(3 * b) % (CAP - T) for b in range(64)])


def _distinct(V, B, T):
    """Distinct rows, mixed parameters: greedy rows next to sampling rows."""
    g = _gen(300 + V + B)
    rows = [_randn_row(V, g, scale=1.0 + 2.0 * b) for b in range(B)]
    tau = [(1.0, 0.0, 0.25)[b % 3] for b in range(B)]
    k = [(50, 2, 0)[b % 3] for b in range(B)]
    p = [(0.9, 0.5, 1.0)[b % 3] for b in range(B)]
    return _make(f"distinct_v{V}_b{B}_t{T}", rows, list(range(B)), T, tau, k, p, seed=-12345 - V, request=1)


def _ties(V, tau, k, p, tag):
    """The maximum repeated at 0, mid and V-1, and on both sides of every slice boundary."""
    S, length = slices(32, V)
    bounds = [s * length for s in range(1, S)]
    sets = [[0, V // 2, V - 1], [V // 2, V - 1], [V - 1]] + [[x - 1, x] for x in bounds] + [bounds + [V - 1]]
    assert len(sets) <= 32 and slices(len(sets), V) == (S, length)
    base = _randn_row(V, _gen(400 + V))
    top = (base.float().max() + 1.0).to(torch.bfloat16)
    rows = []
    for idx in sets:
        r = base.clone()
        r[idx] = top
        rows.append(r)
    return _make(f"ties_v{V}_{tag}", rows, list(range(len(rows))), 1, tau, k, p, seed=77 + V)


def _all_equal(V):
    row = torch.full((V,), 1.5, dtype=torch.bfloat16)
    return _make(f"all_equal_v{V}", [row], [0] * 6, 4, [0.0, 1.0, 1.0, 0.25, 4.0, 1.0], [0, 5, 0, 1, V, 2],
                 [1.0, 0.5, 1e-6, 0.9, 1.0, 1.0], seed=5)


def _tie_at_theta_k(V):
    """A class of 1000 equal values that holds the 50th largest: top-k keeps all of it."""
    g = _gen(500 + V)
    row = _randn_row(V, g)
    v30 = row.float().sort(descending=True).values[30]
    idx = torch.randperm(V, generator=g)[:1000]
    row[idx] = v30.to(torch.bfloat16)
    return _make(f"tie_at_theta_k_v{V}", [row], [0] * 8, 1, [1.0, 1.0, 0.25, 4.0, 1.0, 1.0, 0.0, 4.0],
                 [50, 50, 50, 50, 31, 1030, 50, 200], [1.0, 0.9, 0.5, 1.0, 1.0, 0.9, 0.9, 1e-6], seed=9)


def _neg_inf(V, finite):
    g = _gen(600 + V + finite)
    row = _randn_row(V, g)
    dead = torch.randperm(V, generator=g)[:V - finite]
    row[dead] = -math.inf
    return _make(f"neg_inf_v{V}_f{finite}", [row], [0] * 6, 4, [1.0, 0.0, 4.0, 0.25, 1.0, 1.0], [50, 0, 0, 2, V, 1],
                 [1.0, 1.0, 0.9, 0.5, 0.5, 1.0], seed=11)


_SPECS = (
    [(f"grid_v{V}", _grid, (V,)) for V in VS]
    + [(f"draws_v{V}_k50", _draws, (V, 1.0, 50, 0.9, 4, "k50")) for V in (333, 50257, 128256)]
    + [(f"draws_v{V}_open", _draws, (V, 4.0, 0, 1.0, 1, "open")) for V in (7, 50257, 128256)]
    + [(f"draws_v{V}_p", _draws, (V, 0.25, 0, 0.5, 1, "p")) for V in (333, 128256)]
    + [(f"distinct_v{V}_b3_t4", _distinct, (V, 3, 4)) for V in VS]
    + [(f"distinct_v{V}_b1_t1", _distinct, (V, 1, 1)) for V in VS]
    + [(f"ties_v{V}_greedy", _ties, (V, 0.0, 0, 1.0, "greedy")) for V in (50257, 128256)]
    + [(f"ties_v{V}_k1", _ties, (V, 1.0, 1, 0.5, "k1")) for V in (50257, 128256)]
    + [(f"all_equal_v{V}", _all_equal, (V,)) for V in (333, 50257)]
    + [(f"tie_at_theta_k_v{V}", _tie_at_theta_k, (V,)) for V in (50257,)]
    + [("neg_inf_v7_f1", _neg_inf, (7, 1)), ("neg_inf_v333_f3", _neg_inf, (333, 3)),
       ("neg_inf_v50257_f45000", _neg_inf, (50257, 45000))]
)
_BUILDERS = {name: (fn, args) for name, fn, args in _SPECS}
CASES = tuple(_BUILDERS)
DETERMINISM_CASES = ("grid_v128256", "draws_v50257_k50", "ties_v128256_k1")


@functools.lru_cache(maxsize=None)
def case(name):
    fn, args = _BUILDERS[name]
    c = fn(*args)
    assert c.name == name
    return c


# ---------------------------------------------------------------- running a case through ``ops``
def run(ops, c, device, workspace=None):
    """(next [B], stats [B][4], stream [B][C]) of one launch, on the CPU."""
    dev = torch.device(device)
    B = c.B
    stream = torch.full((B, CAP), SENTINEL, dtype=torch.int32, device=dev)
    if workspace is None:
        workspace = ops.sample_workspace(B, c.V, dev)
    nxt, stats = ops.sample_tokens(
        c.logits.to(dev), c.V, c.T, torch.tensor(c.pos, dtype=torch.int32, device=dev), stream, CAP,
        torch.tensor(c.tau, dtype=torch.float32, device=dev), torch.tensor(c.k, dtype=torch.int32, device=dev),
        torch.tensor(c.p, dtype=torch.float32, device=dev), c.seed, request=c.request, workspace=workspace)
    return nxt.cpu(), stats.cpu().view(B, 4), stream.cpu()


# ---------------------------------------------------------------- the oracle
def first_argmax(l):
    return int((l == l.max()).nonzero()[0])


def theta_k(sorted_desc, k):
    V = sorted_desc.numel()
    return float(sorted_desc[k - 1]) if 0 < k < V else -math.inf


def accept(l, tau, k, p, u, token, stats, eps, what="", sorted_desc=None):
    """Hold one row's (token, stats) to the contract (module docstring); ``l`` float64 [V], ``p``
    and ``tau`` the fp32 values the implementation saw. Returns the row's measured error
    max(|Z - Z_ref|, |c - c_ref|) / Z_ref (0 for a greedy row)."""
    V = l.numel()
    theta, Z, before, wtok = (float(x) for x in stats)
    assert 0 <= token < V, f"{what}: token {token} outside the vocabulary of {V}"
    lmax = float(l.max())
    if not tau > 0:
        assert token == first_argmax(l), f"{what}: greedy token {token}, lowest argmax {first_argmax(l)}"
        assert (theta, Z, before, wtok) == (lmax, 1.0, 0.0, 1.0), f"{what}: greedy stats {stats.tolist()}"
        return 0.0
    if sorted_desc is None:
        sorted_desc = l.sort(descending=True).values
    tk = theta_k(sorted_desc, k)
    w = torch.exp((l - lmax) / tau)
    if p >= 1:
        assert theta == tk, f"{what}: theta {theta} != theta_k {tk} with top-p off"
    else:
        assert theta >= tk and bool((l == theta).any()), f"{what}: theta {theta} is no kept value (theta_k {tk})"
        Z1 = float(w[l >= tk].sum())
        above, incl = float(w[l > theta].sum()), float(w[l >= theta].sum())
        assert above < p * Z1 + eps * Z1, f"{what}: theta {theta} too low: {above / Z1} above it already reaches p {p}"
        assert incl >= p * Z1 - eps * Z1, f"{what}: theta {theta} too high: {incl / Z1} with it misses p {p}"
    kept = l >= theta
    assert bool(kept[token]), f"{what}: token {token} (logit {float(l[token])}) is below theta {theta}"
    Zr = float(w[kept].sum())
    cr = float(w[:token][kept[:token]].sum())
    wr = float(w[token])
    assert cr <= u * Zr + eps * Zr and cr + wr >= u * Zr - eps * Zr, \
        f"{what}: token {token} covers [{cr / Zr}, {(cr + wr) / Zr}] of the kept weight, the draw is {u}"
    err = max(abs(Z - Zr), abs(before - cr)) / Zr
    assert err <= eps and abs(wtok - wr) <= eps * Zr, \
        f"{what}: stats (Z {Z}, before {before}, w {wtok}) against fp64 ({Zr}, {cr}, {wr}): {err} > eps {eps}"
    return err


def check(c, nxt, stats, stream, eps=EPS):
    """Every row of a case against the oracle, and the stream: with no prompt and n < C exactly
    the cell [b][n] changed, to the token. Returns the largest measured error."""
    worst = 0.0
    sd = [r.sort(descending=True).values for r in c.rows]
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
    for b in range(c.B):
        l = c.rows[c.src[b]]
        n = c.n(b)
        err = accept(l, f32(c.tau[b]), c.k[b], f32(c.p[b]), uniform(c.seed, c.request, b, n), int(nxt[b]), stats[b],
                     eps, f"{c.name} row {b} (tau {c.tau[b]}, k {c.k[b]}, p {c.p[b]})", sd[c.src[b]])
        worst = max(worst, err)
        want = torch.full((CAP,), SENTINEL, dtype=torch.int32)
        if n < CAP:
            want[n] = int(nxt[b])
        assert torch.equal(stream[b], want), f"{c.name} row {b}: stream {stream[b].tolist()}"
    return worst


# ---------------------------------------------------------------- the stream rule
def check_stream_rule(ops, device):
    """Prompt forcing, the capacity and a sticky eos against sentinel-filled streams, whole streams
    compared: exactly one cell changes per sequence, or none. Greedy rows: the drawn token is the
    row's lowest argmax."""
    dev = torch.device(device)
    V, B, C = 333, 4, 8
    g = _gen(700)
    first = torch.stack([_randn_row(V, g) for _ in range(B)])
    second = torch.stack([_randn_row(V, g) for _ in range(B)])
    am1 = [first_argmax(r.double()) for r in first]
    am2 = [first_argmax(r.double()) for r in second]
    assert all(a != b for a, b in zip(am1, am2))

    def launch(rows, pos, stream, prompt_len=None, eos=-1, done=None):
        logits = torch.full((B, 384), math.inf, dtype=torch.bfloat16)
        logits[:, :V] = rows
        i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
        s = stream.to(dev)
        d = None if done is None else done.to(dev)
        nxt, _ = ops.sample_tokens(logits.to(dev), V, 1, i32(pos), s, C, torch.zeros(B, device=dev), i32([0] * B),
                                   torch.ones(B, device=dev), 3, prompt_len=None if prompt_len is None else
                                   i32(prompt_len), eos=eos, done=d, workspace=ops.sample_workspace(B, V, dev))
        return nxt.cpu().tolist(), s.cpu(), None if d is None else d.cpu().tolist()

    # the prompt: n < prompt_len is forced and nothing is written; n == prompt_len is the first written
    plen = [5, 5, 0, 3]
    stream = torch.full((B, C), SENTINEL, dtype=torch.int32)
    for b, pl in enumerate(plen):
        stream[b, :pl] = torch.arange(100 + 10 * b, 100 + 10 * b + pl, dtype=torch.int32)
    pos = [2, 4, 2, 2]  # n = 3, 5, 3, 3
    nxt, after, _ = launch(first, pos, stream, prompt_len=plen)
    want = stream.clone()
    want[1, 5], want[2, 3], want[3, 3] = am1[1], am1[2], am1[3]
    assert nxt == [int(stream[0, 3]), am1[1], am1[2], am1[3]] and torch.equal(after, want), (nxt, after.tolist())

    # the capacity: n == C - 1 is the last cell written, at n == C and past it nothing is
    stream = torch.full((B, C), SENTINEL, dtype=torch.int32)
    nxt, after, _ = launch(first, [C - 2, C - 1, C, 0], stream)
    want = stream.clone()
    want[0, C - 1], want[3, 1] = am1[0], am1[3]
    assert nxt == am1 and torch.equal(after, want), (nxt, after.tolist())

    # eos: hit by sequence 0 only; then sticky whatever the logits say; never set inside a prompt
    eos = am1[0]
    stream = torch.full((B, C), SENTINEL, dtype=torch.int32)
    stream[3, :4] = eos  # sequence 3 is inside a prompt made of eos
    done = torch.zeros(B, dtype=torch.int32)
    nxt, after, d = launch(first, [0, 0, 0, 0], stream, prompt_len=[0, 0, 0, 4], eos=eos, done=done)
    want = stream.clone()
    want[0, 1], want[1, 1], want[2, 1] = eos, am1[1], am1[2]
    assert nxt == [eos, am1[1], am1[2], eos] and d == [1, 0, 0, 0] and torch.equal(after, want), (nxt, d)
    nxt2, after2, d2 = launch(second, [1, 1, 1, 1], after, prompt_len=[0, 0, 0, 4], eos=eos,
                              done=torch.tensor(d, dtype=torch.int32))
    want[0, 2], want[1, 2], want[2, 2] = eos, am2[1], am2[2]
    assert nxt2 == [eos, am2[1], am2[2], eos] and d2 == [1, 0, 0, 0] and torch.equal(after2, want), (nxt2, d2)
    # no eos: the same first launch sets nothing
    _n, _s, d3 = launch(first, [0, 0, 0, 0], stream, eos=-1, done=torch.zeros(B, dtype=torch.int32))
    assert d3 == [0, 0, 0, 0]
