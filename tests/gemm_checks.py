"""References, checks, a model of an honest kernel and mutants of it, shared by the CPU and GPU
tests of the bf16 GEMM (test_gemm_ref_cpu.py, test_gemm_exact_gpu.py) on the inputs of
gemm_cases.py.

``ref64`` is the GEMM and its epilogue in float64, written independently of ``ops.ref_linear``
(the CPU path of ``ops.linear`` and the oracle of the older GPU tests). The exact probes compare
with ``torch.equal``; epilogues that cannot be exact (GELU, SiLU, SwiGLU, RoPE, the folded and
post norms, random data) are held to a bound per ELEMENT:

    |out - ref| <= C * (2^-9 * (|pre| + |ref|) + K * 2^-24 * (|x| @ |w|^T))

``pre`` is the value before the residual add. It is rounded to bf16 once and the sum once more;
half a bf16 ulp is between 2^-9 and 2^-8 of a value, so two honest roundings reach at most twice
the first term. The last term is the fp32 accumulation of K products. A global
``max|err| <= 2e-2 * max|ref|`` lets one dropped K element, a bias shifted by a column or a skipped
residual pass; this bound is some thirty times tighter where the reference is small.
"""
import math

import torch

import gemm_cases as gc

BF = torch.bfloat16
EPS = 1e-5

# Largest err / derived bound per epilogue family, measured on an MI355X over the bounded cases of
# test_gemm_exact_gpu.py (the tests print every figure) — with the case that reached it. C is
# 1.5 x that, rounded up to a power of two. Two honest bf16 roundings alone reach 2 (see above);
# no family comes near 4: the fast __expf of GELU / SiLU / SwiGLU and the rsqrtf of the norms do
# not show next to the output rounding.
MEASURED = {
    "linear": 1.729,     # config 38, bias + relu + residual, (133, 120, 768)
    "gelu": 1.726,       # config 38, bias + gelu + residual, (133, 120, 768)
    "silu": 0.9306,      # config 44, bias + silu, (165, 258, 768)
    "swiglu": 0.9411,    # config 44, (165, 288, 768)
    "rope": 1.644,       # config 38, bias + RoPE + residual, (133, 98, 768)
    "layernorm": 0.8623,  # config 13, handed-over statistics + gelu, (261, 280, 768)
    "rmsnorm": 0.8722,   # config 13, in-kernel statistics, (261, 258, 768)
    "postnorm": 1.313,   # config 13, RMSNorm from the norm kernel, (261, 280, 768)
}
C_BOUND = {f: 2.0 ** math.ceil(math.log2(1.5 * m)) for f, m in MEASURED.items()}  # 4: linear, gelu, rope; 2: the rest
assert max(C_BOUND.values()) <= 4.0
# stats_out against the float64 sums of the returned output: at most 0.034 of its N * 2^-24 allowance

ratios = {}  # family -> worst err / derived bound seen (the GPU tests print it: the source of C_BOUND)


# ---------------------------------------------------------------------------------------------
# float64 references

def act64(v, act):
    if act in (None, "none"):
        return v
    if act == "relu":
        return v.clamp_min(0.0)
    if act == "silu":
        return v * torch.sigmoid(v)
    if act == "gelu":  # the tanh form
        return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))
    raise ValueError(act)


def acc64(x, w):
    return x.double() @ w.double().T


def absprod64(x, w):
    return x.double().abs() @ w.double().abs().T


def ref64(x, w, bias=None, act=None, res=None, alpha=1.0):
    """(pre, out) in float64, nothing rounded: pre = act(alpha * x @ w^T + bias), out = pre + res."""
    v = alpha * acc64(x, w)
    if bias is not None:
        v = v + bias.double()
    pre = act64(v, act)
    return pre, pre if res is None else pre + res.double()


def ref64_swiglu(x, w, bias=None, alpha=1.0):
    """W rows interleave gate / up blocks of 16; (out, absprod) with out = silu(gate) * up."""
    v = alpha * acc64(x, w)
    if bias is not None:
        v = v + bias.double()
    M, N = v.shape
    v = v.reshape(M, N // 32, 2, 16)
    ap = absprod64(x, w).reshape(M, N // 32, 2, 16).sum(2)
    return (act64(v[:, :, 0], "silu") * v[:, :, 1]).reshape(M, N // 2), ap.reshape(M, N // 2)


def ref64_rope(x, w, bias, cos_t, sin_t, S, D, cols):
    """Adjacent column pairs of the first ``cols`` outputs rotated by the row's position
    (row % S); (out, absprod) with a pair's two |x| @ |w| sums added."""
    v = acc64(x, w) + (0 if bias is None else bias.double())
    ap = absprod64(x, w)
    M = v.shape[0]
    pos = torch.arange(M) % S
    c, s = cos_t.double()[pos][:, None, :], sin_t.double()[pos][:, None, :]
    p = v[:, :cols].reshape(M, cols // D, D // 2, 2)
    rot = torch.stack([p[..., 0] * c - p[..., 1] * s, p[..., 1] * c + p[..., 0] * s], -1).reshape(M, cols)
    a2 = ap[:, :cols].reshape(M, cols // 2, 2).sum(2).repeat_interleave(2, dim=1)
    return torch.cat([rot, v[:, cols:]], 1), torch.cat([a2, ap[:, cols:]], 1)


def row_stats64(x, stats=None):
    """(mean, mean of squares) of each row: from x in float64, or from the fp32 (sum, sum of
    squares) the kernel is handed."""
    K = x.shape[1]
    if stats is None:
        xd = x.double()
        s, ss = xd.sum(1), (xd * xd).sum(1)
    else:
        s, ss = stats.double()[:, 0], stats.double()[:, 1]
    return s / K, ss / K


def ref64_folded(x, wd, cs, bd, mode, act=None, stats=None):
    """A norm folded into the GEMM, on the operands the kernel receives: the derived bf16 weight,
    its fp32 column sums, the derived bf16 bias and (``stats``) the fp32 row sums.
    LayerNorm: rstd * (x @ wd^T - mu * cs) + bd; RMSNorm: no mean."""
    mu, ms = row_stats64(x, stats)
    if mode == "layernorm":
        rs = 1.0 / torch.sqrt(ms - mu * mu + EPS)
        v = rs[:, None] * (acc64(x, wd) - mu[:, None] * cs.double()[None, :])
    else:
        rs = 1.0 / torch.sqrt(ms + EPS)
        v = rs[:, None] * acc64(x, wd)
    pre = act64(v + bd.double(), act)
    return pre, pre


def ref64_postnorm(out, nw, nb, mode):
    """The next norm of the GEMM's output rows, float64: (normalised rows before the gain, rstd)."""
    mu = out.mean(1, keepdim=True) if mode == "layernorm" else torch.zeros(out.shape[0], 1, dtype=torch.float64)
    rs = 1.0 / torch.sqrt(((out - mu) ** 2).mean(1, keepdim=True) + EPS)
    z = (out - mu) * rs
    y = z * nw.double() + (nb.double() if mode == "layernorm" else 0.0)
    return y, z, rs


# ---------------------------------------------------------------------------------------------
# Exact probes

def expected_exact(p, epi):
    """The one output every correct summation order gives, as bf16 (asserts it is exact)."""
    bias, res, act, alpha = gc.operands(p, epi)
    pre, out = ref64(p.x, p.w, bias, act, res, alpha)
    want = out.to(BF)
    assert torch.equal(want.double(), out), "the probe's output is not exact in bf16"
    return want


def _bf16_exact(v):
    return bool(torch.equal(v.to(BF).double(), v))


def check_probe_preconditions(p, epi):
    """What makes ``torch.equal`` the right metric for a probe; returns the largest magnitude an
    epilogue forms."""
    bias, res, act, alpha = gc.operands(p, epi)
    acc = acc64(p.x, p.w)
    assert torch.equal((p.x.float() @ p.w.float().T).double(), acc), "fp32 and fp64 products differ"
    worst = 0.0
    if p.kind == "integer":
        for name, t in (("x", p.x), ("w", p.w)):
            f = t.float()
            assert bool(((f == 0) | (f.abs() == 1)).all()), f"{name} outside {{-1, 0, 1}}"
            assert 0.70 < (f != 0).float().mean().item() < 0.80, f"{name}: not 75 % non-zeros"
        assert bool((p.bias.float().abs() <= 8).all()) and bool((p.bias.float() % 1 == 0).all())
        assert bool((p.res.float().abs() <= 16).all()) and bool((p.res.float() % 1 == 0).all())
        # an upper bound of every partial sum in any order: the sum of the magnitudes, below 2^24
        assert absprod64(p.x, p.w).max().item() < 2 ** 24
        steps = [acc, alpha * acc]
        steps.append(steps[-1] + (0 if bias is None else bias.double()))
        steps.append(act64(steps[-1], act))
        steps.append(steps[-1] + (0 if res is None else res.double()))
        for v in steps:
            assert bool(((2 * v) % 1 == 0).all()), "a value that is neither an integer nor a half-integer"
            assert v.abs().max().item() <= 256 and _bf16_exact(v), "an intermediate value bf16 cannot hold"
            worst = max(worst, v.abs().max().item())
    elif p.kind == "scaled":
        q = gc.integer_probe(*_mnk(p))
        sx = torch.pow(2.0, (torch.arange(p.x.shape[0]) % 5 - 2).double())[:, None]
        sw = torch.pow(2.0, (torch.arange(p.w.shape[0]) % 7 - 3).double())[:, None]
        assert torch.equal(p.x.double(), q.x.double() * sx) and torch.equal(p.w.double(), q.w.double() * sw)
        ints = acc / (sx * sw.T)  # output (m, n) = one power of two times the integer sum
        assert torch.equal(ints, acc64(q.x, q.w)) and ints.abs().max().item() <= 256
        assert absprod64(q.x, q.w).max().item() < 2 ** 24
        for v in (acc, alpha * acc, act64(alpha * acc, act)):
            assert _bf16_exact(v)
        worst = ints.abs().max().item()
    else:
        M, K = p.x.shape
        sel = gc.selector_k(M, K)
        assert bool((p.x.float().sum(1) == 1).all()) and bool((p.x.float()[torch.arange(M), sel] == 1).all())
        wf = p.w.float()
        assert bool(torch.isfinite(wf).all()) and bool((wf != 0).all()), "selector W holds a zero, Inf or NaN"
        mag = wf.abs()
        assert mag.min().item() >= 2.0 ** -30 and mag.max().item() < 2.0 ** 31
        assert mag.min().item() < 2.0 ** -25 and mag.max().item() > 2.0 ** 25, "magnitudes do not span 2^+-30"
        mant = p.w.view(torch.int16).to(torch.int32) & 127
        assert len(mant.unique()) == 128, "not every mantissa occurs"
        assert len(sel.unique()) > 1
        assert torch.equal(acc, wf.double()[:, sel].T), "the selected column is not the exact product"
        assert _bf16_exact(act64(alpha * acc, act))
        worst = mag.max().item()
    return worst


def _mnk(p):
    return p.x.shape[0], p.w.shape[0], p.x.shape[1]


def check_exact(out, want, what):
    """``out`` equals ``want`` (bf16) bit for bit, signs of zero aside (torch.equal: -0 == 0)."""
    o = out.detach().cpu()
    assert o.dtype == want.dtype and o.shape == want.shape, f"{what}: output {tuple(o.shape)} {o.dtype}"
    if not torch.equal(o, want):
        bad = (o != want) | (o.isnan() != want.isnan())
        r, c = (int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {o.numel()} outputs differ, first at ({r}, {c}): "
                             f"{o[r, c].item()} != {want[r, c].item()}")


def check_poison_placement(pd, M, N, K):
    """The padding of every operand buffer is NaN (canary for the output), the views hold the data."""
    assert pd.abuf.shape == (M + gc.PAD_ROWS, K + 8) and pd.wbuf.shape == (N + gc.PAD_ROWS, K + 16)
    assert pd.a.stride(0) == K + 8 and pd.w.stride(0) == K + 16
    for buf, r, c in ((pd.abuf, M, K), (pd.wbuf, N, K)) + (((pd.rbuf, M, N),) if pd.rbuf is not None else ()):
        b = buf.cpu()
        assert bool(b[r:].isnan().all()) and bool(b[:r, c:].isnan().all()), "padding that is not NaN"
        assert not bool(b[:r, :c].isnan().any())
    assert bool((pd.obuf.cpu() == gc.CANARY).all())


def check_canary(pd, M, N, res, what):
    """Nothing outside the [M][N] output view was written; the residual buffer is as it was."""
    o = pd.obuf.cpu()
    assert bool((o[M:] == gc.CANARY).all()), f"{what}: rows past M were written"
    assert bool((o[:M, N:] == gc.CANARY).all()), f"{what}: bytes past column N were written"
    if pd.rbuf is not None:
        r = pd.rbuf.cpu()
        assert bool(r[M:].isnan().all()) and bool(r[:M, N:].isnan().all()) and torch.equal(r[:M, :N], res), \
            f"{what}: the residual buffer was written"


# ---------------------------------------------------------------------------------------------
# Per-element bound

def derived_bound(pre, ref, absprod, K):
    return 2.0 ** -9 * (pre.abs() + ref.abs()) + K * 2.0 ** -24 * absprod


def check_bound(out, pre, ref, absprod, K, family, what, C=None):
    """Every element of ``out`` within C x the derived bound of ``ref`` (float64); returns the
    largest err / derived bound."""
    o = out.detach().cpu().double()
    assert o.shape == ref.shape, f"{what}: output {tuple(o.shape)} for reference {tuple(ref.shape)}"
    assert bool(torch.isfinite(o).all()), f"{what}: the output holds a value that is not finite"
    d = derived_bound(pre, ref, absprod, K)
    err = (o - ref).abs()
    ratio = torch.where(d > 0, err / d.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), err))
    worst = ratio.max().item()
    ratios[family] = max(worst, ratios.get(family, 0.0))
    print(f"bound ratio {family} {what}: {worst:.4g}")
    C = C_BOUND[family] if C is None else C
    if not worst <= C:
        r, c = (int(v) for v in (ratio == ratio.max()).nonzero()[0])
        raise AssertionError(f"{what}: |err| {err[r, c].item():.4g} is {worst:.4g} x the derived bound "
                             f"{d[r, c].item():.4g} at ({r}, {c}) (allowed {C}); {int((ratio > C).sum())} of "
                             f"{ratio.numel()} outputs are outside")
    return worst


def postnorm_bound(out, pre, absprod, K, z, rs, nw, y, mode):
    """Derived bound of the post-norm y = z * nw (+ nb), z = (c - mu) * rstd, for an input c that
    carries the GEMM's derived bound E: dy <= rstd |nw| (E + mean E + |z| mean(|z| E)) (the mean
    term: LayerNorm only), plus the rounding of y itself."""
    E = derived_bound(pre, out, absprod, K)
    mean_e = E.mean(1, keepdim=True) if mode == "layernorm" else 0.0
    return 2.0 ** -9 * y.abs() + rs * nw.double().abs() * (E + mean_e + z.abs() * (z.abs() * E).mean(1, keepdim=True))


def check_within(out, ref, bound, family, what):
    o = out.detach().cpu().double()
    assert bool(torch.isfinite(o).all()), f"{what}: the output holds a value that is not finite"
    ratio = ((o - ref).abs() / bound.clamp_min(1e-300)).max().item()
    ratios[family] = max(ratio, ratios.get(family, 0.0))
    print(f"bound ratio {family} {what}: {ratio:.4g}")
    assert ratio <= C_BOUND[family], f"{what}: {ratio:.4g} x the derived bound (allowed {C_BOUND[family]})"
    return ratio


def check_stats(st, y, what):
    """``stats_out`` rows = (sum, sum of squares) of the RETURNED bf16 output rows: float64 sums,
    an fp32 accumulation of N terms in any order is within N * 2^-24 * the sum of magnitudes."""
    yd = y.detach().cpu().double()
    N = yd.shape[1]
    s = st.detach().cpu().double()
    for col, (ref, mag) in enumerate(((yd.sum(1), yd.abs().sum(1)), ((yd * yd).sum(1), (yd * yd).sum(1)))):
        tol = N * 2.0 ** -24 * mag
        err = (s[:, col] - ref).abs()
        print(f"stats ratio {what} column {col}: {(err / tol.clamp_min(1e-300)).max().item():.4g}")
        assert bool((err <= tol).all()), f"{what}: row statistic {col} off by {err.max().item():.4g}"


def close_global(a, b, tol=2e-2):
    """The metric of the older GEMM tests: one global max|err| <= tol * max|ref|."""
    err = (a.float() - b.float()).abs().max().item()
    return err <= tol * (b.float().abs().max().item() + 1e-6)


# ---------------------------------------------------------------------------------------------
# A torch model of an honest kernel, and what subtly wrong kernels would return

def honest_model(x, w, bias=None, act=None, res=None, alpha=1.0, tile=(64, 64, 64), kgroups=1, splitk=1,
                 out=None, mutant=None):
    """fp32 accumulation in the kernel's order — K slices, K groups inside a slice taking
    alternate 64-wide K steps, partial sums added group by group, then slice by slice — then
    bf16(act(alpha * acc + bias)) and bf16(that + residual), written into ``out`` ([>= M][>= N],
    default a fresh one). ``mutant`` names one defect (MUTANTS). x / w may be views into the
    poisoned buffers of gemm_cases.padded: the model reads rows and columns through them."""
    (M, K), N = x.shape, w.shape[0]
    bm, bn, _ = tile
    xf, wf = x.float().clone(), w.float()
    if mutant == "last_k_dropped":
        xf[:, K - 1] = 0
    if mutant == "a_row_m_for_last":  # row M - 1 read from row M of the buffer (a clamp off by one)
        base = x._base  # (a contiguous x has no row M to model: left as it is)
        if base is not None and base.shape[0] > M:
            xf[M - 1] = base[M, :K].float()
    steps = K // 64
    per_slice = steps // splitk
    acc = torch.zeros(M, N)
    for s in range(splitk):
        part = torch.zeros(M, N)
        for g in range(kgroups):
            pg = torch.zeros(M, N)
            for t in range(s * per_slice + g, (s + 1) * per_slice if s < splitk - 1 else steps, kgroups):
                if mutant == "k_step_dropped" and s == splitk - 1 and g == kgroups - 1 and t + kgroups >= steps:
                    continue
                pg = pg + xf[:, t * 64:(t + 1) * 64] @ wf[:, t * 64:(t + 1) * 64].T
            part = part + pg
        acc = acc + part
    if K % 64:
        acc = acc + xf[:, steps * 64:] @ wf[:, steps * 64:].T
    b = torch.zeros(N) if bias is None else bias.float().clone()
    if mutant == "bias_shifted_ragged" and bias is not None:
        n0 = (N - 1) // bn * bn  # the ragged last column tile reads bias one column to the right
        b[n0:N - 1] = bias.float()[n0 + 1:N]
    r = torch.zeros(M, N) if res is None else res.float().clone()
    if mutant == "residual_skipped_last_row":
        r[M - 1] = 0
    f32 = lambda v: act64(v.double(), act).float()  # noqa: E731  (relu / none here: exact either way)
    if mutant == "alpha_after_bias":
        pre = f32(alpha * (acc + b))
    elif mutant == "residual_before_act":
        pre = f32(alpha * acc + b + r)
        r = torch.zeros(M, N)
    else:
        pre = f32(alpha * acc + b)
    y = (pre.to(BF).float() + r).to(BF)
    if mutant == "one_ulp":
        i, j = M // 2, N // 2
        y[i, j] = (y[i:i + 1, j:j + 1].view(torch.int16) + 1).view(BF)[0, 0]
    if out is None:
        out = torch.full((M, N), gc.CANARY, dtype=BF)
    if mutant == "tile_unwritten":
        keep = out[bm:M, bn:N].clone()  # the last (ragged) tile keeps what the buffer held
        out[:M, :N] = y
        out[bm:M, bn:N] = keep
    else:
        out[:M, :N] = y
    if mutant == "column_past_n":
        base = out._base
        if base is not None and base.shape[1] > N:
            base[M - 1, N] = y[M - 1, N - 1]
    return out


# mutant -> the check that has to catch it ("exact": torch.equal on the integer probe with the
# full epilogue; "poison": equality with the contiguous run on NaN-padded operands; "canary":
# the bytes around the output view)
MUTANTS = {
    "last_k_dropped": "exact",
    "k_step_dropped": "exact",
    "bias_shifted_ragged": "exact",
    "residual_before_act": "exact",
    "residual_skipped_last_row": "exact",
    "alpha_after_bias": "exact",
    "tile_unwritten": "exact",
    "column_past_n": "canary",
    "a_row_m_for_last": "poison",
    "one_ulp": "exact",
}
