"""Independent reference of the MoE routing, pack and combine operations.

Plain Python loops over exact values (float64 where arithmetic is needed); nothing here calls
the package under test, ``torch.topk`` or ``torch.sort``. torch is used only as the container
the tests hand in and compare against. Every function returns new tensors and leaves its
arguments unchanged.

The rules these functions state:

* routing: per token the experts are ordered by (logit descending, expert index ascending) on
  the exact bf16 values; the first k are selected, in that order; the gates are the softmax of
  the selected logits.
* align: a stable counting sort of assignment i = m * k + j by expert.
* pack / unpack: ``ops.moe_pack`` / ``kernels.h MoePackArgs`` — the listed experts' routed rows
  in the listed order, each expert's rows in sorted order; nothing past ``min(total, cap)`` is
  moved, nothing is cleared, and an overflow only ever sets its ``ovf`` word to 1.
"""
import math

import torch


def route_ref(logits_bf16, k):
    """idx int32 [M][k], gate float64 [M][k] of bf16 logits [M][E]."""
    assert logits_bf16.dtype == torch.bfloat16 and logits_bf16.dim() == 2
    rows = logits_bf16.cpu().to(torch.float64).tolist()  # bf16 -> float64 is exact
    idx, gate = [], []
    for v in rows:
        order = sorted(range(len(v)), key=lambda e: (-v[e], e))[:k]
        p = [math.exp(v[e] - v[order[0]]) for e in order]
        s = sum(p)
        idx.append(order)
        gate.append([t / s for t in p])
    return (torch.tensor(idx, dtype=torch.int32).reshape(len(rows), k),
            torch.tensor(gate, dtype=torch.float64).reshape(len(rows), k))


def align_ref(idx, E):
    """(src_rows [M*k], slot_of [M*k], offsets [E+1]), all int32."""
    k = idx.shape[1]
    flat = idx.cpu().reshape(-1).tolist()
    counts = [0] * E
    for e in flat:
        counts[e] += 1
    offsets = [0] * (E + 1)
    for e in range(E):
        offsets[e + 1] = offsets[e] + counts[e]
    nxt = offsets[:E]
    src_rows, slot_of = [0] * len(flat), [0] * len(flat)
    for i, e in enumerate(flat):  # ascending i: stable
        slot_of[i] = nxt[e]
        src_rows[nxt[e]] = i // k
        nxt[e] += 1
    i32 = torch.int32
    return torch.tensor(src_rows, dtype=i32), torch.tensor(slot_of, dtype=i32), torch.tensor(offsets, dtype=i32)


def pack_rows(offsets, experts, cap):
    """The sorted positions j that one destination moves, in buffer-row order: [(c, j)]."""
    off = [int(v) for v in offsets.tolist()]
    js = [j for e in experts for j in range(off[e], off[e + 1])]
    return list(enumerate(js[:max(0, min(len(js), int(cap)))]))


def ovf_ref(offsets, dests, ovf):
    off = [int(v) for v in offsets.tolist()]
    out = ovf.cpu().clone()
    for _buf, cap, experts, flag, ecaps, eflags in dests:
        total = 0
        for e, ecap, ef in zip(experts, ecaps, eflags):
            n = off[e + 1] - off[e]
            total += n
            if ef >= 0 and n > ecap:
                out[ef] = 1
        if flag >= 0 and total > cap:
            out[flag] = 1
    return out


def pack_ref(x, src_rows, offsets, dests, ovf):
    """dests: [(buf, cap, experts, flag, ecaps, eflags)] -> ([buf'], ovf')."""
    xs, src = x.cpu(), [int(v) for v in src_rows.tolist()]
    H = xs.shape[1]
    bufs = []
    for buf, cap, experts, _flag, _ecaps, _eflags in dests:
        b = buf.cpu().clone()
        flat = b.view(-1)
        for c, j in pack_rows(offsets, experts, cap):
            flat[c * H:(c + 1) * H] = xs[src[j]]
        bufs.append(b)
    return bufs, ovf_ref(offsets, dests, ovf)


def unpack_ref(x, src_rows, offsets, dests, ovf):
    """x holds the expert-sorted rows: -> (x', ovf')."""
    out = x.cpu().clone()
    H = out.shape[1]
    for buf, cap, experts, _flag, _ecaps, _eflags in dests:
        flat = buf.cpu().view(-1)
        for c, j in pack_rows(offsets, experts, cap):
            out[j] = flat[c * H:(c + 1) * H]
    return out, ovf_ref(offsets, dests, ovf)


def combine_ref(expert_out, slot_of, w, slot_range=None):
    """(y, mag) float64 [M][H]: y[m] = sum_j w[m][j] * expert_out[slot_of[m*k+j]] over the slots
    inside ``slot_range`` ([r0, r1), all when None); mag = the same sum of absolute products."""
    M, k = w.shape
    eo = expert_out.cpu().to(torch.float64)
    g = w.cpu().to(torch.float64).tolist()
    sl = slot_of.cpu().reshape(M, k).tolist()
    r0, r1 = (0, 1 << 62) if slot_range is None else (int(slot_range[0]), int(slot_range[1]))
    y = torch.zeros(M, eo.shape[1], dtype=torch.float64)
    mag = torch.zeros_like(y)
    for m in range(M):
        for j in range(k):
            if r0 <= sl[m][j] < r1:
                y[m] += g[m][j] * eo[sl[m][j]]
                mag[m] += abs(g[m][j]) * eo[sl[m][j]].abs()
    return y, mag


def permute_ref(x, src_rows):
    xs = x.cpu()
    out = torch.empty(src_rows.numel(), xs.shape[1], dtype=xs.dtype)
    for r, s in enumerate(src_rows.tolist()):
        out[r] = xs[int(s)]
    return out


def xbatch_ref(offs, reqs, experts, bases):
    """Group g = (request reqs[g], expert experts[g]) -> (offsets int32 [G+1], a_rows int32
    [offsets[G]]): the group's rows are bases[q] + [offs[q][e], offs[q][e+1])."""
    offsets, a_rows = [0], []
    for q, e in zip(reqs, experts):
        off = [int(v) for v in offs[q].tolist()]
        a_rows.extend(bases[q] + r for r in range(off[e], off[e + 1]))
        offsets.append(len(a_rows))
    return torch.tensor(offsets, dtype=torch.int32), torch.tensor(a_rows, dtype=torch.int32)
