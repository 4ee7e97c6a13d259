"""A float64 CPU restatement of the permutation product of an LRP / DMPLRP layer and its three gradients, written from the
definition -- loops over permutations and slots, no selection matrix, no autograd -- and the hand-made batches and the case
list that ``test_lrp_pool_cpu.py`` and ``test_gpu_lrp_pool_fp64.py`` share.

    out[p]       = sum_s row(slot[p, s]) @ W_s            row(t) = x[t] (t < N), z[t - N] (t < N + E), else 0
    dW_s         = sum_p outer(row(slot[p, s]), dout[p])  W_s    = weight[:, :, s]
    d row(t)     = sum_{(p, s): slot[p, s] = t} W_s @ dout[p]
"""
import numpy as np
import torch as th

TILE = 32           # permutations of a tile of csrc/dmp_lrppool.hip's kernels (and table rows of a tile of its table gradient)
LONG_ROW = 64       # entries of one (table row, slot) from which the table gradient sums the row in shares (kPoolLongRow)


def perm_product_fp64(slot, N, E, L, x, z, w, dout):
    """``(out [P, hid], dx [N, in], dz [E, in], dw [in, hid, L*L])`` in double from the int64 slot vector [P * L*L]."""
    L2 = L * L
    x, z, w, dout = (t.detach().cpu().double() for t in (x, z, w, dout))
    slot = slot.detach().cpu().tolist()
    P = len(slot) // L2
    out = th.zeros(P, w.size(1), dtype=th.float64)
    dx, dz, dw = th.zeros_like(x), th.zeros_like(z), th.zeros_like(w)
    panels = [w[:, :, s].contiguous() for s in range(L2)]
    dpanels = [th.zeros_like(p) for p in panels]
    for p in range(P):
        for s in range(L2):
            t = slot[p * L2 + s]
            if t < 0 or t >= N + E:
                continue
            row = x[t] if t < N else z[t - N]
            out[p] += row @ panels[s]
            dpanels[s] += th.outer(row, dout[p])
            g = panels[s] @ dout[p]
            if t < N:
                dx[t] += g
            else:
                dz[t - N] += g
    for s in range(L2):
        dw[:, :, s] = dpanels[s]
    return out, dx, dz, dw


# ---------------------------------------------------------------------------------------------------- hand-made graphs
def _g(edges, n, rev=None):
    if edges:
        s, t = (np.array(c, np.int64) for c in zip(*edges))
    else:
        s = t = np.zeros(0, np.int64)
    return (s, t, n, np.zeros(len(s), bool) if rev is None else np.array(rev, bool))


def isolated(k=1):
    """k nodes, no edge: one permutation each, only slot 0 filled."""
    return _g([], k)


def path():
    return _g([(0, 1), (1, 2), (2, 3)], 4)


def clique5():
    """Every ordered pair of five nodes: at L 4 every slot of every permutation is filled."""
    return _g([(u, v) for u in range(5) for v in range(5) if u != v], 5)


def star(k, extra=()):
    """Node 0 with k neighbours (k 9 at L 4: 504 permutations of one node) and a few edges among the leaves."""
    return _g([(0, j) for j in range(k, 0, -1)] + list(extra), k + 1)


def duplicates():
    """(2, 1) three times, (0, 1) twice: one neighbour each, the LAST edge of a pair fills the slot."""
    return _g([(2, 1), (0, 1), (2, 1), (1, 2), (0, 1), (2, 0), (2, 1), (0, 2)], 3)


def reversed_flags():
    """Reversed-flag edges are no neighbours and fill no slot; (1, 3) exists both ways, once flagged."""
    return _g([(0, 1), (1, 0), (0, 2), (2, 0), (1, 3), (3, 1), (3, 2), (2, 3), (0, 3)], 4,
              [False, True, False, True, False, True, False, False, True])


def mix():
    return [isolated(), path(), clique5(), duplicates(), reversed_flags()]


def stars24(total):
    """Stars with four neighbours (24 + 4 permutations at L 4) and isolated nodes up to exactly ``total`` permutations."""
    many, rest = divmod(total, 28)
    return [star(4, [(1, 2)])] * many + ([isolated(rest)] if rest else [])


def cases():
    """ids -> dict(graphs, L, fin, hid).  The slots: ``mix`` at every L; the widths: (64, 64) and (128, 128) everywhere,
    the two unequal pairs on ``mix`` at L 4; the counts: 0, 1, one below / above a tile, a few hundred (the star of 9)."""
    out = {}
    for L in (1, 3, 4, 6):
        for w in (64, 128):
            out["mix-L%d-w%d" % (L, w)] = dict(graphs=mix(), L=L, fin=w, hid=w)
    out["mix-L4-in64-hid128"] = dict(graphs=mix(), L=4, fin=64, hid=128)
    out["mix-L4-in128-hid64"] = dict(graphs=mix(), L=4, fin=128, hid=64)
    out["star9-L4-in64-hid128"] = dict(graphs=[star(9, [(1, 2), (2, 1), (3, 1)]), path()], L=4, fin=64, hid=128)
    out["star9-L4-in128-hid64"] = dict(graphs=[star(9, [(1, 2), (2, 1), (3, 1)]), path()], L=4, fin=128, hid=64)
    for k in (LONG_ROW - 1, LONG_ROW, LONG_ROW + 1):          # at L 2 a hub of k neighbours fills slot 0 of exactly k permutations
        out["star%d-L2-w64" % k] = dict(graphs=[path(), star(k, [(1, 2)])], L=2, fin=64, hid=64)
    for w in (64, 128):
        out["star9-L4-w%d" % w] = dict(graphs=[star(9, [(1, 2), (2, 1), (3, 1)]), path()], L=4, fin=w, hid=w)
        out["P0-w%d" % w] = dict(graphs=[_g([], 0)], L=4, fin=w, hid=w)
        out["P1-w%d" % w] = dict(graphs=[isolated()], L=4, fin=w, hid=w)
        out["P%d-w%d" % (TILE - 1, w)] = dict(graphs=stars24(TILE - 1), L=4, fin=w, hid=w)
        out["P%d-w%d" % (TILE + 1, w)] = dict(graphs=stars24(TILE + 1), L=4, fin=w, hid=w)
    return out


def stable_seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


def inputs(name, N, E, P, L, fin, hid, small=False):
    """CPU fp32 ``(x [N, in], z [E, in], w [in, hid, L*L], bias [hid], dout [P, hid], coef [N, hid])``.  Rows N(0, 1), weights
    N(0, 1 / (in L)): a product entry is a sum of in * (L .. L*L) terms and comes out at 1 .. sqrt(L).  ``small``: weights and
    upstream factors a tenth / a fiftieth of that, for comparisons with an ABSOLUTE floor (see test_gpu_lrp_pool_fp64.py)."""
    g = th.Generator().manual_seed(stable_seed(name))
    x, z = th.randn(N, fin, generator=g), th.randn(E, fin, generator=g)
    w = th.randn(fin, hid, L * L, generator=g) / float(np.sqrt(fin * L)) * (0.1 if small else 1.0)
    bias = th.randn(hid, generator=g) * 0.1
    coef = th.randn(N, hid, generator=g) * (0.02 if small else 1.0)
    dout = th.randn(P, hid, generator=g)          # drawn last: an index at a capacity changes nothing else
    return x, z, w, bias, dout, coef
