"""The oracle of the device labeller's tests (test_subiso_device_cpu.py, test_gpu_subiso_device.py): a plain-Python
backtracking restatement of the search that returns the matches AND the number of trials, the two weight definitions as
loops over match rows, the case list both files share, and a plain-Python walk of a batch image (what the kernel is handed)
so that the image builder can be checked without a GPU.

The search, as csrc/dmp_subiso.cpp states it: pattern nodes are placed in id order; a candidate for node k is a graph node of
k's label that no earlier node uses; it is accepted when every pattern edge whose later endpoint is k has a graph edge
between the images with its label; a TRIAL is one candidate whose edge checks are evaluated.  pn > gn is 0 matches without
a search (0 trials), pn = 0 is one empty match."""
import numpy as np


def A(*xs):
    return np.array(xs, dtype=np.int64)


def search(pair):
    """-> (rows [count, pn] int64 in lexicographic order, trials, the largest number of trials under ONE image of node 0)."""
    ps, pd, pvl, pel, gs, gd, gvl, gel = (np.asarray(a, np.int64).tolist() for a in pair)
    pn, gn = len(pvl), len(gvl)
    if pn > gn:
        return np.zeros((0, pn), np.int64), 0, 0
    have = set(zip(gs, gd, gel))
    touching = [[(u, v, l) for u, v, l in zip(ps, pd, pel) if max(u, v) == k] for k in range(pn)]
    rows, f, used = [], [0] * pn, [False] * gn
    trials = [0]

    def place(k):
        if k == pn:
            rows.append(tuple(f))
            return
        for x in range(gn):
            if gvl[x] != pvl[k] or used[x]:
                continue
            trials[0] += 1
            f[k] = x
            if all((f[u], f[v], l) in have for u, v, l in touching[k]):
                used[x] = True
                place(k + 1)
                used[x] = False

    per_root = 0
    if pn == 0:
        place(0)
    else:
        for x in range(gn):                      # the images of node 0 one by one: the kernel's work items
            if gvl[x] != pvl[0]:
                continue
            before = trials[0]
            trials[0] += 1
            f[0] = x
            if all((f[u], f[v], l) in have for u, v, l in touching[0]):
                used[x] = True
                place(1)
                used[x] = False
            per_root = max(per_root, trials[0] - before)
    return np.array(rows, np.int64).reshape(len(rows), pn), trials[0], per_root


def node_weights(pair, rows):
    """Per graph node the matches whose image contains it (the reference's loop over rows, then over a row's entries)."""
    w = np.zeros(len(pair[6]), np.int64)
    for row in rows:
        for x in row:
            w[x] += 1
    return w


def edge_weights(pair, rows):
    """Per graph edge k the sum over matches f and pattern edges (u, v, l) of [src_k = f(u), dst_k = f(v), label_k = l]: a
    duplicated pattern edge counts twice and every parallel graph edge with that label is counted."""
    ps, pd, _, pel, gs, gd, _, gel = (np.asarray(a, np.int64).tolist() for a in pair)
    w = np.zeros(len(gs), np.int64)
    for row in rows:
        for u, v, l in zip(ps, pd, pel):
            for k in range(len(gs)):
                if gs[k] == row[u] and gd[k] == row[v] and gel[k] == l:
                    w[k] += 1
    return w


def expected(pair):
    rows, trials, per_root = search(pair)
    return {"rows": rows, "count": len(rows), "trials": trials, "per_root": per_root, "node": node_weights(pair, rows),
            "edge": edge_weights(pair, rows)}


# ------------------------------------------------------------------------------------------------------------ the cases
def random_pair(rng, pn, pm, gn, gm, nvl, nel, copies=0, path=False):
    """A pattern (``path``: node k hangs on node k - 1, so that the id order is a connected order) and a graph of random
    edges (a multigraph: self loops and repeats may occur) with ``copies`` planted images of the pattern."""
    if path and pn > 1:
        a = np.arange(1, pn)
        flip = rng.random(pn - 1) < 0.5
        ps, pd = np.where(flip, a, a - 1), np.where(flip, a - 1, a)
        extra = pm - (pn - 1)
        ps = np.concatenate([ps, rng.integers(0, pn, extra)])
        pd = np.concatenate([pd, rng.integers(0, pn, extra)])
    else:
        ps, pd = (rng.integers(0, pn, pm), rng.integers(0, pn, pm)) if pn else (A(), A())
    pvl, pel = rng.integers(0, nvl, pn), rng.integers(0, nel, len(ps))
    gvl = rng.integers(0, nvl, gn)
    gs, gd, gel = (rng.integers(0, gn, gm), rng.integers(0, gn, gm), rng.integers(0, nel, gm)) if gn else (A(), A(), A())
    for _ in range(copies):
        where = rng.choice(gn, size=pn, replace=False)
        gvl[where] = pvl
        gs, gd, gel = np.concatenate([gs, where[ps]]), np.concatenate([gd, where[pd]]), np.concatenate([gel, pel])
    return tuple(np.asarray(a, np.int64) for a in (ps, pd, pvl, pel, gs, gd, gvl, gel))


def complete_digraph_pair():
    """A single-label complete digraph on 9 nodes and a directed 4-path: 9 * 8 * 7 * 6 = 3,024 matches, 1 + 8 + 56 + 336 = 401
    trials under every image of node 0."""
    gs, gd = zip(*[(u, v) for u in range(9) for v in range(9) if u != v])
    z = lambda n: np.zeros(n, np.int64)
    return (A(0, 1, 2), A(1, 2, 3), z(4), z(3), A(*gs), A(*gd), z(9), z(72))


def cases():
    """name -> pair: the smallest shapes at which the kernel can go wrong."""
    rng = np.random.default_rng(7)
    z = lambda n: np.zeros(n, np.int64)
    c = {}
    c["pn0"] = (A(), A(), A(), A(), A(0, 1), A(1, 2), A(0, 1, 0), A(3, 3))
    c["pn0_empty_graph"] = (A(), A(), A(), A(), A(), A(), A(), A())
    c["pn1_gn1"] = (A(), A(), A(2), A(), A(), A(), A(2), A())
    c["pn1_selfloop_gn1"] = (A(0), A(0), A(2), A(5), A(0), A(0), A(2), A(5))
    c["pn2_gn1_pn_above_gn"] = (A(0), A(1), A(0, 0), A(1), A(0), A(0), A(0), A(1))
    c["pn2_gn2_pn_equals_gn"] = (A(0), A(1), A(0, 0), A(1), A(0, 1), A(1, 0), A(0, 0), A(1, 1))
    c["pn2_empty_graph"] = (A(0), A(1), A(0, 0), A(1), A(), A(), A(), A())
    c["pn4_gn4_no_edges"] = (A(), A(), z(4), A(), A(0, 1), A(1, 2), z(4), A(0, 0))               # 4! injective maps
    c["pn3_gn5_no_edges_labels"] = (A(), A(), A(0, 1, 0), A(), A(0), A(1), A(0, 1, 0, 0, 1), A(0))  # 3 * 2 * 2 = 12
    c["pattern_selfloop"] = (A(0, 0, 1), A(0, 1, 1), A(0, 0), A(1, 2, 1), A(0, 0, 1, 2, 2, 2, 3), A(0, 1, 1, 2, 3, 3, 3), z(4),
                             A(1, 2, 1, 1, 2, 2, 1))
    c["pattern_duplicate_edge"] = (A(0, 0), A(1, 1), z(2), A(4, 4), A(0, 0, 1, 2), A(1, 1, 2, 0), z(3), A(4, 4, 4, 5))
    c["pattern_two_labels_one_pair"] = (A(0, 0), A(1, 1), z(2), A(4, 5), A(0, 0, 1, 1, 2), A(1, 1, 2, 2, 0), z(3), A(4, 5, 4, 4, 5))
    c["graph_parallel_equal_label"] = (A(0), A(1), z(2), A(7), A(0, 0, 0, 1), A(1, 1, 1, 2), z(3), A(7, 7, 7, 7))
    c["graph_parallel_other_labels"] = (A(0), A(1), z(2), A(7), A(0, 0, 0, 1), A(1, 1, 1, 2), z(3), A(7, 8, 9, 8))
    c["node_label_absent"] = (A(0), A(1), A(0, 9), A(1), A(0, 1), A(1, 2), A(0, 0, 0), A(1, 1))
    c["edge_label_absent"] = (A(0), A(1), A(0, 0), A(9), A(0, 1), A(1, 2), A(0, 0, 0), A(1, 1))
    c["big_labels"] = (A(0), A(1), A(-5, 2 ** 40), A(-2 ** 50), A(0, 1, 1), A(1, 0, 2), A(-5, 2 ** 40, -5), A(-2 ** 50, -2 ** 50, 3))
    c["complete_digraph_4path"] = complete_digraph_pair()
    c["roots_gn2"] = random_pair(rng, 2, 1, 2, 6, 1, 2)
    for gn in (63, 64, 65, 130):                        # one label: gn images of node 0, around the wave of 64
        c["roots_gn%d" % gn] = random_pair(rng, 3, 3, gn, 4 * gn, 1, 2, copies=min(2, gn // 3), path=True)
    c["roots_gn512"] = random_pair(rng, 2, 1, 512, 2048, 1, 2)
    c["pn3"] = random_pair(rng, 3, 4, 24, 96, 2, 2, copies=2, path=True)
    c["pn4"] = random_pair(rng, 4, 6, 33, 132, 2, 2, copies=3, path=True)
    c["pn8"] = random_pair(rng, 8, 10, 65, 260, 3, 2, copies=3, path=True)
    c["pn8_gn8_pn_equals_gn"] = random_pair(rng, 8, 8, 8, 16, 2, 2, copies=1, path=True)
    c["pn16_gn512"] = random_pair(rng, 16, 20, 512, 1900, 24, 3, copies=3, path=True)
    c["pn16_pm64"] = random_pair(rng, 16, 64, 40, 160, 2, 1, copies=2, path=True)
    return c


def batch(size, seed=0):
    """``size`` pairs: pairs of very different sizes next to each other, an empty graph in the middle."""
    rng = np.random.default_rng(100 + seed)
    big = cases()
    heavy = [big[k] for k in ("roots_gn130", "pn8", "roots_gn65", "pn16_pm64")]
    out = []
    for i in range(size):
        if i == size // 2:
            out.append((A(0), A(1), A(0, 0), A(1), A(), A(), A(), A()))
        elif i % 16 == 1:
            out.append(heavy[(i // 16) % len(heavy)])
        else:
            pn = int(rng.integers(0, 5))
            gn = int(rng.integers(1, 13))
            out.append(random_pair(rng, pn, int(rng.integers(0, 5)) if pn else 0, gn, int(rng.integers(0, 3 * gn)), 2, 2,
                                   copies=1 if gn >= pn and pn else 0))
    return out


def mixed_pn17_pair():
    """17 pattern nodes (one more than the kernel admits) in a graph small enough for the host search."""
    return random_pair(np.random.default_rng(5), 17, 16, 20, 60, 6, 2, copies=1, path=True)


def raw_pairs(dataset):
    """The 8-tuples a ``PairDataset``'s samples were labelled from: the forward halves of its edge arrays."""
    half = lambda g, k: np.asarray(g[k][:len(g[k]) // 2], np.int64)
    out = []
    for x in dataset.samples:
        p, g = x["pattern"], x["graph"]
        out.append((half(p, "src"), half(p, "dst"), np.asarray(p["vlabel"], np.int64), half(p, "elabel"),
                    half(g, "src"), half(g, "dst"), np.asarray(g["vlabel"], np.int64), half(g, "elabel")))
    return out


# ------------------------------------------------------------- a plain-Python walk of a batch image (subiso.build_image)
def walk_image(im, budget, weights=True):
    """What ``dmp_subiso_label_dev`` computes from an image, item by item as the kernel does it (a chunk's lanes one after the
    other; LDS columns as Python lists): counts, trials, complete, node weights [total_gn], edge weights [total_gm]."""
    n = im["num_pairs"]
    d = im["desc"].astype(np.int64)
    ok = (d[:, 0] <= 16) & (d[:, 1] <= 64) & (d[:, 2] <= im["max_gn"]) & (d[:, 3] <= im["max_um"]) if n else np.zeros(0, bool)
    counts = np.where(ok & (d[:, 0] == 0), 1, 0).astype(np.int64) if n else np.zeros(0, np.int64)
    trials, complete = np.zeros(n, np.int64), ok.copy()
    nw, uw = np.zeros(im["total_gn"], np.int64), np.zeros(im["total_um"], np.int64)
    for c in range(im["num_chunks"]):
        i, root0 = int(im["chunk_pair"][c]), int(im["chunk_root"][c])
        pn, pm, gn, um, pno, peo, gno, uo = (int(x) for x in d[i])
        ent = im["g_ent"][uo:uo + um].tolist()
        rowptr = (im["g_rowptr"][gno:gno + gn + 1].astype(np.int64) - uo).tolist()
        cand = im["g_cand"][gno:gno + gn].tolist()
        pe, pel = im["p_ends"][peo:peo + pm].tolist(), im["p_elab"][peo:peo + pm].tolist()
        tend, cbeg, cend = (im[k][pno:pno + pn].tolist() for k in ("p_tend", "p_cbeg", "p_cend"))
        assert all(0 <= r <= um for r in rowptr) and all(0 <= v < gn for v in cand) and all(0 <= e >> 32 < gn for e in ent)

        def find(mu, mv, lab):
            lo, end = rowptr[mu], rowptr[mu + 1]
            hi, key = end, (mv << 32) | lab
            while lo < hi:
                mid = (lo + hi) >> 1
                if ent[mid] < key:
                    lo = mid + 1
                else:
                    hi = mid
            return lo if lo < end and ent[lo] == key else -1

        for lane in range(64):
            root = cbeg[0] + root0 + lane
            if root >= cend[0]:
                break
            f, pos, used, k, tr = [0] * 16, [0] * 16, set(), 0, 0
            pos[0] = root
            while True:
                cur, end = pos[k], (root + 1 if k == 0 else cend[k])
                if cur >= end:
                    if k == 0:
                        break
                    k -= 1
                    used.discard(f[k])
                    continue
                pos[k] = cur + 1
                v = cand[cur]
                if v in used:
                    continue
                if tr >= budget:
                    complete[i] = False
                    break
                tr += 1
                f[k] = v
                if any(find(f[pe[e] & 255], f[pe[e] >> 8], pel[e]) < 0 for e in range(tend[k - 1] if k else 0, tend[k])):
                    continue
                if k + 1 < pn:
                    used.add(v)
                    k += 1
                    pos[k] = cbeg[k]
                    continue
                counts[i] += 1
                if weights:
                    for j in range(pn):
                        nw[gno + f[j]] += 1
                    for e in range(pm):
                        uw[uo + find(f[pe[e] & 255], f[pe[e] >> 8], pel[e])] += 1
            trials[i] += tr
    return {"counts": counts, "trials": trials, "complete": complete, "node_weights": nw,
            "edge_weights": uw[im["g_inv"]] if im["total_gm"] else np.zeros(0, np.int64)}
