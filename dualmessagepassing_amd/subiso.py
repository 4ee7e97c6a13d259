"""Labels of (pattern, graph) pairs on the device: exact subisomorphism counts and the matching weights.

``label_pairs`` is the device twin of ``harness.count_subisomorphisms_batch`` (csrc/dmp_subiso.cpp, a depth-first search
over a pool of host threads): the same matches in the same node order, searched by ``dmp_subiso_label_dev``
(csrc/dmp_subiso_dev.hip) with a work item per (pair, image of pattern node 0).  Besides the counts it can return the
node and edge weights of the matching loss -- ``compute_nodeseq_subisoweights`` / ``compute_edgeseq_subisoweights`` as sums
over the matches, accumulated during the search, so that a pair whose enumeration would not fit in memory still gets them.

The road of a batch: range checks (numpy, nothing uploaded before they pass) -> the batch's image (label codes, the pattern
edges by their later endpoint, the graphs' distinct edges as a CSR, the candidate lists; vectorised numpy) -> ONE upload ->
the launches -> ONE read.  Pairs the kernel does not finish (not admitted, or an item ran out of its trial budget) are
finished on the host, so the labels are exact either way; ``fallback`` says how many took that road.

Admitted by the kernel: pattern nodes <= 16, pattern edges <= 64, graph nodes <= 512, DISTINCT (src, dst, label) graph
edges <= 2048 (the reference's "large" setting is 512 nodes / 2,048 edges), fewer than 2**31 nodes / edges in the batch.
"""
import ctypes

import numpy as np

from . import _abi, _lib
from .harness import _i64, count_subisomorphisms_batch, enumerate_subisomorphisms

MAX_PN, MAX_PM, MAX_GN, MAX_GM = _abi.DMP_SUBISO_MAX_PN, _abi.DMP_SUBISO_MAX_PM, _abi.DMP_SUBISO_MAX_GN, _abi.DMP_SUBISO_MAX_GM
MAX_BUDGET = _abi.DMP_SUBISO_MAX_BUDGET
ITEMS_PER_LAUNCH = 2048 * 64         # one search launch takes at most 2048 chunks of 64 items (dmp_subiso_dev.hip)
# The trial budget of one work item.  Rule: a launch in which EVERY item spends its whole budget stays under one second,
#   DEFAULT_BUDGET = the largest power of two with  DEFAULT_BUDGET * ITEMS_PER_LAUNCH <= trials_per_second * 1 s.
# Measured on an MI355X by scripts/kbench_subiso.py (profiles/subiso_device_kbench.json): 5.4e10 trials per second on a
# full launch of 131072 items that all run out of budget, linear from budget 4096 to 65536 -> 2**18 = 262144, at which such
# a launch takes 0.63 s.
DEFAULT_BUDGET = 262144
_NAMES = ("p_src", "p_dst", "p_vlabel", "p_elabel", "g_src", "g_dst", "g_vlabel", "g_elabel")


def _flatten(pairs):
    """The pairs back to back (the layout of ``dmp_subiso_count_batch``) after the range checks: ``ValueError`` naming the
    pair for a tuple that is not 8 one-dimensional arrays, ragged edge arrays or an edge endpoint outside its graph."""
    n = len(pairs)
    cols = [[] for _ in range(8)]
    lens = np.zeros((n, 8), np.int64)
    for i, p in enumerate(pairs):
        if len(p) != 8:
            raise ValueError("label_pairs: pair %d is a tuple of %d arrays, not of 8" % (i, len(p)))
        for k in range(8):
            a = _i64(p[k])
            if a.ndim != 1:
                raise ValueError("label_pairs: pair %d: %s is not one-dimensional" % (i, _NAMES[k]))
            cols[k].append(a)
            lens[i, k] = a.size
    ragged = (lens[:, 0] != lens[:, 1]) | (lens[:, 0] != lens[:, 3]) | (lens[:, 4] != lens[:, 5]) | (lens[:, 4] != lens[:, 7])
    if ragged.any():
        raise ValueError("label_pairs: pair %d: src, dst and elabel of a graph differ in length" % int(np.flatnonzero(ragged)[0]))
    flat = [np.concatenate(c) if n else np.zeros(0, np.int64) for c in cols]
    pn, pm, gn, gm = lens[:, 2], lens[:, 0], lens[:, 6], lens[:, 4]
    ids = np.arange(n)
    for what, a, b, size, m in (("pattern", flat[0], flat[1], pn, pm), ("graph", flat[4], flat[5], gn, gm)):
        of = np.repeat(ids, m)
        bad = (a < 0) | (a >= size[of]) | (b < 0) | (b >= size[of])
        if bad.any():
            raise ValueError("label_pairs: pair %d: an edge endpoint of the %s lies outside its nodes" % (int(of[np.flatnonzero(bad)[0]]), what))
    return flat, pn, pm, gn, gm


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def build_image(flat, pn, pm, gn, gm):
    """The batch's image for ``dmp_subiso_label_dev`` as numpy arrays (the field names of ``dmp_subiso_image``; the header
    describes each), plus ``admitted`` [n] bool.  Vectorised: no Python loop over pairs, nodes or edges."""
    ps, pd, pvl, pel, gs, gd, gvl, gel = flat
    n = len(pn)
    ids = np.arange(n)
    pno, peo, gno, geo = _offsets(pn), _offsets(pm), _offsets(gn), _offsets(gm)
    tpn, tpm, tgn, tgm = int(pno[-1]), int(peo[-1]), int(gno[-1]), int(geo[-1])
    # label codes: one space per kind, pattern and graph together
    vcode = np.unique(np.concatenate([pvl, gvl]), return_inverse=True)[1].reshape(-1)
    ecode = np.unique(np.concatenate([pel, gel]), return_inverse=True)[1].reshape(-1)
    pvc, gvc, pec, gec = vcode[:tpn], vcode[tpn:], ecode[:tpm], ecode[tpm:]
    nl = int(vcode.max()) + 1 if vcode.size else 1
    # candidate lists: a graph's nodes by (label, id); a pattern node's range in them
    gpid, ppid = np.repeat(ids, gn), np.repeat(ids, pn)
    gloc = np.arange(tgn) - gno[gpid]
    order = np.lexsort((gloc, gvc, gpid))
    gkey = (gpid * nl + gvc)[order]
    pkey = ppid * nl + pvc
    cbeg = np.searchsorted(gkey, pkey, "left") - gno[ppid]
    cend = np.searchsorted(gkey, pkey, "right") - gno[ppid]
    # pattern edges by their later endpoint, ties in edge order (lexsort is stable)
    epid = np.repeat(ids, pm)
    later = np.maximum(ps, pd)
    eorder = np.lexsort((later, epid))
    p_ends = ((ps & 255) | ((pd & 255) << 8))[eorder]
    tend = np.searchsorted((pno[epid] + later)[eorder], np.arange(tpn), "right") - peo[ppid]
    # the graphs' distinct (src, dst, label) edges, sorted: a CSR by source
    gepid = np.repeat(ids, gm)
    o = np.lexsort((gec, gd, gs, gepid))
    spid, ssrc, sdst, slab = gepid[o], gs[o], gd[o], gec[o]
    new = np.ones(tgm, bool)
    if tgm > 1:
        new[1:] = (spid[1:] != spid[:-1]) | (ssrc[1:] != ssrc[:-1]) | (sdst[1:] != sdst[:-1]) | (slab[1:] != slab[:-1])
    inv = np.empty(tgm, np.int64)
    inv[o] = np.cumsum(new) - 1
    ent = ((sdst & 0x7FFFFFFF) << 32 | slab)[new]
    um = np.bincount(spid[new], minlength=n).astype(np.int64) if n else np.zeros(0, np.int64)
    uo = _offsets(um)
    rowptr = np.searchsorted((gno[spid] + ssrc)[new], np.arange(tgn + 1), "left")
    admitted = (pn <= MAX_PN) & (pm <= MAX_PM) & (gn <= MAX_GN) & (um <= MAX_GM)
    # the work list: chunks of 64 candidates of pattern node 0, for every admitted pair with a search to run
    searched = admitted & (pn >= 1) & (pn <= gn)
    first = np.minimum(pno[:-1], max(tpn - 1, 0))
    roots = np.where(searched, (cend - cbeg)[first] if tpn else 0, 0)
    nch = (roots + 63) // 64
    cpair = np.repeat(ids, nch)
    croot = (np.arange(int(nch.sum())) - _offsets(nch)[:-1][cpair]) * 64
    i32 = lambda a: np.ascontiguousarray(np.minimum(a, 2 ** 31 - 1), dtype=np.int32)
    desc = np.stack([pn, pm, gn, um, pno[:-1], peo[:-1], gno[:-1], uo[:-1]], axis=1) if n else np.zeros((0, 8), np.int64)
    return {"desc": i32(desc), "p_cbeg": i32(cbeg), "p_cend": i32(cend), "p_tend": i32(tend), "p_ends": i32(p_ends), "p_elab": i32(pec[eorder]),
            "g_rowptr": i32(rowptr), "g_ent": np.ascontiguousarray(ent, dtype=np.int64), "g_cand": i32(gloc[order]), "g_inv": i32(inv),
            "chunk_pair": i32(cpair), "chunk_root": i32(croot),
            "num_pairs": n, "total_pn": tpn, "total_pm": tpm, "total_gn": tgn, "total_gm": tgm, "total_um": int(uo[-1]),
            "num_chunks": int(cpair.size), "max_gn": int(gn[admitted].max()) if admitted.any() else 0,
            "max_um": int(um[admitted].max()) if admitted.any() else 0, "admitted": admitted}


_ARRAYS = ("desc", "p_cbeg", "p_cend", "p_tend", "p_ends", "p_elab", "g_rowptr", "g_ent", "g_cand", "g_inv", "chunk_pair", "chunk_root")
_SCALARS = ("num_pairs", "total_pn", "total_pm", "total_gn", "total_gm", "total_um", "num_chunks", "max_gn", "max_um")


def _pack(arrays):
    """The arrays in one byte buffer, each at a multiple of 16 bytes: one upload.  -> (buffer, offsets)."""
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += (a.nbytes + 15) // 16 * 16
    buf = np.zeros(max(total, 16), np.uint8)
    for a, o in zip(arrays, offs):
        buf[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    return buf, offs


def launch(image, device, weights=(), budget=None, fill=0):
    """Upload an image (``build_image``), run ``dmp_subiso_label_dev`` and read the result back: one upload, one read, no host
    synchronisation in between.  -> ``counts``, ``trials`` (int64 [n]), ``complete`` (bool [n]), ``node_weights`` [total_gn] /
    ``edge_weights`` [total_gm] (flat, or None), as the kernels left them.  ``fill``: what the output buffer holds before the
    launches (the kernels write every element; tests pass a sentinel)."""
    import torch
    device = torch.device(device)
    budget = DEFAULT_BUDGET if budget is None else int(budget)
    if not 1 <= budget <= MAX_BUDGET:
        raise ValueError("label_pairs: budget %d outside 1 .. %d" % (budget, MAX_BUDGET))
    n, tgn, tgm, tum = image["num_pairs"], image["total_gn"], image["total_gm"], image["total_um"]
    want_n, want_e = "node" in weights, "edge" in weights
    buf, offs = _pack([image[k] for k in _ARRAYS])
    # the outputs in one int64 buffer: counts | trials | node weights | edge weights | complete (bytes); the workspace apart
    o_nw = 2 * n
    o_ew = o_nw + (tgn if want_n else 0)
    o_cp = o_ew + (tgm if want_e else 0)
    words = o_cp + (n + 7) // 8
    with torch.cuda.device(device):
        lib = _lib.load()
        dbuf = torch.from_numpy(buf).to(device)
        out = torch.full((max(words, 1),), int(fill), dtype=torch.int64, device=device)
        work = torch.empty(max(tum, 1), dtype=torch.int64, device=device) if want_e else None
        _lib.require_gpu(dbuf, out, work)
        img = _abi.dmp_subiso_image()
        for k, o in zip(_ARRAYS, offs):
            setattr(img, k, dbuf.data_ptr() + o)
        for k in _SCALARS:
            setattr(img, k, image[k])
        base = out.data_ptr()
        _lib.check(lib.dmp_subiso_label_dev(ctypes.byref(img), budget, base, base + 8 * n, base + 8 * o_cp,
                                            base + 8 * o_nw if want_n else None, base + 8 * o_ew if want_e else None,
                                            _lib.ptr(work), _lib.stream_ptr()), "dmp_subiso_label_dev")
        host = out.cpu().numpy()                      # the one read (synchronises)
    return {"counts": host[:n].copy(), "trials": host[n:2 * n].copy(), "complete": host[o_cp:].view(np.uint8)[:n].astype(bool),
            "node_weights": host[o_nw:o_nw + tgn].copy() if want_n else None,
            "edge_weights": host[o_ew:o_ew + tgm].copy() if want_e else None}


def weights_from_rows(pair, rows):
    """``(node_weights [gn], edge_weights [gm])`` of one pair from its enumerated rows [count, pn]: per graph node the rows that
    contain it; per graph edge k the sum over rows f and pattern edges (u, v, l) of [src_k = f(u), dst_k = f(v), label_k = l]."""
    ps, pd, _, pel, gs, gd, gvl, gel = (_i64(a) for a in pair)
    gn = len(gvl)
    rows = np.asarray(rows, np.int64).reshape(-1, max(len(pair[2]), 1))[:, :len(pair[2])]
    node_w = np.bincount(rows.reshape(-1), minlength=gn).astype(np.int64) if gn else np.zeros(0, np.int64)
    code = np.unique(np.concatenate([pel, gel]), return_inverse=True)[1].reshape(-1)
    nc = int(code.max()) + 1 if code.size else 1
    keys, inv = np.unique((gs * gn + gd) * nc + code[len(pel):], return_inverse=True)
    uw = np.zeros(len(keys), np.int64)
    if len(rows):
        for u, v, c in zip(ps.tolist(), pd.tolist(), code[:len(pel)].tolist()):
            uw += np.bincount(np.searchsorted(keys, (rows[:, u] * gn + rows[:, v]) * nc + c), minlength=len(keys))
    return node_w, uw[inv.reshape(-1)] if len(gs) else np.zeros(0, np.int64)


def label_pairs(pairs, device, weights=(), budget=None, threads=0, fill=0):
    """Exact labels of ``pairs`` (the list of 8-tuples ``count_subisomorphisms_batch`` takes: p_src, p_dst, p_vlabel, p_elabel,
    g_src, g_dst, g_vlabel, g_elabel).  ``weights``: a subset of ("node", "edge").  Returns a dict:

    ``counts`` int64 [n];  ``node_weights`` / ``edge_weights``: per pair an int64 array [gn] / [gm], or None when not asked
    for;  ``complete`` bool [n] and ``trials`` int64 [n] as the kernel left them (a trial: a candidate whose edge checks were
    evaluated; -1 for every pair on a CPU device, where nothing is launched);  ``fallback``: the pairs finished on the host.

    The kernel admits pn <= 16, pm <= 64, gn <= 512 and at most 2048 distinct (src, dst, label) graph edges; any other pair,
    and a pair one of whose work items -- (pair, image of pattern node 0) -- needs more than ``budget`` trials, comes back
    incomplete and is finished on the host over ``threads`` threads (0: all cores): counts by ``dmp_subiso_enumerate``
    without rows, weights from the host-enumerated rows.  The labels are exact either way.  ``budget`` defaults to
    ``DEFAULT_BUDGET`` = 262144: the largest power of two at which a launch of 131072 items that ALL spend it stays under one
    second at the measured 5.4e10 trials per second (0.63 s; profiles/subiso_device_kbench.json).  On a CPU device every pair goes the host road.
    A ragged tuple or an edge endpoint outside its graph is a ``ValueError`` naming the pair, raised before anything is
    uploaded or any library entry is called."""
    import torch
    weights = tuple(weights)
    if any(w not in ("node", "edge") for w in weights):
        raise ValueError("label_pairs: weights is a subset of ('node', 'edge'), got %r" % (weights,))
    flat, pn, pm, gn, gm = _flatten(pairs)
    n = len(pairs)
    device = torch.device(device)
    gno, geo = _offsets(gn), _offsets(gm)
    lim = 2 ** 31
    if device.type == "cuda" and n and max(n, pn.sum(), pm.sum(), gno[-1], geo[-1]) < lim:
        res = launch(build_image(flat, pn, pm, gn, gm), device, weights, budget, fill)
    else:
        if budget is not None and not 1 <= int(budget) <= MAX_BUDGET:
            raise ValueError("label_pairs: budget %d outside 1 .. %d" % (int(budget), MAX_BUDGET))
        res = {"counts": np.zeros(n, np.int64), "trials": np.full(n, -1, np.int64), "complete": np.zeros(n, bool),
               "node_weights": np.zeros(int(gno[-1]), np.int64) if "node" in weights else None,
               "edge_weights": np.zeros(int(geo[-1]), np.int64) if "edge" in weights else None}
    todo = np.flatnonzero(~res["complete"])
    if todo.size:
        res["counts"][todo] = count_subisomorphisms_batch([pairs[i] for i in todo], threads)
        if weights:
            for i in todo.tolist():
                # (an empty pattern has one empty match; the host enumeration cannot shape its rows)
                rows = enumerate_subisomorphisms(*pairs[i]) if pn[i] else np.zeros((1, 0), np.int64)
                nw, ew = weights_from_rows(pairs[i], rows)
                if res["node_weights"] is not None:
                    res["node_weights"][gno[i]:gno[i + 1]] = nw
                if res["edge_weights"] is not None:
                    res["edge_weights"][geo[i]:geo[i + 1]] = ew
    split = lambda a, off: None if a is None else [a[off[i]:off[i + 1]] for i in range(n)]
    return {"counts": res["counts"], "node_weights": split(res["node_weights"], gno), "edge_weights": split(res["edge_weights"], geo),
            "complete": res["complete"], "trials": res["trials"], "fallback": int(todo.size)}


def count_subisomorphisms_device(pairs, device, **kw):
    """``counts`` of the pairs by ``label_pairs`` (int64 [n])."""
    return label_pairs(pairs, device, **kw)["counts"]
