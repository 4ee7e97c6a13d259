"""Thin training / evaluation harness around the drop-in model.

Reproduces the loop semantics of ``SubgraphCountingMatching/train.py:449-844`` (train_epoch) and
``:847-1061`` (evaluate_epoch) for the GraphAdj models on the MI355X path: count loss
``bp_crit(leaky_relu(pred_c, neg_slp), counts)``, evaluation metric on ``relu(pred_c)``, optional
representation regulariser, gradient clipping, AdamW; without the reference's seven ``.item()``
host syncs per step (running sums stay on the device).  Plus a synthetic (pattern, graph) dataset
with exact subgraph-isomorphism counts for smoke-level training runs: the reference's datasets are
external downloads that are not available offline.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from .collate import collate_device, subiso_weights
from .dp import FlatGradSync


def _i64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int64))


def enumerate_subisomorphisms(p_src, p_dst, p_vl, p_el, g_src, g_dst, g_vl, g_el, limit=-1):
    """All label-preserving injective maps of the pattern's nodes into the graph's nodes such that
    every pattern edge (u -> v, label l) has an image edge with the same label (non-induced
    subgraph isomorphisms: a sample's ``subisomorphisms`` rows, whose number is its ``counts``),
    as an int64 array [counts, pattern_nodes] in lexicographic order.  Native depth-first search on the host
    (``dmp_subiso_enumerate``, csrc/dmp_subiso.cpp); ``enumerate_subisomorphisms_py`` is its plain-Python twin."""
    from . import _lib
    lib = _lib.load()
    arrs = [_i64(a) for a in (p_src, p_dst, p_vl, p_el, g_src, g_dst, g_vl, g_el)]
    ps, pd, pvl, pel, gs, gd, gvl, gel = arrs
    P = lambda a: a.ctypes.data if a.size else None
    pn, cap = len(pvl), 1024
    while True:
        rows = np.empty((cap, max(pn, 1)), dtype=np.int64)
        c = int(lib.dmp_subiso_enumerate(pn, len(ps), P(ps), P(pd), P(pvl), P(pel), len(gvl), len(gs), P(gs), P(gd), P(gvl), P(gel),
                                         rows.ctypes.data, cap, int(limit)))
        if c < 0:
            raise ValueError("enumerate_subisomorphisms: edge endpoints outside the graphs")
        if c <= cap:
            return rows[:c, :pn].copy().reshape(-1, pn)
        cap = c


def count_subisomorphisms_batch(pairs, threads=0):
    """``counts`` of many pairs at once over a pool of host threads (``dmp_subiso_count_batch``); ``pairs``: a list of
    ``(p_src, p_dst, p_vl, p_el, g_src, g_dst, g_vl, g_el)``."""
    from . import _lib
    lib = _lib.load()
    n = len(pairs)
    cat = lambda k: _i64(np.concatenate([_i64(p[k]) for p in pairs])) if n else np.zeros(0, np.int64)
    off = lambda k: _i64(np.concatenate([[0], np.cumsum([len(p[k]) for p in pairs])]))
    ps, pd, pvl, pel, gs, gd, gvl, gel = (cat(k) for k in range(8))
    pno, peo, gno, geo = off(2), off(0), off(6), off(4)
    counts = np.zeros(n, np.int64)
    P = lambda a: a.ctypes.data if a.size else None
    rc = lib.dmp_subiso_count_batch(n, P(pno), P(peo), P(ps), P(pd), P(pvl), P(pel), P(gno), P(geo), P(gs), P(gd), P(gvl), P(gel),
                                    P(counts), int(threads))
    if rc != 0:
        raise ValueError("count_subisomorphisms_batch: bad input")
    return counts


def enumerate_subisomorphisms_py(p_src, p_dst, p_vl, p_el, g_src, g_dst, g_vl, g_el):
    """The same enumeration as plain backtracking in Python (cross-check of the native search)."""
    np_, ng = len(p_vl), len(g_vl)
    adj = {}
    for u, v, l in zip(g_src.tolist(), g_dst.tolist(), g_el.tolist()):
        adj.setdefault((u, v), set()).add(l)
    pe = list(zip(p_src.tolist(), p_dst.tolist(), p_el.tolist()))
    touching = [[(u, v, l) for (u, v, l) in pe if u == k or v == k] for k in range(np_)]
    mapping, used = [-1] * np_, [False] * ng

    found = []

    def rec(k):
        if k == np_:
            found.append(tuple(mapping))
            return
        for cand in range(ng):
            if used[cand] or g_vl[cand] != p_vl[k]:
                continue
            mapping[k] = cand
            good = True
            for u, v, l in touching[k]:   # every pattern edge whose endpoints are both placed
                mu, mv = mapping[u], mapping[v]
                if mu >= 0 and mv >= 0 and l not in adj.get((mu, mv), ()):
                    good = False
                    break
            if good:
                used[cand] = True
                rec(k + 1)
                used[cand] = False
            mapping[k] = -1

    rec(0)
    return np.array(found, dtype=np.int64).reshape(-1, np_)


def count_subisomorphisms(p_src, p_dst, p_vl, p_el, g_src, g_dst, g_vl, g_el):
    """``counts`` of a (pattern, graph) pair: the number of subisomorphisms."""
    return int(count_subisomorphisms_batch([(p_src, p_dst, p_vl, p_el, g_src, g_dst, g_vl, g_el)], threads=1)[0])


def _er_edges(n, m, rng):
    total = n * (n - 1)
    pick = rng.choice(total, size=m, replace=False)
    u = pick // (n - 1)
    r = pick % (n - 1)
    return u.astype(np.int64), (r + (r >= u)).astype(np.int64)


class PairDataset:
    """(pattern, graph) samples in memory, stored the way the reference's preprocessing leaves a
    GraphAdj sample: ids = arange, reversed edges appended ([forward | reversed], id + max_ne,
    label + max_nel, is_reversed; train.py:299-327).  ``shape`` holds the dataset-wide maxima the
    model vocabulary is sized by (train.py:1164-1181)."""

    def __init__(self, samples, shape):
        self.samples, self.shape = samples, shape

    @classmethod
    def from_loaded(cls, loaded):
        """Samples as ``dataio.load_data`` returns them (forward edges only) -> PairDataset."""
        mx = lambda f: max([f(x) for x in loaded] + [1])
        shape = dict(p_nodes=mx(lambda x: x["pattern"]["num_nodes"]), p_edges=mx(lambda x: len(x["pattern"]["src"])),
                     g_nodes=mx(lambda x: x["graph"]["num_nodes"]), g_edges=mx(lambda x: len(x["graph"]["src"])),
                     n_vlabels=mx(lambda x: int(max(x["pattern"]["vlabel"].max(initial=0), x["graph"]["vlabel"].max(initial=0))) + 1),
                     n_elabels=mx(lambda x: int(max(x["pattern"]["elabel"].max(initial=0), x["graph"]["elabel"].max(initial=0))) + 1))
        samples = []
        for x in loaded:
            p, g = x["pattern"], x["graph"]
            samples.append({"id": x["id"],
                            "pattern": cls._with_rev(p["src"], p["dst"], p["vlabel"], p["elabel"], shape["p_edges"], shape["n_elabels"]),
                            "graph": cls._with_rev(g["src"], g["dst"], g["vlabel"], g["elabel"], shape["g_edges"], shape["n_elabels"]),
                            "counts": int(x["counts"]), "subisomorphisms": np.asarray(x["subisomorphisms"], np.int64).reshape(-1, p["num_nodes"])})
        return cls(samples, shape)

    @staticmethod
    def _with_rev(u, v, vl, el, max_ne, max_nel):
        e = len(u)
        return {"src": np.concatenate([u, v]), "dst": np.concatenate([v, u]), "vlabel": vl,
                "elabel": np.concatenate([el, el + max_nel]), "eid": np.concatenate([np.arange(e), max_ne + np.arange(e)]),
                "rev": np.concatenate([np.zeros(e, bool), np.ones(e, bool)]), "num_nodes": len(vl)}

    def __len__(self):
        return len(self.samples)

    def subset(self, indices):
        return PairDataset([self.samples[i] for i in indices], self.shape)

    def model_config(self, hid_dim=64, layers=3, rep_net="DMPNN", **kw):
        s = self.shape
        cfg = dict(max_ngv=s["g_nodes"], max_ngvl=s["n_vlabels"], max_nge=2 * s["g_edges"], max_ngel=2 * s["n_elabels"],
                   max_npv=s["p_nodes"], max_npvl=s["n_vlabels"], max_npe=2 * s["p_edges"], max_npel=2 * s["n_elabels"],
                   base=2, hid_dim=hid_dim, share_rep_net=True, rep_residual=True, enc_net="Multihot",
                   emb_net="Orthogonal", filter_net="ScalarFilter", rep_net=rep_net, rep_num_graph_layers=layers,
                   rep_num_pattern_layers=layers, rep_dmpnn_batch_norm=False, rep_act_func="relu",
                   pred_net="SumPredictNet", pred_hid_dim=hid_dim, node_pred=True, edge_pred=True)
        cfg.update(kw)
        return cfg

    def to_files(self, root, shared_graph=False):
        """Write the forward edges of every sample in the reference's directory layout
        (``dataio.save_pairs``); sample ``i`` becomes pattern ``P_<i // 10>`` ... only when the
        samples carry no ids of their own: synthetic sets get ``P_i`` / ``G_i``."""
        from . import dataio
        out = []
        for i, x in enumerate(self.samples):
            fwd = lambda g: {"num_nodes": g["num_nodes"], "src": g["src"][:len(g["src"]) // 2], "dst": g["dst"][:len(g["dst"]) // 2],
                             "vlabel": g["vlabel"], "elabel": g["elabel"][:len(g["elabel"]) // 2]}
            pid, gid = (x["id"].split("-", 1) if "id" in x else ("P_%d" % i, "G_%d" % i))
            out.append({"pattern_id": pid, "graph_id": gid, "pattern": fwd(x["pattern"]), "graph": fwd(x["graph"]),
                        "counts": x["counts"], "subisomorphisms": x["subisomorphisms"]})
        dataio.save_pairs(root, out, shared_graph)

    def batchify(self, indices, device, return_weights=None):
        """``GraphAdjDataset.batchify`` (dataset.py:1604-1636) + ``.to(device)`` (train.py:606-607):
        concatenated local arrays are uploaded once, batching itself happens on the device.  Returns
        ``(pattern, graph, counts [B, 1], (node_weights, edge_weights))``; the weights (pre-padded
        int64 ``[B, max]``, or None) are computed on the device when ``return_weights`` names them."""
        meta, tensors = self.batch_arrays(indices, device)
        out = self.graphs_from_arrays(meta, tensors)
        counts = tensors[-1]
        weights = (None, None)
        if return_weights:
            subs = [self.samples[i]["subisomorphisms"].reshape(-1) for i in indices]
            ptr_host = np.concatenate([[0], np.cumsum([len(x) for x in subs])]).astype(np.int64)
            hint = sum(self.samples[i]["counts"] * len(self.samples[i]["pattern"]["src"]) for i in indices)
            weights = subiso_weights(out[0], out[1], torch.from_numpy(np.concatenate(subs)).to(device),
                                     torch.from_numpy(ptr_host).to(device), return_weights, work_hint=int(hint))
        return out[0], out[1], counts, weights

    def edge_seq(self):
        """The edge-sequence view of this dataset (``EdgeSeqPairs``): what the sequence rep-nets (CNN) train on."""
        if getattr(self, "_edge_seq", None) is None:
            self._edge_seq = EdgeSeqPairs(self)
        return self._edge_seq

    def lrp(self, seq_len=4):
        """The local-relational-pooling view of this dataset (``LRPPairs``): what the LRP / DMPLRP models train on."""
        views = self.__dict__.setdefault("_lrp_views", {})
        if int(seq_len) not in views:
            views[int(seq_len)] = LRPPairs(self, seq_len)
        return views[int(seq_len)]

    def resident(self, device):
        """The view of this dataset that lives on ``device`` (``resident.ResidentPairs``): uploaded once, every batch then
        assembled there by one launch from one small upload.  Same batches, bit for bit; opt-in."""
        from .resident import ResidentPairs
        return ResidentPairs(self, device)

    ARRAYS_PER_GRAPH = 9    # src, dst, num_nodes, num_edges, node id, node label, edge id, edge label, is_reversed

    def pad_buckets(self, batch_size, levels=4):
        """``pad`` for ``batch_arrays``: the per-graph maxima of the dataset per side and the number of capacity levels.  A
        padded batch holds ``batch_size`` real + ``batch_size`` inert pairs and its four totals (nodes / edges of both sides)
        are those of level k of ``levels`` -- k / levels of what ``batch_size`` largest graphs would take, the smallest level
        this batch fits -- so a ragged dataset meets at most ``levels`` batch shapes and a recorded step (``GraphedTrainStep``)
        replays for every batch."""
        out = {"batch": int(batch_size), "levels": int(levels)}
        for key in ("pattern", "graph"):
            out[key] = (max(2, max(int(x[key]["num_nodes"]) for x in self.samples)), max(1, max(len(x[key]["src"]) for x in self.samples)))
        return out

    def sub_capacity(self, batch_size):
        """``subs`` for ``batch_arrays``: the summed length of the ``batch_size`` longest flattened ``subisomorphisms`` arrays
        of the dataset -- what any batch of that many pairs fits.  One number per dataset and batch size."""
        caps = self.__dict__.setdefault("_sub_caps", {})
        key = (int(batch_size), len(self.samples))
        if key not in caps:
            lens = sorted((int(np.asarray(x["subisomorphisms"]).size) for x in self.samples), reverse=True)
            caps[key] = int(sum(lens[:max(0, int(batch_size))]))
        return caps[key]

    def batch_arrays(self, indices, device, pad=None, subs=None):
        """The uploaded half of ``batchify``: ``(meta, tensors)`` with ``tensors`` = the pattern batch's nine arrays
        (local endpoints, sizes, ids, labels, reversed flags), the graph batch's nine and ``counts [B, 1]``, and ``meta``
        = per side ``(total nodes, total edges, largest graph's nodes, largest graph's edges)`` as host ints.  Everything
        ``graphs_from_arrays`` then does happens on the device without a host sync (``dp.StepGraph`` records it).
        ``pad`` (``pad_buckets``): the batch is extended to ``2 pad["batch"]`` pairs by INERT pairs -- pairs of one-label graphs
        (pattern label 0, target label 1: the filter gates wipe the inert target rows) whose sizes take the four totals up to a capacity level, and whose weight in the loss is zero (a last tensor,
        ``weights [2 B, 1]``, is appended).  Pairs are
        independent in the model (block-diagonal batches, no BatchNorm), so the real pairs' predictions are unchanged and
        an inert pair, whose prediction carries no loss, adds exact zeros to every gradient: a ragged dataset then meets a
        handful of batch shapes instead of one per batch.
        ``subs`` (``sub_capacity``): two more tensors at the end, ``sub_flat [subs]`` int64 -- the pairs' ``subisomorphisms``
        rows flattened back to back (one host concatenation, one upload), zeros from the real total on -- and ``sample_ptr
        [pairs + 1]`` int64, the first element of every pair (an inert pair's range is empty; the last entry is the real
        total): the inputs of ``collate.subiso_weights`` at a size that does not depend on the batch."""
        meta, tensors = [], []
        extra, level = 0, 0
        if pad is not None:
            B, K = pad["batch"], pad["levels"]
            if len(indices) > B:
                raise ValueError("batch_arrays(pad=...): more pairs than the padding was laid out for")
            extra = 2 * B - len(indices)                          # inert pairs: the batch always holds 2 B pairs
            tot = {key: (sum(int(self.samples[i][key]["num_nodes"]) for i in indices), sum(len(self.samples[i][key]["src"]) for i in indices))
                   for key in ("pattern", "graph")}
            # level k: k / K of what B largest graphs would take, + one node and one edge for each of B inert graphs (an inert
            # graph without an edge would put 1 / 0 into the heads' length features, pred.py:93-96)
            caps = lambda key, k: (-(-B * pad[key][0] * k // K) + B, -(-B * pad[key][1] * k // K) + B)
            fits = lambda k: all(tot[key][0] + extra <= caps(key, k)[0] and tot[key][1] + extra <= caps(key, k)[1] for key in tot)
            level = next((k for k in range(1, K + 1) if fits(k)), None)
            if level is None:
                raise ValueError("batch_arrays(pad=...): the batch does not fit %d graphs of the dataset's largest size" % B)
        for key in ("pattern", "graph"):
            gs = [self.samples[i][key] for i in indices]
            if pad is not None:
                cn, ce = caps(key, level)
                # an inert TARGET graph carries a node / edge label its (label-0) inert pattern does not use: the filter gates
                # (ScalarFilter: a target row is kept when its label occurs in the pattern) zero every one of its rows, so the
                # gated kernels leave them out and a gate capacity calibrated on the real pairs holds for the padded batch too
                # (label 0 on both sides kept every inert edge: ~3 x the real rows as live work, and with ``gate_compact`` every
                # padded batch overflowed its capacity -- ADVICE r5).  One-label vocabularies have no such label: 0 there.
                lab = (0, 0) if key == "pattern" else (1 if self.shape.get("n_vlabels", 1) > 1 else 0, 1 if self.shape.get("n_elabels", 1) > 1 else 0)
                gs = gs + self._inert_graphs(tot[key], cn, ce, extra, pad[key], vlabel=lab[0], elabel=lab[1])
            cat = lambda k, dt=torch.int64: torch.from_numpy(np.concatenate([g[k] for g in gs])).to(dt).to(device)
            nn_ = np.array([g["num_nodes"] for g in gs], np.int64)
            ne_ = np.array([len(g["src"]) for g in gs], np.int64)
            nid = torch.from_numpy(np.concatenate([np.arange(n) for n in nn_])).to(device)
            tensors += [cat("src"), cat("dst"), torch.from_numpy(nn_).to(device), torch.from_numpy(ne_).to(device), nid,
                        cat("vlabel"), cat("eid"), cat("elabel"), cat("rev", torch.bool)]
            if pad is not None:     # the dataset's per-graph maxima: one signature per capacity level, whatever this batch holds
                meta.append((int(nn_.sum()), int(ne_.sum()), int(pad[key][0]), int(pad[key][1])))
            else:
                meta.append((int(nn_.sum()), int(ne_.sum()), int(nn_.max(initial=0)), int(ne_.max(initial=0))))
        counts = torch.tensor([self.samples[i]["counts"] for i in indices] + [0] * extra, dtype=torch.float32, device=device)
        tail = []
        if subs is not None:
            rows = [np.asarray(self.samples[i]["subisomorphisms"], np.int64).reshape(-1) for i in indices]
            ptr_host = np.zeros(len(indices) + extra + 1, np.int64)
            np.cumsum([len(r) for r in rows], out=ptr_host[1:len(indices) + 1])
            ptr_host[len(indices) + 1:] = ptr_host[len(indices)]
            if ptr_host[-1] > int(subs):
                raise ValueError("batch_arrays(subs=%d): the batch's subisomorphism rows take %d elements" % (int(subs), ptr_host[-1]))
            flat = np.zeros(int(subs), np.int64)
            if ptr_host[-1]:
                flat[:ptr_host[-1]] = np.concatenate(rows)
            tail = [torch.from_numpy(flat).to(device), torch.from_numpy(ptr_host).to(device)]
        if pad is None:
            return tuple(meta), tensors + [counts.unsqueeze(-1)] + tail
        weights = torch.tensor([1.0] * len(indices) + [0.0] * extra, dtype=torch.float32, device=device)
        return tuple(meta), tensors + [counts.unsqueeze(-1), weights.unsqueeze(-1)] + tail

    @staticmethod
    def _inert_graphs(tot, cap_n, cap_e, extra, largest=None, vlabel=0, elabel=0):
        """``extra`` one-label graphs (node label ``vlabel``, edge label ``elabel``) that take a side's node / edge totals ``tot`` up to ``(cap_n, cap_e)``: nodes dealt evenly
        (every inert graph has at least one), edges too (at least one each; a ring over the graph's nodes: valid endpoints,
        parallel edges when the ring wraps).  ``largest``: the dataset's largest graph (nodes, edges) no inert graph may exceed."""
        n_pad, e_pad = cap_n - tot[0], cap_e - tot[1]
        if n_pad < extra or e_pad < extra:
            raise ValueError("batch_arrays(pad=...): the batch does not fit its capacity level")
        out = []
        for j in range(extra):
            n = n_pad // extra + (1 if j < n_pad % extra else 0)
            e = e_pad // extra + (1 if j < e_pad % extra else 0)
            if largest is not None and (n > largest[0] or e > largest[1]):
                raise ValueError("batch_arrays(pad=...): an inert graph would exceed the dataset's largest graph (a batch of empty graphs?)")
            a = np.arange(e, dtype=np.int64) % n
            out.append({"src": a, "dst": (a + 1) % n, "vlabel": np.full(n, vlabel, np.int64), "elabel": np.full(e, elabel, np.int64),
                        "eid": np.arange(e, dtype=np.int64), "rev": np.zeros(e, bool), "num_nodes": n})
        return out

    @classmethod
    def graphs_from_arrays(cls, meta, tensors):
        """``(pattern, graph)`` BatchedGraphs from ``batch_arrays``' output (device collate)."""
        from .collate import collate_device_many
        jobs = []
        for side, (n, e, max_n, max_e) in enumerate(meta):
            src, dst, nn_, ne_, nid, vlabel, eid, elabel, rev = tensors[side * cls.ARRAYS_PER_GRAPH:(side + 1) * cls.ARRAYS_PER_GRAPH]
            jobs.append(dict(local_src=src, local_dst=dst, num_nodes=nn_, num_edges=ne_, total_nodes=n, total_edges=e,
                             ndata={"id": nid, "label": vlabel}, edata={"id": eid, "label": elabel, "is_reversed": rev},
                             max_nodes=max_n, max_edges=max_e))
        return collate_device_many(jobs)                         # both sides in one pair of launches


class LRPPairs(PairDataset):
    """A ``PairDataset`` as the LRP / DMPLRP models need it (the part of the reference's ``LRPDataset``, dataset.py:1642-1862,
    that is not the enumeration itself): once, here on the host, every sample's number of ego-net permutations per side and
    the largest number of distinct neighbours, from the degree sequences alone (``PermIndex.counts_host``: closed form), and
    the check that no graph has a non-reversed self-loop.  The batches it hands out are ``PairDataset``'s, with the hints on
    the graph objects (``lrp_seq_len``, ``lrp_max_degree`` and ``lrp_total`` or ``lrp_capacity``) that let
    ``model(pattern, graph)`` build both permutation indexes on the device without reading anything back.
    ``batch_arrays(perms=perm_capacity(...))``: the indexes are built at a capacity level instead of their exact totals --
    what a recorded step needs; the level is part of ``meta`` (the step's shape signature)."""

    def __init__(self, pairs, seq_len=4):
        from .lrp import PermIndex
        self.samples, self.shape, self.seq_len = pairs.samples, pairs.shape, int(seq_len)
        self.perm_counts = np.zeros((len(self.samples), 2), np.int64)          # [sample, (pattern, graph)]
        self.max_degree = 0
        for i, x in enumerate(self.samples):
            for side, key in enumerate(("pattern", "graph")):
                g = x[key]
                total, deg, loop = PermIndex.counts_host(g["src"], g["dst"], g["num_nodes"], g.get("rev"), self.seq_len)
                if loop:
                    raise ValueError("sample %d (%s): %s has a non-reversed self-loop, which a permutation index cannot hold"
                                     % (i, x.get("id", "?"), key))
                self.perm_counts[i, side] = total
                self.max_degree = max(self.max_degree, deg)

    def lrp(self, seq_len=4):
        return self if int(seq_len) == self.seq_len else PairDataset(self.samples, self.shape).lrp(seq_len)

    def subset(self, indices):
        return PairDataset.subset(self, indices).lrp(self.seq_len)

    def resident(self, device):
        raise NotImplementedError("LRPPairs.resident: the LRP view's batches carry permutation indexes the device store does not hold")

    def model_config(self, hid_dim=64, layers=3, rep_net="DMPLRP", **kw):
        kw.setdefault("lrp_seq_len", self.seq_len)
        return PairDataset.model_config(self, hid_dim, layers, rep_net, **kw)

    def perm_capacity(self, batch_size, levels=4):
        """``perms`` for ``batch_arrays``: per level k = 1 .. ``levels`` the ``(pattern, graph)`` capacities in permutations,
        k / levels of the sum of the ``batch_size`` largest counts of the dataset per side (as ``pad_buckets`` /
        ``sub_capacity`` lay their levels out).  The top level holds any batch of that many pairs."""
        top = [int(np.sort(self.perm_counts[:, side])[::-1][:max(0, int(batch_size))].sum()) for side in (0, 1)]
        return tuple(tuple(-(-t * k // int(levels)) for t in top) for k in range(1, int(levels) + 1))

    def batch_arrays(self, indices, device, pad=None, subs=None, perms=None):
        """``PairDataset.batch_arrays`` with one more entry at the end of ``meta``: ``("lrp", seq_len, max_degree, level,
        pattern total, graph total, pattern capacity, graph capacity)`` -- the exact totals (``perms`` None: an eager step) or
        the capacities at a level of ``perms`` (``perm_capacity``): the smallest level that holds the target side, the top
        level for the pattern side.  With ``pad`` the inert pairs count too: an inert graph is a ring, each of its nodes
        has one neighbour at most and so exactly one permutation, whatever ``seq_len``; a capacity then grows by the padded
        batch's node total (a constant of the padding level)."""
        meta, tensors = PairDataset.batch_arrays(self, indices, device, pad=pad, subs=subs)
        idx = np.asarray(indices, np.int64)
        totals = [int(t) for t in self.perm_counts[idx].sum(axis=0)] if len(idx) else [0, 0]
        if pad is not None:
            for side, key in enumerate(("pattern", "graph")):
                totals[side] += int(meta[side][0]) - sum(int(self.samples[i][key]["num_nodes"]) for i in indices)
        hint = ("lrp", self.seq_len, max(self.max_degree, 1 if pad is not None else 0))
        if perms is None:
            return meta + (hint + (0,) + tuple(totals) + (None, None),), tensors
        grow = [int(meta[side][0]) if pad is not None else 0 for side in (0, 1)]
        # the level is the target side's (where the permutations are: ~100 x the patterns' at the README sizes); the pattern
        # side always takes its top level -- a joint level let a few hundred pattern permutations push the target side up
        level = next((k for k, caps in enumerate(perms, 1) if totals[1] <= caps[1] + grow[1]), None)
        if level is None or totals[0] > perms[-1][0] + grow[0]:
            raise ValueError("batch_arrays(perms=...): the batch's %d / %d permutations exceed the top capacity level" % tuple(totals))
        return meta + (hint + (level, None, None, perms[-1][0] + grow[0], perms[level - 1][1] + grow[1]),), tensors

    @classmethod
    def graphs_from_arrays(cls, meta, tensors):
        _, seq_len, max_degree, _level, p_total, g_total, p_cap, g_cap = meta[-1]
        pattern, graph = super().graphs_from_arrays(meta[:-1], tensors)
        for g, total, cap in ((pattern, p_total, p_cap), (graph, g_total, g_cap)):
            g.lrp_seq_len, g.lrp_max_degree, g.lrp_total, g.lrp_capacity = seq_len, max_degree, total, cap
        return pattern, graph


class EdgeSeqPairs:
    """A ``PairDataset`` as the reference's ``EdgeSeqDataset`` after ``add_reversed_edges`` (dataset.py:885-1052,
    train.py:273-297): every pattern and graph a sorted tuple sequence with its reversed tuples merged in, and the per-tuple
    subisomorphism edge weights, prepared once here on the host.  ``batchify`` has ``PairDataset.batchify``'s signature and
    returns ``(EdgeSeq pattern, EdgeSeq graph, counts [B, 1], (None, edge_weights [B, L] or None))``: one upload and
    index ops per batch (``EdgeSeq.batch``)."""

    def __init__(self, pairs):
        from . import edgeseq
        self.samples, self.shape = pairs.samples, pairs.shape
        nel = int(self.shape["n_elabels"])
        self.seqs = []
        for x in self.samples:
            item = {}
            for key in ("pattern", "graph"):
                g = x[key]
                e = len(g["src"]) // 2                            # the stored form: [forward | reversed] edges
                fwd = edgeseq.from_graph(g["src"][:e], g["dst"][:e], np.arange(g["num_nodes"]), g["vlabel"], g["elabel"][:e])
                code, flag, _ = edgeseq.add_reversed_edges(fwd, nel)
                item[key] = (fwd, code, flag)
            w = edgeseq.edge_weights(item["pattern"][0], item["graph"][0], x["subisomorphisms"], int(x["counts"]))
            item["edge_weights"] = edgeseq.map_reversed_weights(item["graph"][1], item["graph"][2], w, nel)
            self.seqs.append(item)

    def __len__(self):
        return len(self.samples)

    def resident(self, device):
        raise NotImplementedError("EdgeSeqPairs.resident: the edge-sequence view's batches are tuple sequences the device store does not hold")

    def batchify(self, indices, device, return_weights=None):
        from .edgeseq import EdgeSeq
        items = [self.seqs[i] for i in indices]
        if isinstance(return_weights, str):
            return_weights = return_weights.split(",")
        want = bool(return_weights) and "edge" in return_weights
        pattern, _ = EdgeSeq.batch([x["pattern"][1] for x in items], device, flags=[x["pattern"][2] for x in items])
        graph, extra = EdgeSeq.batch([x["graph"][1] for x in items], device, flags=[x["graph"][2] for x in items],
                                     extra=[[x["edge_weights"] for x in items]] if want else None)
        counts = torch.tensor([self.samples[i]["counts"] for i in indices], dtype=torch.float32, device=device).unsqueeze(-1)
        return pattern, graph, counts, (None, extra[0] if want else None)


class SyntheticPairs(PairDataset):
    """Directed ER (pattern, graph) pairs with uniform labels and exact counts."""

    def __init__(self, num_pairs, p_nodes, p_edges, g_nodes, g_edges, n_vlabels, n_elabels, seed=0):
        rng = np.random.default_rng(seed)
        self.shape = dict(p_nodes=p_nodes, p_edges=p_edges, g_nodes=g_nodes, g_edges=g_edges,
                          n_vlabels=n_vlabels, n_elabels=n_elabels)
        self.samples = []
        for _ in range(num_pairs):
            pu, pv = _er_edges(p_nodes, p_edges, rng)
            gu, gv = _er_edges(g_nodes, g_edges, rng)
            pvl, gvl = rng.integers(0, n_vlabels, p_nodes), rng.integers(0, n_vlabels, g_nodes)
            pel, gel = rng.integers(0, n_elabels, p_edges), rng.integers(0, n_elabels, g_edges)
            sub = enumerate_subisomorphisms(pu, pv, pvl, pel, gu, gv, gvl, gel)
            self.samples.append({"pattern": self._with_rev(pu, pv, pvl, pel, p_edges, n_elabels),
                                 "graph": self._with_rev(gu, gv, gvl, gel, g_edges, n_elabels),
                                 "counts": len(sub), "subisomorphisms": sub})


class SmallLikePairs(PairDataset):
    """Ragged (pattern, graph) pairs in the size ranges of the reference's "small" setting (SubgraphCountingMatching/
    README.md:72-94: patterns of at most 8 nodes / 8 edges, graphs of at most 64 nodes / 256 edges, at most 16 labels) with
    exact counts; the published dataset itself is a download that is not available offline.  A pattern is a random
    spanning tree plus random extra edges (connected: an isolated pattern node would multiply the count by the number of
    free graph nodes); a graph is directed ER noise with uniform labels into which 0 .. 12 copies of its pattern are
    planted (node labels overwritten, the pattern's edges added), so that counts are mostly small positive numbers instead
    of zeros and rare explosions.  Counts are EXACT whatever the planting did: they come from the native search over a
    pool of host threads (``count_subisomorphisms_batch``) or, with a ``device``, from the device search
    (``subiso.label_pairs``: the same counts, so a seed yields the same samples either way); the enumerations themselves are
    not kept (count loss only)."""

    def __init__(self, num_pairs, seed=0, threads=0, device=None):
        rng = np.random.default_rng(seed)
        self.shape = dict(p_nodes=8, p_edges=8, g_nodes=64, g_edges=256, n_vlabels=16, n_elabels=16)
        raw = []
        for _ in range(num_pairs):
            pn = int(rng.choice([3, 4, 8]))
            pe = int({3: rng.choice([2, 4]), 4: rng.choice([4, 8]), 8: 8}[pn])
            gn = int(rng.choice([8, 16, 32, 64]))
            ge = int(min(gn * rng.choice([1, 2, 4]), 256))
            nl = int(rng.choice([4, 8, 16]))
            # pattern: a spanning tree in random orientation, then distinct extra ordered pairs
            perm = rng.permutation(pn)
            pairs = set()
            for k in range(1, pn):
                a, b = int(perm[k]), int(perm[rng.integers(0, k)])
                pairs.add((a, b) if rng.random() < 0.5 else (b, a))
            while len(pairs) < pe:
                a, b = int(rng.integers(0, pn)), int(rng.integers(0, pn))
                if a != b:
                    pairs.add((a, b))
            pu, pv = (np.array(x, np.int64) for x in zip(*sorted(pairs)))
            pvl, pel = rng.integers(0, nl, pn), rng.integers(0, nl, pe)
            gvl = rng.integers(0, nl, gn)
            copies = int(rng.integers(0, min(12, gn // pn) + 1))
            edges = {}
            for _c in range(copies):
                where = rng.choice(gn, size=pn, replace=False)
                gvl[where] = pvl
                for u, v, l in zip(pu, pv, pel):
                    edges[(int(where[u]), int(where[v]))] = int(l)
            while len(edges) < ge:                            # ER noise up to the edge budget
                a, b = int(rng.integers(0, gn)), int(rng.integers(0, gn))
                if a != b and (a, b) not in edges:
                    edges[(a, b)] = int(rng.integers(0, nl))
            keys = sorted(edges)[:256]
            gu, gv = (np.array(x, np.int64) for x in zip(*keys))
            gel = np.array([edges[k] for k in keys], np.int64)
            raw.append((pu, pv, pvl, pel, gu, gv, gvl, gel))
        if device is None:
            counts = count_subisomorphisms_batch(raw, threads)
        else:
            from .subiso import label_pairs
            counts = label_pairs(raw, device, threads=threads)["counts"]
        self.samples = []
        for (pu, pv, pvl, pel, gu, gv, gvl, gel), c in zip(raw, counts):
            self.samples.append({"pattern": self._with_rev(pu, pv, pvl, pel, 8, 16), "graph": self._with_rev(gu, gv, gvl, gel, 256, 16),
                                 "counts": int(c), "subisomorphisms": np.zeros((0, len(pvl)), np.int64)})


_CRIT = {"MAE": F.l1_loss, "MSE": F.mse_loss, "SMSE": F.smooth_l1_loss}
_CRIT_KIND = {"MSE": 0, "MAE": 1, "SMSE": 2}


class _CountLossHIP(torch.autograd.Function):
    """``bp_crit(leaky_relu(pred, neg_slope), target)`` (mean) and its gradient seed in ONE launch (``dmp_count_loss``)."""

    @staticmethod
    def forward(ctx, pred, target, kind, neg_slope):
        from . import _lib
        lib = _lib.load()
        p, t = pred.detach().reshape(-1).contiguous(), target.reshape(-1).contiguous()
        _lib.require_gpu(p, t)
        loss = torch.empty(1, dtype=torch.float32, device=p.device)
        dpred = torch.empty_like(p)
        with _lib.timed("count_loss[n=%d]", (p.numel(),), 12 * p.numel()):
            _lib.check(lib.dmp_count_loss(_lib.ptr(p), _lib.ptr(t), p.numel(), int(kind), float(neg_slope), _lib.ptr(loss), _lib.ptr(dpred),
                                          _lib.stream_ptr()), "dmp_count_loss")
        ctx.dpred, ctx.shape = dpred, pred.shape
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        return (ctx.dpred * g).view(ctx.shape), None, None, None


def count_loss(pred, target, bp_loss="MSE", neg_slope=1.0):
    """The count loss of train.py:624-628, ``bp_crit(F.leaky_relu(pred, neg_slope), target)`` with reduction 'mean'
    (``neg_slope`` 1: the plain criterion).  On the GPU, for fp32 tensors of equal size, the criterion, its mean and the
    gradient seed are ONE launch (five as tensor ops); anything else goes through the tensor ops."""
    if (bp_loss in _CRIT_KIND and pred.is_cuda and pred.dtype == torch.float32 and torch.is_tensor(target)
            and target.is_cuda and target.dtype == torch.float32 and not target.requires_grad and target.numel() == pred.numel()
            and 0 < pred.numel() <= (1 << 22) and 0.0 <= float(neg_slope) <= 1.0
            and pred.reshape(-1).shape == target.reshape(-1).shape and (pred.dim() == target.dim() or pred.dim() == 1 or target.dim() == 1)):
        return _CountLossHIP.apply(pred, target, _CRIT_KIND[bp_loss], float(neg_slope))
    act = pred if float(neg_slope) == 1.0 else F.leaky_relu(pred, neg_slope)
    return _CRIT[bp_loss](act, target)
SCHEDULE_CYCLES = 2     # utils/anneal.py:7, utils/cyclical.py:7 (NUM_CYCLES, what train.py:510-562 passes)


def scheduled_value(spec, step, total_steps, cycles=SCHEDULE_CYCLES):
    """A loss weight / slope at optimisation step ``step`` from the reference's specification (config.py:480-515,
    train.py:499-600): a number, ``"anneal_<shape>$a$b"`` (utils/anneal.py: ramp from a to b over the first half of each of
    ``cycles`` periods, then hold b) or ``"cyclical_<shape>$a$b"`` (utils/cyclical.py: a -> b -> a every period); shape is
    ``linear``, ``cosine`` or ``none`` / ``constant`` (always b).  Past ``total_steps``: b."""
    if isinstance(spec, (int, float)):
        return float(spec)
    kind, a, b = spec.rsplit("$", 2)
    a, b = float(a), float(b)
    mode, _, shape = kind.partition("_")
    if mode not in ("anneal", "cyclical"):
        raise ValueError(spec)
    if step > total_steps or shape in ("", "none", "constant"):
        return b
    phase = (cycles * step / max(1, total_steps)) % 1.0          # position inside the current period
    if shape == "linear":
        ramp = lambda t: t
    elif shape == "cosine":
        ramp = lambda t: (1.0 - math.cos(math.pi * t)) / 2.0
    else:
        raise NotImplementedError(shape)
    if mode == "anneal":
        return a + (b - a) * ramp(2.0 * phase) if phase < 0.5 else b
    if shape == "linear":                                         # there and back
        return a + (b - a) * 2.0 * phase if phase < 0.5 else b + (a - b) * (2.0 * phase - 1.0)
    return a + (b - a) * ramp(2.0 * phase)


def lr_factor(name, step, warmup, total, cycles=SCHEDULE_CYCLES, floor=1e-3):
    """Learning-rate multiplier of the reference's schedulers (utils/scheduler.py:12-178) at scheduler step ``step``:
    linear warm-up over ``warmup`` steps where the name says so, then constant / linear / cosine decay towards ``floor``
    over ``total`` steps, ``cycles`` periods, optionally restarting every period."""
    has_warmup = "warmup" in name
    if has_warmup and step < warmup:
        return step / max(1.0, float(warmup))
    if name.startswith("constant"):
        return 1.0
    begin = warmup if has_warmup else 0
    progress = (step - begin) / float(max(1, total - begin))
    if name.startswith("linear"):
        if name.endswith("restart"):
            return floor if progress >= 1.0 else max(floor, 1.0 - (cycles * progress) % 1.0)
        span = total - begin if has_warmup else total            # scheduler.py:49-52 divides by the full length without warm-up
        return max(floor, (total - step) / float(max(1, span)))
    if name.startswith("cosine"):
        if name.endswith("restart"):
            return floor if progress >= 1.0 else max(floor, 0.5 * (1.0 + math.cos(math.pi * ((cycles * progress) % 1.0))))
        return max(floor, 0.5 * (1.0 + math.cos(math.pi * cycles * 2.0 * progress)))
    raise NotImplementedError(name)


class RunSchedule:
    """Everything of a reference run configuration that varies with the optimisation step (train.py:1233-1253 for the
    learning rate, :499-600 for the loss terms), from the ``config`` dictionary of ``config.py`` / ``config.json``."""

    def __init__(self, config, num_train, lr=None):
        self.config = config
        bsz, epochs = config["train_batch_size"], config["train_epochs"]
        self.base_lr = config["lr"] if lr is None else lr
        self.warmup = int(num_train / bsz * 0.5 * min(epochs * 0.06, config.get("early_stop_rounds", 10)))
        self.total = int(num_train / bsz * epochs)
        self.floor = max(1e-3, config.get("weight_decay", 0.0))
        if self.floor > 1e-8:
            self.total -= self.warmup
        self.cycles = max(1, self.total / 20000)
        self.name = config.get("scheduler", "constant")
        self.epoch_steps = int(math.ceil(num_train / bsz))
        self.sched_step = 0

    def lr(self):
        return self.base_lr * lr_factor(self.name, self.sched_step, self.warmup, self.total, self.cycles, self.floor)

    def loss_terms(self, epoch, batch_id):
        step = epoch * self.epoch_steps + batch_id
        total = self.config["train_epochs"] * self.epoch_steps
        c = self.config
        return {k: scheduled_value(c.get(k, d), step, total) for k, d in
                (("neg_pred_slp", 0.0), ("match_loss_w", 0.0), ("match_reg_w", 0.0), ("rep_reg_w", 0.0))}


def _match_terms(crit, pred, weights, mask, pred_c, neg_slp):
    """train.py:627-649: matching loss and regulariser of one of pred_v / pred_e ([B, max_len])."""
    with torch.no_grad():
        weights = weights.float().masked_fill_(~mask, 0)
        pred.masked_fill_(~mask, 0)  # in place on the model output, as the reference does
    loss = crit(F.leaky_relu(pred, neg_slp), weights) * pred.size(1)
    reg = crit(F.relu(pred - pred_c), torch.zeros_like(pred)) * pred.size(1)
    return loss, reg


def _coef3(coef, device, dtype):
    """(neg_slope, match_loss_w, match_reg_w) as a tensor of three numbers on ``device``."""
    if torch.is_tensor(coef):
        return coef.reshape(-1)[:3].to(device=device, dtype=dtype)
    return torch.tensor([float(c) for c in coef], dtype=dtype, device=device)


def match_terms_tensor(pred, weights, mask, pred_c, coef, bp_loss, pair_weights=None):
    """``match_terms`` in tensor ops, any dtype, no host sync (the CPU path, and the fp64 reference of the kernel's tests).
    The definition (see ``match_terms``): real pairs = nonzero ``pair_weights``, n of them; window = the last Lr columns of
    the real pairs, Lr the largest ``Lc - first live column`` among them; x = pred where mask else 0 -- a VALUE-only
    replacement, as ``_match_terms``' in-place ``masked_fill_`` under ``no_grad``: the gradient still reaches ``pred`` at
    a masked window position; sums over the window divided by n (0 for n == 0); exact zeros outside the window."""
    B, Lc = pred.shape
    dt, dev = pred.dtype, pred.device
    c = _coef3(coef, dev, dt)
    mask = mask.reshape(B, Lc) != 0
    real = torch.ones(B, dtype=torch.bool, device=dev) if pair_weights is None else pair_weights.reshape(-1) != 0
    n = real.sum().to(dt)
    inv_n = torch.where(n > 0, 1.0 / n.clamp(min=1), torch.zeros_like(n))
    cols = torch.arange(Lc, device=dev)
    first = torch.where(mask, cols.view(1, -1), torch.full_like(cols, Lc).view(1, -1)).amin(dim=1) if Lc else cols.new_zeros(B)
    ext = torch.where(real, Lc - first, torch.zeros_like(first))
    Lr = ext.amax() if B else cols.new_zeros(())
    window = real.view(-1, 1) & (cols.view(1, -1) >= Lc - Lr)
    x = torch.where(mask, pred, pred - pred.detach())
    t = torch.where(mask, weights.reshape(B, Lc).to(dt), torch.zeros((), dtype=dt, device=dev))
    zero = torch.zeros_like(x)
    crit = _CRIT[bp_loss]
    act = torch.where(x > 0, x, x * c[0])
    loss = torch.where(window, crit(act, t, reduction="none"), zero).sum() * inv_n
    reg = torch.where(window, crit(F.relu(x - pred_c.reshape(B, 1)), zero, reduction="none"), zero).sum() * inv_n
    return c[1] * loss + c[2] * reg, loss, reg


class _MatchLossHIP(torch.autograd.Function):
    """One matching term and the gradient seeds of its weighted sum in three launches (``dmp_match_loss``)."""

    @staticmethod
    def forward(ctx, pred, pred_c, weights, mask, coef, kind, pair_weights):
        from . import _lib
        from .attn import _out
        lib = _lib.load()
        B, Lc = pred.shape
        p = pred.detach()
        if p.stride(1) != 1 or p.stride(0) < Lc:
            p = p.contiguous()
        c = pred_c.detach().reshape(-1).contiguous()
        w = weights.reshape(B, Lc).contiguous()
        m = mask.reshape(B, Lc).contiguous()
        m = m.view(torch.uint8) if m.dtype == torch.bool else (m != 0).view(torch.uint8)
        pw = None if pair_weights is None else pair_weights.detach().reshape(-1).contiguous()
        _lib.require_gpu(p, c, w, m, coef, pw)
        words = int(lib.dmp_match_loss_workspace_words(B, Lc))
        if words <= 0:
            raise _lib.DmpError("dmp_match_loss: shape [%d, %d] is outside the kernel's range" % (B, Lc))
        dev = p.device
        ws = torch.empty(words, dtype=torch.int32, device=dev)
        terms, dpred, dpred_c = _out((3,), torch.float32, dev), _out((B, Lc), torch.float32, dev), _out((B,), torch.float32, dev)
        with _lib.timed("match_loss[B=%d,Lc=%d]", (B, Lc), 17 * B * Lc):
            _lib.check(lib.dmp_match_loss(_lib.ptr(p), p.stride(0), _lib.ptr(w), _lib.ptr(m), _lib.ptr(c), _lib.ptr(pw), _lib.ptr(coef),
                                          B, Lc, int(kind), _lib.ptr(terms), _lib.ptr(dpred), _lib.ptr(dpred_c), _lib.ptr(ws),
                                          _lib.stream_ptr()), "dmp_match_loss")
        ctx.dpred, ctx.dpred_c, ctx.c_shape = dpred, dpred_c, pred_c.shape
        total, loss, reg = terms[2], terms[0], terms[1]
        ctx.mark_non_differentiable(loss, reg)
        return total, loss, reg

    @staticmethod
    def backward(ctx, g, _gl, _gr):
        return ctx.dpred * g, (ctx.dpred_c * g).view(ctx.c_shape), None, None, None, None, None


def match_terms(pred, weights, mask, pred_c, coef, bp_loss, pair_weights=None):
    """The matching loss and regulariser of train.py:627-649 for one of pred_v / pred_e, aware of a padded batch:
    ``(match_loss_w * loss + match_reg_w * reg, loss, reg)`` with

        loss = (1/n) sum_window crit(leaky_relu(x, neg_slope) - t),     reg = (1/n) sum_window crit(relu(x - pred_c[i]))

    ``pred`` [B, Lc], ``weights`` [B, Lc] (the pre-padded subisomorphism weights), ``mask`` [B, Lc], ``pred_c`` [B] or
    [B, 1], ``coef`` = (neg_slope, match_loss_w, match_reg_w) as three numbers or a device tensor, ``pair_weights`` [B]
    of 0 / 1 (0: an inert pair of a padded batch).  n = the real pairs; the window = the last Lr columns of the real
    pairs, Lr the longest stretch from a real pair's first live column to the row's end; x / t = pred / weights where
    ``mask``, else 0.  On an unpadded batch this is ``_match_terms`` (which stays the restatement it is checked against),
    its treatment of masked positions included; a padded batch gives what its real pairs alone give.  Unlike
    ``_match_terms`` it leaves ``pred`` as it is.  On the GPU in fp32 (int64 weights, a criterion of the kernel) it is one
    autograd node over ``dmp_match_loss`` -- three launches, the coefficients read on the device, so a recorded step
    replays with the values of its step --; anything else, and a shape the kernel refuses, goes through
    ``match_terms_tensor``."""
    B, Lc = pred.shape
    if (bp_loss in _CRIT_KIND and pred.is_cuda and pred.dtype == torch.float32 and pred_c.dtype == torch.float32 and pred_c.is_cuda
            and torch.is_tensor(weights) and weights.is_cuda and weights.dtype == torch.int64 and not weights.requires_grad
            and mask.is_cuda and pred_c.numel() == B and weights.numel() == B * Lc and mask.numel() == B * Lc
            and (pair_weights is None or (pair_weights.is_cuda and pair_weights.dtype == torch.float32 and pair_weights.numel() == B))):
        from . import _lib
        if int(_lib.load().dmp_match_loss_workspace_words(B, Lc)) > 0:       # 0: DMP_ERR_UNSUPPORTED for this shape
            c = _coef3(coef, pred.device, torch.float32).contiguous()
            return _MatchLossHIP.apply(pred, pred_c, weights, mask, c, _CRIT_KIND[bp_loss], pair_weights)
    return match_terms_tensor(pred, weights, mask, pred_c, coef, bp_loss, pair_weights)


def train_epoch(model, optimizer, dataset, batch_size, device, sync=None, bp_loss="MSE", eval_metric="MAE",
                neg_slp=0.0, rep_reg_w=0.0, match_loss_w=0.0, match_reg_w=0.0, max_grad_norm=8.0, order=None,
                schedule=None, epoch=0, match_weights=("node", "edge"), trace=None, graph=None):
    """One pass over ``dataset`` (train.py:449-844): count loss, optional representation regulariser
    and, with ``match_loss_w`` / ``match_reg_w`` and a model built with ``pred_return_weights``, the
    node / edge matching losses against the batch's subisomorphism weights.  With a ``RunSchedule`` the four loss
    coefficients and the learning rate follow the run configuration step by step, as train.py:499-600,686 do.  Returns
    ``{"bp_loss", "eval_metric"}`` (sample-weighted means, one host sync at the end).  ``trace``: a list that receives
    one ``(loss, eval_metric)`` pair of device scalars per step (what the reference writes to its SummaryWriter).
    ``graph``: a ``GraphedTrainStep`` (see there) -- batches whose shape it has recorded are one HIP graph replay each;
    steps with matching terms go to it when it was built with exactly those terms (``match_weights``), else they run here."""
    model.train()
    sync = sync or FlatGradSync(model)
    order = np.arange(len(dataset)) if order is None else np.asarray(order)
    tot_loss = torch.zeros((), device=device)
    tot_eval = torch.zeros((), device=device)
    cnt = 0
    if isinstance(match_weights, str):
        match_weights = tuple(w for w in match_weights.split(",") if w in ("node", "edge"))
    for b_id, i in enumerate(range(0, len(order), batch_size)):
        idx = order[i:i + batch_size]
        if schedule is not None:
            terms = schedule.loss_terms(epoch, b_id)
            neg_slp, match_loss_w, match_reg_w, rep_reg_w = (terms["neg_pred_slp"], terms["match_loss_w"], terms["match_reg_w"],
                                                             terms["rep_reg_w"])
            for group in optimizer.param_groups:
                group["lr"] = schedule.lr()
        want = (tuple(match_weights) or None) if (match_loss_w > 0 or match_reg_w > 0) else None
        # a recorded step computes the terms it was built with: it takes the batch when those are the wanted ones (with both
        # coefficients 0 its matching terms are multiplied by 0 on the device: the same step, still one replay)
        if graph and (want is None or set(want) == set(getattr(graph, "match_weights", ()))):
            loss, ev = (graph(dataset, idx, device, neg_slp, rep_reg_w, match_loss_w, match_reg_w) if getattr(graph, "match_weights", ())
                        else graph(dataset, idx, device, neg_slp, rep_reg_w))
            if schedule is not None:
                schedule.sched_step += 1
            with torch.no_grad():
                if trace is not None:
                    trace.append((loss.clone(), ev.clone()))
                tot_loss += loss * len(idx)
                tot_eval += ev * len(idx)
            cnt += len(idx)
            continue
        pattern, graph_b, counts, (node_w, edge_w) = dataset.batchify(idx, device, return_weights=want)
        sync.detach_grads()
        # the representation regulariser reads the last layer's edge rows: with it the layer forms them itself (the deferred
        # form would run the layer's forward a second time on first access)
        lazy, model.lazy_edge_rep = getattr(model, "lazy_edge_rep", True), not (rep_reg_w > 0)
        try:
            out = model(pattern, graph_b)
        finally:
            model.lazy_edge_rep = lazy
        pred = out["pred_c"]
        loss = count_loss(pred, counts, bp_loss, neg_slp) if pred.shape == counts.shape else _CRIT[bp_loss](F.leaky_relu(pred, neg_slp), counts)
        for w, pk, mk in ((node_w, "pred_v", "g_v_mask"), (edge_w, "pred_e", "g_e_mask")):
            if w is not None and out[pk] is not None:
                if pk == "pred_e":      # train.py:636-641 (the graph models' refine_edge_weights is the identity)
                    with torch.no_grad():
                        w = model.refine_edge_weights(w.float())
                m_loss, m_reg = _match_terms(_CRIT[bp_loss], out[pk], w, out[mk], pred, neg_slp)
                loss = loss + match_loss_w * m_loss + match_reg_w * m_reg
        if rep_reg_w > 0:  # train.py:651-659 (bp_crit with slope 1: the plain criterion against zeros)
            reg = sum(_CRIT[bp_loss](out[k], torch.zeros_like(out[k])) * out[k].size(1)
                      for k in ("p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep") if out[k] is not None)
            loss = loss + rep_reg_w * reg
        loss.backward()
        sync.pack()
        sync.sync()
        if max_grad_norm > 0:
            torch.nn.utils.clip_grad_norm_(sync.params, max_grad_norm)
        optimizer.step()
        if schedule is not None:
            schedule.sched_step += 1
        with torch.no_grad():
            if trace is not None:
                trace.append((loss.detach(), _CRIT[eval_metric](F.relu(pred), counts)))
            tot_loss += loss.detach() * len(idx)
            tot_eval += _CRIT[eval_metric](F.relu(pred), counts) * len(idx)
        cnt += len(idx)
    return {"bp_loss": float(tot_loss / max(cnt, 1)), "eval_metric": float(tot_eval / max(cnt, 1))}


class _RecordedStep:
    """What the recorded steps (``GraphedTrainStep``, ``GraphedEvalStep``) share, each rule stated once: which models a
    recording takes, when and how a batch is padded, and the capacities (subisomorphism rows, LRP permutation indexes)
    that keep a batch's tensors at a shape the recording has seen."""

    _EAGER = "runs eagerly"          # how the refusal of an edge-sequence model names the eager route

    def _init_shared(self, model, max_shapes, pad, match_weights, exact_shapes=False):
        """``exact_shapes``: a step that reads every row of the batch (the representation regulariser) is never padded;
        neither is a model with BatchNorm layers (their statistics would see the inert rows)."""
        from .seqmodel import EdgeSeqModel
        if isinstance(model, EdgeSeqModel):
            raise ValueError("%s records the graph models' steps only: %s (an edge-sequence model) %s"
                             % (type(self).__name__, type(model).__name__, self._EAGER))
        self.model = model
        if isinstance(match_weights, str):
            match_weights = match_weights.split(",")
        self.match_weights = tuple(w for w in ("node", "edge") if w in (match_weights or ()))
        self._sub_caps = {}
        self._perm_caps = {}
        self.dataset_cls = None
        self.pad, self._pad_spec = pad, None
        if pad and (exact_shapes or any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) for m in model.modules())):
            self.pad = None
        self.max_shapes = int(max_shapes)

    def _padding(self, dataset, indices):
        """The dataset's padding layout (``pad_buckets``), decided at the first batch: the batch size is that batch's."""
        if self.pad and self._pad_spec is None:
            ragged = len({(int(x[k]["num_nodes"]), len(x[k]["src"])) for x in dataset.samples for k in ("pattern", "graph")}) > 2
            self._pad_spec = dataset.pad_buckets(len(indices), levels=self.max_shapes) if (self.pad is True or ragged) else False
        return self._pad_spec or None

    def _batch_kwargs(self, dataset, indices):
        """The keyword arguments of ``dataset.batch_arrays`` for this batch: the padding when the batch fits it, the LRP
        view's permutation capacities (refused outside the device index build) and, with ``match_weights``, the
        subisomorphism rows' capacity -- one of each per batch size."""
        self.dataset_cls = type(dataset)
        if getattr(self, "_samples", None) is not dataset.samples:      # another dataset: a layout and capacities of its own
            self._samples, self._pad_spec = dataset.samples, None
            self._sub_caps.clear()
            self._perm_caps.clear()
        lrp = hasattr(dataset, "perm_capacity")         # the LRP view: both permutation indexes at a capacity level
        pad = self._padding(dataset, indices)
        if pad is not None and len(indices) > pad["batch"]:
            pad = None
        kw = {} if pad is None else {"pad": pad}
        size = pad["batch"] if pad is not None else len(indices)      # one capacity per batch size: what any such batch fits
        if lrp:
            from . import _abi
            if dataset.max_degree > _abi.DMP_LRP_MAX_NEIGHBOURS or not 1 <= dataset.seq_len <= _abi.DMP_LRP_MAX_SEQ_LEN:
                raise ValueError("%s: a node with %d distinct neighbours / lrp_seq_len %d is outside the device index build "
                                 "(the host build cannot be recorded): run eagerly"
                                 % (type(self).__name__, dataset.max_degree, dataset.seq_len))
            if size not in self._perm_caps:
                self._perm_caps[size] = dataset.perm_capacity(size, levels=self.max_shapes)
            kw["perms"] = self._perm_caps[size]
        if self.match_weights:
            if size not in self._sub_caps:
                self._sub_caps[size] = dataset.sub_capacity(size)
            kw["subs"] = self._sub_caps[size]
        return kw

    def _subiso(self, meta, pattern, graph, subs):
        """The batch's ``(node, edge)`` subisomorphism weights on the device from ``(sub_flat, sample_ptr)`` at the dataset's
        capacity.  The work of the edge-weight kernel (rows x pattern edges) sizes its grid only: a constant of the
        recording, from the capacity and the largest pattern."""
        hint = int(subs[0].numel()) * max(1, int(meta[0][3])) // max(1, int(meta[0][2]))
        return subiso_weights(pattern, graph, subs[0], subs[1], self.match_weights, validate=False, work_hint=hint)


class GraphedTrainStep(_RecordedStep):
    """The training step of ``train_epoch`` (collate, forward, count loss and, with ``match_weights``, the subisomorphism
    weights and the matching terms, backward, gradient pack, clipping, AdamW) as ONE HIP graph per batch shape (``dp.StepGraph``): at the reference's own batch size (64 pairs of small
    graphs, config.py) a step is ~150 launches of microseconds each behind ~3 ms of Python, and a replay is a single
    ``hipGraphLaunch``.  Needs one rank (no collective is recorded), ``FlatAdamW(capturable=True)`` and a dataset with
    ``batch_arrays`` / ``graphs_from_arrays``.  The negative slope of the losses, the representation regulariser's weight
    and the two matching coefficients are device scalars written before every replay (a coefficient annealed to 0
    multiplies its term by 0 on the device: the step keeps replaying), the learning rate goes through
    ``optimizer.sync_hyper()``.  Batches of a shape seen for the first time, and shapes beyond ``max_shapes``
    recordings, run eagerly -- through the same function, so both ways compute the same step.  Run the training loop
    under ``with step.steps.on_stream():`` when it also copies sizeable tensors between host and device (checkpoints,
    predictions): see ``dp.StepGraph`` (``fit(graph=True)`` does)."""

    _EAGER = "trains eagerly (train_epoch without graph=...)"

    def __init__(self, model, optimizer, sync, bp_loss="MSE", eval_metric="MAE", max_grad_norm=8.0, with_rep_reg=False,
                 max_shapes=4, pad="auto", match_weights=()):
        """``pad``: ragged datasets (every batch another pair of (N, E) totals: the reference's bucket-sorted batches,
        utils/sampler.py:10-84, train.py:1283-1290) never repeat a shape, so nothing would replay.  ``"auto"`` / True:
        batches are padded with inert pairs to one of ``max_shapes`` capacity levels (``PairDataset.batch_arrays(pad=...)``;
        "auto": only when the dataset's graphs differ in size); the inert pairs carry weight 0 in the loss and the metric.
        Not with the representation regulariser (it reads every row) or BatchNorm layers (their statistics would see the
        inert rows): such runs keep the exact shapes.
        ``match_weights``: a tuple out of "node" and "edge" -- the step then takes the batch's subisomorphism rows at a
        fixed capacity (``PairDataset.sub_capacity``: no new batch shape), computes the weights on the device
        (``collate.subiso_weights``) and adds ``match_terms`` for every named term whose head the model has; the inert
        pairs of a padded batch are left out of the terms by their pair weights.
        ``hyper``, the step's last input, holds the four device scalars as (rep_reg_w, neg_slp, match_loss_w, match_reg_w):
        in this order its last three are the contiguous coefficient triple ``dmp_match_loss`` reads.  Nothing outside this
        class reads it."""
        from .dp import StepGraph
        self._init_shared(model, max_shapes, pad, match_weights, exact_shapes=with_rep_reg)
        if getattr(sync, "world", 1) != 1:
            raise ValueError("GraphedTrainStep records single-rank steps only")
        if not getattr(optimizer, "capturable", False):
            raise ValueError("GraphedTrainStep needs FlatAdamW(capturable=True)")
        self.optimizer, self.sync = optimizer, sync
        self.bp, self.ev, self.max_grad_norm, self.with_rep_reg = _CRIT[bp_loss], _CRIT[eval_metric], max_grad_norm, with_rep_reg
        self.bp_name = bp_loss
        self.hyper = None
        self._hyper_host = None
        self.steps = StepGraph(self._step, optimizer=optimizer, max_shapes=max_shapes)

    def _step(self, meta, *tensors):
        pattern, graph = self.dataset_cls.graphs_from_arrays(meta, tensors)
        n = 2 * self.dataset_cls.ARRAYS_PER_GRAPH
        counts, hyper = tensors[n], tensors[-1]                 # hyper: (rep_reg_w, neg_slp, match_loss_w, match_reg_w)
        subs = tensors[-3:-1] if self.match_weights else ()       # (sub_flat at the dataset's capacity, sample_ptr)
        weights = tensors[n + 1] if len(tensors) == n + 3 + len(subs) else None        # a padded batch: 1 for the real pairs, 0 for the inert ones
        self.sync.detach_grads()
        lazy, self.model.lazy_edge_rep = getattr(self.model, "lazy_edge_rep", True), not self.with_rep_reg   # see train_epoch
        try:
            out = self.model(pattern, graph)
        finally:
            self.model.lazy_edge_rep = lazy
        pred = out["pred_c"]
        act = torch.where(pred > 0, pred, pred * hyper[1])                        # leaky_relu with the slope on the device
        if weights is not None:      # the mean over the REAL pairs (train.py:463-480's batch mean)
            loss = (self.bp(act, counts, reduction="none") * weights).sum() / weights.sum()
        else:
            loss = self.bp(act, counts)
        if self.with_rep_reg:
            reg = sum(self.bp(out[k], torch.zeros_like(out[k])) * out[k].size(1)
                      for k in ("p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep") if out[k] is not None)
            loss = loss + hyper[0] * reg
        if subs:
            with torch.no_grad():
                node_w, edge_w = self._subiso(meta, pattern, graph, subs)
                if edge_w is not None:                        # train.py:636-641 (the graph models' is the identity)
                    edge_w = self.model.refine_edge_weights(edge_w)
            for w, pk, mk in ((node_w, "pred_v", "g_v_mask"), (edge_w, "pred_e", "g_e_mask")):
                if w is not None and out[pk] is not None:
                    loss = loss + match_terms(out[pk], w, out[mk], pred, hyper[1:4], self.bp_name, pair_weights=weights)[0]
        loss.backward()
        self.sync.pack()
        self.sync.sync()
        if self.max_grad_norm > 0:
            torch.nn.utils.clip_grad_norm_(self.sync.params, self.max_grad_norm)
        self.optimizer.step()
        with torch.no_grad():
            if weights is not None:
                return loss.detach(), (self.ev(F.relu(pred), counts, reduction="none") * weights).sum() / weights.sum()
            return loss.detach(), self.ev(F.relu(pred), counts)

    def __call__(self, dataset, indices, device, neg_slp=0.0, rep_reg_w=0.0, match_loss_w=0.0, match_reg_w=0.0):
        if rep_reg_w > 0 and not self.with_rep_reg:
            raise ValueError("GraphedTrainStep(with_rep_reg=True) to train with the representation regulariser")
        if (match_loss_w > 0 or match_reg_w > 0) and not self.match_weights:
            raise ValueError("GraphedTrainStep(match_weights=...) to train with the matching terms")
        meta, tensors = dataset.batch_arrays(indices, device, **self._batch_kwargs(dataset, indices))
        if self.hyper is None:
            self.hyper = torch.zeros(4, dtype=torch.float32, device=device)
        host = (float(rep_reg_w), float(neg_slp), float(match_loss_w), float(match_reg_w))
        if self._hyper_host != host:
            for k, v in enumerate(host):
                if self._hyper_host is None or self._hyper_host[k] != v:
                    self.hyper[k:k + 1].fill_(v)
            self._hyper_host = host
        return self.steps(meta, *tensors, self.hyper)


def binary_auc(target, pred):
    """``sklearn.metrics.roc_auc_score`` of two BINARY vectors (train.py:1014: ``counts > 0`` against ``relu(pred_c) > 0``):
    a one-threshold ROC curve, whose area is (TPR + TNR) / 2.  NaN when ``target`` holds one class only (sklearn raises)."""
    t, p = target.reshape(-1) != 0, pred.reshape(-1) != 0
    pos, neg = int(t.sum()), int((~t).sum())
    if pos == 0 or neg == 0:
        return float("nan")
    return 0.5 * (int((t & p).sum()) / pos + int((~t & ~p).sum()) / neg)


class EvalBuffers:
    """What ``eval_terms`` writes for one evaluation pass, all on ``device``: ``rows`` [4, cap] fp32 -- ``pred`` (row 0),
    ``target`` (1) and the two matching heads' per-pair errors ``err`` (2: node, 3: edge) --, ``cursor`` int64 [1] (the rows
    written so far), ``sums`` float64 [4] (pairs, sum |e|, sum e^2, sum smooth_l1(e)) and ``overflow`` int32 [1]."""

    def __init__(self, cap, device):
        self.cap = int(cap)
        self.rows = torch.zeros((4, self.cap), dtype=torch.float32, device=device)
        self.pred, self.target, self.err = self.rows[0], self.rows[1], (self.rows[2], self.rows[3])
        self.cursor = torch.zeros(1, dtype=torch.int64, device=device)
        self.sums = torch.zeros(4, dtype=torch.float64, device=device)
        self.overflow = torch.zeros(1, dtype=torch.int32, device=device)

    def reset(self):
        self.cursor.zero_()
        self.sums.zero_()
        self.overflow.zero_()


def eval_terms_tensor(pred_c, target, heads, buf, pair_weights=None):
    """``eval_terms`` in tensor ops (the CPU path, the route of a batch the kernel refuses, and the restatement the kernel
    is tested against).  The definition (see ``eval_terms``): real pairs = nonzero ``pair_weights``; their rows, compacted
    in batch order, start at ``buf.cursor``; rows at or beyond ``buf.cap`` are dropped and raise ``buf.overflow``.  The
    boolean gather reads the number of real pairs back on a device: not for a recording."""
    p, t = F.relu(pred_c.detach().reshape(-1)), target.reshape(-1).to(pred_c.dtype)
    n = p.numel()
    real = torch.ones(n, dtype=torch.bool, device=p.device) if pair_weights is None else pair_weights.reshape(-1) != 0
    row = buf.cursor + torch.cumsum(real, 0) - 1
    keep = real & (row < buf.cap)
    dest = row[keep]
    buf.pred[dest] = p[keep].to(buf.pred.dtype)
    buf.target[dest] = t[keep].to(buf.target.dtype)
    for k, head in enumerate(heads or ()):
        if head is not None:
            pred, w = head
            err = (F.relu(pred.detach()) - w.reshape(pred.shape).to(pred.dtype)).abs().sum(dim=1)
            buf.err[k][dest] = err[keep].to(buf.err[k].dtype)
    e = (p - t)[real].double()               # the difference in the predictions' own precision, as torch forms it, then widened
    a = e.abs()
    count = real.sum()
    buf.sums += torch.stack([count.double(), a.sum(), (e * e).sum(), torch.where(a < 1, 0.5 * e * e, a - 0.5).sum()])
    buf.overflow |= (buf.cursor + count > buf.cap).to(buf.overflow.dtype)
    buf.cursor += count
    return buf.sums


def eval_terms(pred_c, target, heads, buf, pair_weights=None):
    """What one evaluation batch leaves in ``buf`` (``EvalBuffers``), with no host read: for the REAL pairs (nonzero
    ``pair_weights`` [n], None: every pair; a 0 marks an inert pair of a padded batch, anywhere in the batch), compacted
    in batch order at rows ``cursor .. cursor + real - 1``,

        pred[row] = relu(pred_c[i])    target[row] = target[i]    err[k][row] = sum_j |relu(pred_k[i, j]) - float(w_k[i, j])|

    for each of the up to two ``heads`` (``(pred [n, Lc], weights [n, Lc])`` or None; k = 0 node, 1 edge; the sum runs
    over the whole padded row and masks nothing: train.py:952,967), ``sums`` grows by the real pairs' (1, |e|, e^2,
    smooth_l1(e)) with e = relu(pred_c) - target formed in fp32 and summed in fp64, and ``cursor`` advances by the
    number of real pairs.  Rows at or beyond ``buf.cap`` are not written; they raise ``buf.overflow``.  Returns ``buf.sums``.
    On the GPU in fp32 with int64 weights it is one launch of ``dmp_eval_terms`` (one workgroup, fixed summation order);
    anything else, and a batch the kernel refuses (more than 2^22 pairs), goes through ``eval_terms_tensor``."""
    heads = tuple(heads or ())
    if len(heads) > 2:
        raise ValueError("eval_terms: at most two matching heads (node, edge)")
    heads = (heads + (None, None))[:2]
    n = pred_c.numel()
    cuda32 = lambda x: x.is_cuda and x.dtype == torch.float32
    if (cuda32(pred_c) and cuda32(target) and target.numel() == n and buf.rows.is_cuda and n <= 1 << 22
            and (pair_weights is None or (cuda32(pair_weights) and pair_weights.numel() == n))
            and all(h is None or (cuda32(h[0]) and h[0].dim() == 2 and h[0].size(0) == n and 1 <= h[0].size(1) <= 1 << 30 and h[1].is_cuda
                                  and h[1].dtype == torch.int64 and h[1].numel() == h[0].numel()) for h in heads)):
        from . import _lib
        lib = _lib.load()
        p, t = pred_c.detach().reshape(-1).contiguous(), target.reshape(-1).contiguous()
        pw = None if pair_weights is None else pair_weights.detach().reshape(-1).contiguous()
        args, keep = [], [p, t, pw]
        for k, h in enumerate(heads):
            if h is None:
                args += [None, 0, None, 0, None]
                continue
            hp, hw = h[0].detach(), h[1].reshape(h[0].shape).contiguous()
            if hp.stride(1) != 1 or hp.stride(0) < hp.size(1):
                hp = hp.contiguous()
            keep += [hp, hw]
            args += [_lib.ptr(hp), hp.stride(0), _lib.ptr(hw), hp.size(1), _lib.ptr(buf.err[k])]
        _lib.require_gpu(*keep, buf.rows, buf.cursor, buf.sums, buf.overflow)
        moved = 12 * n + sum(12 * h[0].numel() for h in heads if h is not None)
        with _lib.timed("eval_terms[n=%d]", (n,), moved):
            rc = lib.dmp_eval_terms(_lib.ptr(p), _lib.ptr(t), _lib.ptr(pw), n, *args, _lib.ptr(buf.cursor), buf.cap, _lib.ptr(buf.pred),
                                    _lib.ptr(buf.target), _lib.ptr(buf.sums), _lib.ptr(buf.overflow), _lib.stream_ptr())
        if rc != -2:        # DMP_ERR_UNSUPPORTED: the tensor ops below
            _lib.check(rc, "dmp_eval_terms")
            return buf.sums
    return eval_terms_tensor(pred_c, target, heads, buf, pair_weights)


class GraphedEvalStep(_RecordedStep):
    """The forward-only twin of ``GraphedTrainStep``: one batch of ``evaluate_epoch`` (collate, the model's forward in eval
    mode without a gate capacity, with ``match_weights`` the subisomorphism weights, ``eval_terms``) as ONE HIP graph per
    batch shape.  Nothing of a batch is read on the host: predictions, counts and per-pair matching errors collect in
    result buffers on the device behind a device-side cursor, the metrics' sums in four fp64 accumulators
    (``EvalBuffers``); ``evaluate_epoch(graph=step)`` reads them once at the end of the pass.  Padding, the LRP view's
    permutation capacities and the refusals are ``GraphedTrainStep``'s.  On a CPU device the step runs directly.

    The buffers, the cursor and the sums are state the recorded function updates in place -- as a training step updates
    the parameters --, NOT arguments of it: ``dp.StepGraph`` copies an argument into a buffer of the recording's own, so a
    result written through an argument would stay in that copy, and a cursor passed as one would be overwritten by the
    caller's before every replay.  ``begin`` keeps the buffers while they are large enough; when a pass needs more rows it
    allocates larger ones and drops the recordings, which hold the old addresses (they are made again, one per shape).
    ``steps_like``: the ``dp.StepGraph`` of the run's training step -- this object's recordings then share its side
    stream, so a loop that trains and evaluates under one ``on_stream()`` meets one side stream only."""

    _EAGER = "is evaluated eagerly (evaluate_epoch without graph=...)"

    def __init__(self, model, eval_metric="MAE", max_shapes=4, pad="auto", match_weights=(), steps_like=None):
        if eval_metric not in _CRIT:
            raise ValueError("GraphedEvalStep: eval_metric %r (one of %s)" % (eval_metric, ", ".join(_CRIT)))
        self._init_shared(model, max_shapes, pad, match_weights)
        self.eval_metric = eval_metric
        self._steps_like = steps_like
        self.buffers = None
        self.heads_seen = [False, False]
        self.steps = self._new_steps()

    def _new_steps(self):
        from .dp import StepGraph
        old = getattr(self, "steps", None)                       # recordings are dropped, the side stream is kept
        stream = self._steps_like.stream if self._steps_like is not None else (old._stream if old is not None else None)
        return StepGraph(self._step, max_shapes=self.max_shapes, stream=stream)

    def on_stream(self, device=None):
        """``steps.on_stream()`` for a pass on a GPU (``device``, or where the buffers live); nothing on a CPU device."""
        import contextlib
        cuda = torch.device(device).type == "cuda" if device is not None else (self.buffers is not None and self.buffers.rows.is_cuda)
        return self.steps.on_stream() if cuda else contextlib.nullcontext()

    def begin(self, n_rows, device):
        """Start a pass of ``n_rows`` pairs (call it under ``on_stream(device)``, as the batches): cursor, sums and overflow
        word zeroed; the result buffers are kept while they hold ``n_rows`` rows on ``device`` and regrown (the recordings
        dropped with them) when they do not."""
        device = torch.device(device)
        buf = self.buffers
        if buf is None or buf.cap < n_rows or buf.rows.device.type != device.type or (device.index is not None and buf.rows.device.index != device.index):
            self.buffers = EvalBuffers(n_rows, device)
            self.steps = self._new_steps()
        else:
            buf.reset()
        self.model.eval()

    def _step(self, meta, *tensors):
        pattern, graph = self.dataset_cls.graphs_from_arrays(meta, tensors)
        n = 2 * self.dataset_cls.ARRAYS_PER_GRAPH
        counts = tensors[n]
        subs = tensors[-2:] if self.match_weights else ()       # (sub_flat at the dataset's capacity, sample_ptr)
        weights = tensors[n + 1] if len(tensors) == n + 2 + len(subs) else None     # a padded batch: 0 for the inert pairs
        model = self.model
        # no optimizer step here that could drop a batch which does not fit a gate capacity: every edge row as it stands
        cap, model.gate_capacity = getattr(model, "gate_capacity", None), None
        try:
            with torch.no_grad():
                out = model(pattern, graph)
                heads = [None, None]
                if subs:
                    found = self._subiso(meta, pattern, graph, subs)
                    for k, (w, pk, refine) in enumerate(zip(found, ("pred_v", "pred_e"), (model.refine_node_weights, model.refine_edge_weights))):
                        if w is not None and out[pk] is not None:
                            heads[k] = (out[pk], refine(w))
                self.heads_seen = [h is not None for h in heads]       # a property of the model, the same for every batch
                return eval_terms(out["pred_c"], counts, heads, self.buffers, pair_weights=weights)
        finally:
            model.gate_capacity = cap

    def __call__(self, dataset, indices, device):
        """One batch of the pass ``begin`` started; returns the sums (device, still growing)."""
        if self.buffers is None:
            raise RuntimeError("GraphedEvalStep: begin(n_rows, device) starts a pass")
        if self.model.training:
            self.model.eval()
        meta, tensors = dataset.batch_arrays(indices, device, **self._batch_kwargs(dataset, indices))
        if tensors[0].is_cuda:
            return self.steps(meta, *tensors)
        return self._step(meta, *tensors)

    def results(self, expected, collect=True):
        """The pass's outcome, read once: ``(sums [4] float64 on the host, rows)`` with ``rows`` = ``[4, expected]`` fp32 on the
        host (``EvalBuffers.rows``' layout) or None without ``collect``.  ``RuntimeError`` when the cursor is not
        ``expected`` or the overflow word is set."""
        buf = self.buffers
        state = torch.cat([buf.sums, buf.cursor.double(), buf.overflow.double()]).cpu()       # 48 bytes: one read
        if int(state[5]) != 0:
            raise RuntimeError("GraphedEvalStep: the pass wrote %d rows into result buffers of %d" % (int(state[4]), buf.cap))
        if int(state[4]) != int(expected) or int(state[0]) != int(expected):
            raise RuntimeError("GraphedEvalStep: %d result rows (%d pairs counted) for a dataset of %d pairs"
                               % (int(state[4]), int(state[0]), int(expected)))
        return state[:4], (buf.rows[:, :int(expected)].cpu() if collect else None)


def _evaluate_recorded(step, dataset, batch_size, device, eval_metric, match_weights, collect):
    """``evaluate_epoch`` through a ``GraphedEvalStep``."""
    if isinstance(match_weights, str):
        match_weights = match_weights.split(",")
    if match_weights is not None and tuple(w for w in ("node", "edge") if w in match_weights) != step.match_weights:
        raise ValueError("evaluate_epoch(graph=step): the step was built with match_weights=%r" % (step.match_weights,))
    if step.match_weights and not all(x.get("subisomorphisms") is not None for x in dataset.samples):
        raise ValueError("evaluate_epoch(graph=step): the step computes matching errors and a sample has no subisomorphisms")
    model = step.model
    cap, model.gate_capacity = getattr(model, "gate_capacity", None), None
    try:
        with step.on_stream(device):
            step.begin(len(dataset), device)
            for i in range(0, len(dataset), batch_size):
                step(dataset, np.arange(i, min(i + batch_size, len(dataset))), device)
            sums, rows = step.results(len(dataset), collect)      # the pass's only reads: under on_stream (dp.StepGraph)
    finally:
        model.gate_capacity = cap
    count = max(float(sums[0]), 1.0)
    res = {"MAE": float(sums[1]) / count, "MSE": float(sums[2]) / count}
    res["eval_metric"] = float(sums[{"MAE": 1, "MSE": 2, "SMSE": 3}[eval_metric]]) / count
    res["RMSE"] = res["MSE"] ** 0.5
    if rows is not None:
        res["pred"], res["counts"] = rows[0].clone(), rows[1].clone()
        res["AUC"] = binary_auc(res["counts"] > 0, res["pred"] > 0)
        for k, (key, mean) in enumerate((("NED", "MNED"), ("EED", "MEED"))):
            if step.heads_seen[k]:
                res[key] = rows[2 + k].clone()
                res[mean] = float(res[key].mean())
    return res


@torch.no_grad()
def evaluate_epoch(model, dataset, batch_size, device, eval_metric="MAE", match_weights=None, graph=None, collect=True):
    """train.py:847-1061: MAE / MSE / RMSE of ``relu(pred_c)``, the AUC of ``relu(pred_c) > 0`` against ``counts > 0``
    and the predictions themselves.  With ``match_weights`` ("node", "edge" or both; every sample needs its
    ``subisomorphisms``) and a model whose heads return weights, also the matching half: per pair ``NED`` / ``EED`` = the
    sum of ``|relu(pred) - weights|`` over the whole padded row (train.py:952,967 mask nothing there), their means
    ``MNED`` / ``MEED``, and flat ``pred_v`` / ``pred_e`` / ``node_weights`` / ``edge_weights``: every pair's live
    positions back to back.
    ``graph``: a ``GraphedEvalStep`` built for ``model`` -- every batch then goes through ``dataset.batch_arrays`` and the step
    (one HIP graph replay per recorded batch shape), nothing is read per batch, and the scalars come from the step's fp64
    sums; the matching half is the step's own ``match_weights``.  With ``collect`` (the default) ``pred``, ``counts`` and
    ``NED`` / ``EED`` arrive in ONE copy at the end of the pass and ``AUC`` / ``MNED`` / ``MEED`` are computed from them;
    ``collect=False`` returns ``MAE`` / ``MSE`` / ``RMSE`` / ``eval_metric`` only, from one read of a few numbers.  The flat
    live-position lists (``pred_v``, ``pred_e``, ``node_weights``, ``edge_weights``) are NOT produced on this route: their
    lengths depend on the data (``evaluate_run``, which writes them, evaluates eagerly).  A pass whose row count does not
    come out at ``len(dataset)`` raises ``RuntimeError``."""
    if graph is not None:
        if graph.model is not model:
            raise ValueError("evaluate_epoch(graph=step): the step was built for another model")
        return _evaluate_recorded(graph, dataset, batch_size, device, eval_metric, match_weights, collect)
    model.eval()
    preds, targets = [], []
    if isinstance(match_weights, str):
        match_weights = match_weights.split(",")
    want = tuple(w for w in ("node", "edge") if w in (match_weights or ()))
    if want and not all(x.get("subisomorphisms") is not None for x in dataset.samples):
        want = ()
    match = {k: [] for k in ("NED", "EED", "pred_v", "pred_e", "node_weights", "edge_weights")}
    # no optimizer step here that could drop a batch which does not fit a gate capacity: every edge row as it stands
    cap, model.gate_capacity = getattr(model, "gate_capacity", None), None
    try:
        for i in range(0, len(dataset), batch_size):
            idx = np.arange(i, min(i + batch_size, len(dataset)))
            pattern, graph, counts, weights = dataset.batchify(idx, device, return_weights=want) if want else dataset.batchify(idx, device)
            out = model(pattern, graph)
            preds.append(F.relu(out["pred_c"]))
            targets.append(counts)
            for w, pk, mk, ek, wk in ((weights[0], "pred_v", "g_v_mask", "NED", "node_weights"),
                                      (weights[1], "pred_e", "g_e_mask", "EED", "edge_weights")):
                if w is None or out[pk] is None:
                    continue
                w = (model.refine_node_weights if pk == "pred_v" else model.refine_edge_weights)(w.float())
                live = out[mk].reshape(w.shape).bool()
                match[wk].append(w[live])                     # row-major: pair after pair, each pair's live positions
                match[pk].append(out[pk][live])
                match[ek].append((F.relu(out[pk]) - w).abs().sum(dim=1))
    finally:
        model.gate_capacity = cap
    pred, target = torch.cat(preds), torch.cat(targets)
    res = {"MAE": float(F.l1_loss(pred, target)), "MSE": float(F.mse_loss(pred, target)),
           "eval_metric": float(_CRIT[eval_metric](pred, target)), "pred": pred.view(-1).cpu(), "counts": target.view(-1).cpu()}
    res["RMSE"] = res["MSE"] ** 0.5
    res["AUC"] = binary_auc(target > 0, pred > 0)
    for k, parts in match.items():
        if parts:
            res[k] = torch.cat(parts).cpu()
    for mean, k in (("MNED", "NED"), ("MEED", "EED")):
        if k in res:
            res[mean] = float(res[k].mean())
    return res


def evaluate_run(save_dir, datasets, device, batch_size=None, eval_metric=None, epoch=None, stamp="", match_weights=None):
    """``evaluate.py`` (lines 60-245) for a run directory written by ``fit`` (or by the reference's ``train.py``):
    ``config.json`` -> ``build_model``; the dev-best epoch of ``log.txt`` (``utils/log.py:60-76``) -> its ``epoch%d.pt``
    (strict load); every split of ``datasets`` (name -> PairDataset) evaluated and written to
    ``eval_<split>_results_<stamp>.json`` with the reference's result layout (``data`` / ``prediction`` / ``error``);
    one "best" line per split appended to ``log.txt``.  ``match_weights``: the run's own (``config.json``) unless given;
    with it the result file also carries ``node_weights`` / ``edge_weights`` (``data``), ``pred_v`` / ``pred_e``
    (``prediction``) and ``NED`` / ``EED`` / ``MNED`` / ``MEED`` (``error``) where the model and the split have them, and
    always ``RMSE`` / ``AUC``.  Returns ``{split: {"MAE", "MSE", "eval_metric"}}``."""
    import json
    from . import dataio
    from .basemodel import build_model
    config = dataio.load_config(os.path.join(save_dir, "config.json"))
    metric = eval_metric or config.get("eval_metric", "MAE")
    if match_weights is None:
        match_weights = config.get("match_weights", None)
    if isinstance(match_weights, str):
        match_weights = [w for w in match_weights.split(",") if w in ("node", "edge")]
    if epoch is None:
        best = dataio.get_best_epochs(os.path.join(save_dir, "log.txt"))
        epoch = best["eval-" + metric]["dev"][0]
    model = build_model(config).to(device)
    model.load_state_dict(torch.load(dataio.checkpoint_path(save_dir, epoch), map_location=device), strict=True)
    out = {}
    with open(os.path.join(save_dir, "log.txt"), "a") as log:
        for split, ds in datasets.items():
            res = evaluate_epoch(model, ds, batch_size or config.get("eval_batch_size", 64), device, eval_metric=metric,
                                 match_weights=match_weights)
            out[split] = {k: res[k] for k in ("MAE", "MSE", "eval_metric")}
            ids = [x.get("id", str(i)) for i, x in enumerate(ds.samples)]
            with open(os.path.join(save_dir, "eval_%s_results_%s.json" % (split, stamp)), "w") as f:
                doc = {"data": {"id": ids, "counts": res["counts"].tolist()}, "prediction": {"pred_c": res["pred"].tolist()},
                       "error": {"MAE": res["MAE"], "MSE": res["MSE"], "RMSE": res["RMSE"], "AUC": res["AUC"]}}
                for part, keys in (("data", ("node_weights", "edge_weights")), ("prediction", ("pred_v", "pred_e")),
                                   ("error", ("NED", "EED", "MNED", "MEED"))):
                    for k in keys:
                        if k in res:
                            doc[part][k] = res[k].tolist() if torch.is_tensor(res[k]) else res[k]
                json.dump(doc, f)
            log.write(dataio.best_line(split, epoch, epoch, **{"eval-" + metric: "%.3f" % res["eval_metric"]}) + "\n")
    return out


def validate_samples(samples):
    """Host-side check of a dataset, once: every edge endpoint of every pattern / graph inside ``[0, number_of_nodes)``
    (the device index builds only flag such edges in a status word that the training loop does not read back) and the
    reversed-edge flags, when present, one per edge.  Raises ``ValueError`` naming the first offending sample."""
    samples = getattr(samples, "samples", samples)
    for i, x in enumerate(samples):
        for key in ("pattern", "graph"):
            g = x[key]
            if isinstance(g, dict):                          # PairDataset's stored form: numpy arrays
                n, src, dst, rev = int(g["num_nodes"]), np.asarray(g["src"]), np.asarray(g["dst"]), g.get("rev")
            else:                                            # a graph object (BatchedGraph / DGL surface)
                n = int(g.number_of_nodes())
                src, dst = (t.detach().cpu().numpy() for t in g.all_edges(form="uv", order="eid"))
                rev = g.edata.get("is_reversed") if hasattr(g, "edata") else None
            if len(src) != len(dst):
                raise ValueError("sample %d (%s): %s has %d sources for %d destinations" % (i, x.get("id", "?"), key, len(src), len(dst)))
            if len(src) and (min(src.min(), dst.min()) < 0 or max(src.max(), dst.max()) >= n):
                raise ValueError("sample %d (%s): %s has an edge endpoint outside [0, %d)" % (i, x.get("id", "?"), key, n))
            if rev is not None and len(rev) != len(src):
                raise ValueError("sample %d (%s): %s has %d is_reversed flags for %d edges" % (i, x.get("id", "?"), key, len(rev), len(src)))
    return len(samples)


def fit(model, optimizer, train_set, dev_set, epochs, batch_size, device, save_dir=None, config=None, sync=None,
        eval_metric="MAE", seed=0, eval_graph=False, **train_kw):
    """The epoch loop of ``train.py:1296-1380`` reduced to its contract: per epoch one shuffled training
    pass and one dev evaluation; with ``save_dir`` the run directory the reference's tooling expects --
    ``config.json``, ``epoch%d.pt`` (state dict of every epoch), ``log.txt`` whose "best" lines
    (``utils/log.py:50-57``) ``dataio.get_best_epochs`` reads back.  Returns the per-epoch history.
    ``graph=True`` (with ``FlatAdamW(capturable=True)``, one rank): training steps whose batch shape repeats are
    recorded once and replayed as one HIP graph (``GraphedTrainStep``).
    ``eval_graph=True``: when ``graph`` resolved to a recorded training step, the dev pass is recorded too
    (``GraphedEvalStep`` on the training recordings' side stream, ``evaluate_epoch(graph=..., collect=False)``: one read of
    a few numbers per epoch); without a recorded training step the dev pass runs eagerly, as ``graph=True`` falls back.
    ``gate_compact=True`` (or a margin, e.g. 1.25): training forward passes run the rep-net on the target edges the filter
    gate keeps (``model.set_gate_capacity``; capacity = the largest kept count over the training batches in their stored order x the margin; batches are shuffled in training, so a batch can still exceed it: such steps are dropped, counted, and a warning is raised above 1 % of the steps).
    A batch that keeps more than that raises a device flag and the optimizer drops its step (``FlatAdamW.set_veto``, as a
    loss-scaling optimizer drops an overflowed step); the history counts them (``dropped_steps``).  Evaluation passes run
    on every edge row.  Single rank only (the veto is rank-local: refused with a multi-rank ``sync``)."""
    from . import dataio
    from .tuning import enable_tuned_gemms
    if train_kw.get("gate_compact") and getattr(sync, "world", 1) > 1:
        # the overflow flag and the capacity are rank-local: a rank whose batch overflowed would still feed its (wrong)
        # gradients to the all-reduce and only IT would drop the step -- the replicas would drift apart for good
        raise ValueError("fit(gate_compact=...) is a single-rank option: the overflow veto is rank-local (world size %d)" % sync.world)
    validate_samples(train_set)
    validate_samples(dev_set)
    enable_tuned_gemms()      # the layer's [rows, 128] x [128, 128..384] products with the solutions picked for MI355X
    sync = sync or FlatGradSync(model)
    if train_kw.get("graph") is True:       # graph=True: replay recorded steps where the setup allows it, else eager
        ok = getattr(optimizer, "capturable", False) and getattr(sync, "world", 1) == 1
        # the regulariser is part of the recording when it can be on at ANY step of the run: a positive constant, or a
        # schedule's value (a number or an annealing spec string in its config: on unless it is the constant 0)
        reg = train_kw.get("rep_reg_w", 0.0)
        sched = train_kw.get("schedule")
        if sched is not None:
            reg = sched.config.get("rep_reg_w", 0.0)
        on = lambda v: (isinstance(v, str) and v.strip() not in ("", "0", "0.0")) or (not isinstance(v, str) and float(v) > 0)
        with_reg = on(reg)
        # the matching terms likewise: recorded when one of their coefficients can be non-zero at any step
        coefs = [(sched.config if sched is not None else train_kw).get(k, 0.0) for k in ("match_loss_w", "match_reg_w")]
        match = train_kw.get("match_weights", ("node", "edge")) if any(on(c) for c in coefs) else ()
        train_kw["graph"] = GraphedTrainStep(model, optimizer, sync, bp_loss=train_kw.get("bp_loss", "MSE"), eval_metric=eval_metric,
                                             max_grad_norm=train_kw.get("max_grad_norm", 8.0), with_rep_reg=with_reg,
                                             match_weights=match) if ok else None
    elif not train_kw.get("graph"):
        train_kw.pop("graph", None)
    rng = np.random.default_rng(seed)
    compact = train_kw.pop("gate_compact", False)
    if compact and hasattr(model, "calibrate_gate_capacity") and hasattr(optimizer, "set_veto"):
        margin, cap = (1.15 if compact is True else float(compact)), 0
        with torch.enable_grad():
            for i in range(0, len(train_set), batch_size):     # every training batch once: the gates only (no rep-net pass)
                pattern, graph_b = train_set.batchify(np.arange(i, min(i + batch_size, len(train_set))), device)[:2]
                cap = max(cap, model.calibrate_gate_capacity(pattern, graph_b, margin=margin, multiple=256) or 0)
        model.set_gate_capacity(cap or None)
        # (bit 0: a batch kept more edges than the capacity; bit 1: a graph without nodes was dealt padding edges -- both make
        # the step's gradients unusable, both drop it)
        optimizer.set_veto(model.compaction_word if cap else None, mask=3)
    log = None
    if save_dir is not None:
        os.makedirs(save_dir, exist_ok=True)
        if config is not None:
            dataio.save_config(config, os.path.join(save_dir, "config.json"))
        log = open(os.path.join(save_dir, "log.txt"), "w")
    best, history = (float("inf"), -1), []
    import gc
    gc.collect()
    gc.freeze()      # model / dataset / optimizer objects: out of the cyclic collector's way for the whole run
    import contextlib
    graphed = train_kw.get("graph")
    # recorded steps: the whole loop (evaluation, checkpoint copies) on the recordings' side stream -- see dp.StepGraph
    stream_ctx = graphed.steps.on_stream() if graphed else contextlib.nullcontext()
    dev_kw = {}
    if eval_graph and isinstance(graphed, GraphedTrainStep):
        dev_kw = {"graph": GraphedEvalStep(model, eval_metric=eval_metric, steps_like=graphed.steps), "collect": False}
    try:
      with stream_ctx:
        for epoch in range(epochs):
            tr = train_epoch(model, optimizer, train_set, batch_size, device, sync=sync, eval_metric=eval_metric,
                             order=rng.permutation(len(train_set)), **dict(train_kw, epoch=epoch))
            dev = evaluate_epoch(model, dev_set, batch_size, device, eval_metric=eval_metric, **dev_kw)
            history.append({"epoch": epoch, "train": tr, "dev": {k: dev[k] for k in ("MAE", "MSE", "eval_metric")}})
            if getattr(model, "gate_capacity", None):
                history[-1]["dropped_steps"] = model.compaction_dropped_steps()       # cumulative (one host sync per epoch)
                steps_so_far = (epoch + 1) * max(1, -(-len(train_set) // batch_size))
                if history[-1]["dropped_steps"] > 0.01 * steps_so_far:
                    import warnings
                    warnings.warn("fit(gate_compact): %d of %d optimizer steps were dropped (batches that kept more edges than the "
                                  "capacity): raise the margin" % (history[-1]["dropped_steps"], steps_so_far))
            if save_dir is not None:
                torch.save(model.state_dict(), dataio.checkpoint_path(save_dir, epoch))
            if dev["eval_metric"] < best[0]:
                best = (dev["eval_metric"], epoch)
            if log is not None:
                log.write("data_type: train\tepoch: %03d/%03d\tbp_loss: %.5f\teval-%s: %.5f\n"
                          % (epoch, epochs, tr["bp_loss"], eval_metric, tr["eval_metric"]))
                log.write("data_type: dev\tepoch: %03d/%03d\teval-%s: %.5f\n" % (epoch, epochs, eval_metric, dev["eval_metric"]))
                log.write(dataio.best_line("dev", best[1], epochs, **{"eval-" + eval_metric: "%.5f" % best[0]}) + "\n")
                log.flush()
    finally:
        gc.unfreeze()
        if log is not None:
            log.close()
    return history
