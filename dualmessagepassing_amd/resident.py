"""A ``PairDataset`` that lives on the device: every batch is assembled there by one launch from one small upload.

``PairDataset.batch_arrays`` builds a batch on the host -- list comprehensions over the samples, eighteen concatenations, the
inert padding graphs as Python dicts -- and uploads its twenty-odd arrays one by one.  Nothing of that changes between
epochs.  ``PairDataset.resident(device)`` uploads the dataset once (``resident_store``: the samples' arrays back to back in
narrow types); a batch is then ``resident_plan`` -- vectorised numpy over the per-sample sizes, one int64 array -- one upload
of that plan and one launch of ``dmp_collate_resident`` (csrc/dmp_resident.hip) that writes every tensor ``batch_arrays``
returns, with the same values, shapes and dtypes.
"""
import numpy as np
import torch

from . import _abi, _lib
from .harness import PairDataset

SIDES = ("pattern", "graph")
_NARROW = (("src", np.int32), ("dst", np.int32), ("vlabel", np.int32), ("elabel", np.int32), ("eid", np.int32), ("rev", np.uint8))
PLAN_HEAD = 4            # the plan's first entries: the inert labels (pattern node, pattern edge, graph node, graph edge)


def _narrow(a, dtype, what):
    a = np.asarray(a)
    if dtype is np.uint8:                       # the reversed flags: bool, or integers that are 0 / 1
        if a.dtype != np.bool_ and a.size and (a.min() < 0 or a.max() > 1):
            raise ValueError("resident store: %s holds a value that is no 0 / 1 flag" % what)
        return a.astype(np.uint8)
    a = a.astype(np.int64)
    info = np.iinfo(dtype)
    if a.size and (a.min() < info.min or a.max() > info.max):
        raise ValueError("resident store: %s holds %d, outside its %s storage" % (what, a.min() if a.min() < info.min else a.max(), np.dtype(dtype).name))
    return a.astype(dtype)


def _cat(parts, dtype):
    return np.concatenate(parts) if parts else np.zeros(0, dtype)


def _ptr(sizes):
    out = np.zeros(len(sizes) + 1, np.int64)
    np.cumsum(sizes, out=out[1:])
    return out


def resident_store(samples):
    """The host image of the store, pure numpy: per side ``src`` / ``dst`` / ``vlabel`` / ``elabel`` / ``eid`` (int32) and ``rev``
    (uint8) of every sample back to back with ``node_ptr`` / ``edge_ptr`` [S + 1] (int64); ``counts`` [S] float32, converted as
    ``torch.tensor(list_of_ints, dtype=float32)`` converts; ``subs`` (int32), the samples' ``subisomorphisms`` rows flattened
    back to back, and ``sub_ptr`` [S + 1].  ``sizes``: the per-sample node / edge / row-element counts the plans are made of.
    A value that does not fit its storage type is a ``ValueError``."""
    store, sizes = {}, {}
    for key in SIDES:
        gs = [x[key] for x in samples]
        nodes = np.array([int(g["num_nodes"]) for g in gs], np.int64)
        edges = np.array([len(g["src"]) for g in gs], np.int64)
        side = {}
        for name, dtype in _NARROW:
            side[name] = _narrow(_cat([np.asarray(g[name]).reshape(-1) for g in gs], np.int64), dtype, "%s.%s" % (key, name))
            want = nodes.sum() if name == "vlabel" else edges.sum()
            if side[name].size != want:
                raise ValueError("resident store: %s.%s has %d entries for %d %s" % (key, name, side[name].size, want,
                                                                                     "nodes" if name == "vlabel" else "edges"))
        side["node_ptr"], side["edge_ptr"] = _ptr(nodes), _ptr(edges)
        store[key], sizes[key] = side, (nodes, edges)
    rows = [np.asarray(x["subisomorphisms"], np.int64).reshape(-1) for x in samples]
    sizes["subs"] = np.array([r.size for r in rows], np.int64)
    store["subs"] = _narrow(_cat(rows, np.int64), np.int32, "subisomorphisms")
    store["sub_ptr"] = _ptr(sizes["subs"])
    store["counts"] = torch.tensor([x["counts"] for x in samples], dtype=torch.float32).numpy()
    return store, sizes


def resident_plan(sizes, indices, pad=None, subs=None, n_vlabels=1, n_elabels=1):
    """The plan of one batch, pure numpy and without a loop over the samples: ``(meta, plan, info)``.  ``sizes``:
    ``resident_store``'s; ``indices`` / ``pad`` / ``subs``: ``PairDataset.batch_arrays``'; ``n_vlabels`` / ``n_elabels``: the
    dataset's vocabulary sizes (an inert graph takes label 1 where there is one).  ``meta`` is ``batch_arrays``' own; the
    capacity level, the dealing of nodes and edges to the inert pairs (even split, the remainder to the first ones) and every
    ``ValueError`` are ``batch_arrays``' too.  ``plan`` (int64, the layout ``dmp_collate_resident`` reads): the four inert
    labels, the sample of every slot (-1: inert), then the exclusive prefix sums [slots + 1] of pattern nodes, pattern edges,
    graph nodes, graph edges and subisomorphism elements.  ``info``: ``slots``, ``real``, the four totals, ``sub_total``."""
    S = len(sizes["subs"])
    idx = np.asarray(indices, np.int64).reshape(-1)
    if idx.size and (idx.min() < -S or idx.max() >= S):
        raise IndexError("batch index outside the dataset's %d samples" % S)
    idx = np.where(idx < 0, idx + S, idx)
    real, extra, level = len(idx), 0, 0
    per = {key: (sizes[key][0][idx], sizes[key][1][idx]) for key in SIDES}
    tot = {key: (int(per[key][0].sum()), int(per[key][1].sum())) for key in SIDES}
    if pad is not None:
        B, K = pad["batch"], pad["levels"]
        if real > B:
            raise ValueError("batch_arrays(pad=...): more pairs than the padding was laid out for")
        extra = 2 * B - real
        caps = lambda key, k: (-(-B * pad[key][0] * k // K) + B, -(-B * pad[key][1] * k // K) + B)
        fits = lambda k: all(tot[key][0] + extra <= caps(key, k)[0] and tot[key][1] + extra <= caps(key, k)[1] for key in SIDES)
        level = next((k for k in range(1, K + 1) if fits(k)), None)
        if level is None:
            raise ValueError("batch_arrays(pad=...): the batch does not fit %d graphs of the dataset's largest size" % B)
    slots = real + extra
    plan = np.zeros(PLAN_HEAD + slots + 5 * (slots + 1), np.int64)
    plan[PLAN_HEAD:PLAN_HEAD + real] = idx
    plan[PLAN_HEAD + real:PLAN_HEAD + slots] = -1
    prefix = plan[PLAN_HEAD + slots:].reshape(5, slots + 1)
    meta, deal = [], np.arange(extra)
    for side, key in enumerate(SIDES):
        nodes, edges = per[key]
        if extra:
            cn, ce = caps(key, level)
            n_pad, e_pad = cn - tot[key][0], ce - tot[key][1]
            if n_pad < extra or e_pad < extra:
                raise ValueError("batch_arrays(pad=...): the batch does not fit its capacity level")
            if -(-n_pad // extra) > pad[key][0] or -(-e_pad // extra) > pad[key][1]:      # the first inert graph is the largest
                raise ValueError("batch_arrays(pad=...): an inert graph would exceed the dataset's largest graph (a batch of empty graphs?)")
            nodes = np.concatenate([nodes, n_pad // extra + (deal < n_pad % extra)])
            edges = np.concatenate([edges, e_pad // extra + (deal < e_pad % extra)])
            if key == "graph":
                plan[2], plan[3] = (1 if n_vlabels > 1 else 0), (1 if n_elabels > 1 else 0)
        np.cumsum(nodes, out=prefix[2 * side, 1:])
        np.cumsum(edges, out=prefix[2 * side + 1, 1:])
        if pad is not None:
            meta.append((int(prefix[2 * side, -1]), int(prefix[2 * side + 1, -1]), int(pad[key][0]), int(pad[key][1])))
        else:
            meta.append((int(prefix[2 * side, -1]), int(prefix[2 * side + 1, -1]), int(nodes.max(initial=0)), int(edges.max(initial=0))))
    np.cumsum(sizes["subs"][idx], out=prefix[4, 1:real + 1])
    prefix[4, real + 1:] = prefix[4, real]
    if subs is not None and prefix[4, -1] > int(subs):
        raise ValueError("batch_arrays(subs=%d): the batch's subisomorphism rows take %d elements" % (int(subs), prefix[4, -1]))
    info = {"slots": slots, "real": real, "nodes": (meta[0][0], meta[1][0]), "edges": (meta[0][1], meta[1][1]), "sub_total": int(prefix[4, -1])}
    return tuple(meta), plan, info


class ResidentPairs(PairDataset):
    """``PairDataset.resident(device)``: the dataset's view whose batches are assembled on ``device``.  ``samples``, ``shape``,
    ``pad_buckets``, ``sub_capacity``, ``model_config`` and ``batchify`` are the source's (``batchify`` runs through this
    ``batch_arrays``); ``subset`` gives the subset's own resident view.  ``batch_arrays`` returns what the source's returns, bit
    for bit, from one upload (the plan) and one launch.  A batch above ``DMP_RESIDENT_MAX_SLOTS`` pairs, an empty batch and
    a request for another device go through the source's host path."""

    def __init__(self, source, device):
        self.samples, self.shape = source.samples, source.shape
        host, self.sizes = resident_store(self.samples)            # raises before anything is uploaded
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.DmpError("PairDataset.resident: the store lives on an AMD GPU (got %s)" % (device,))
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        # The store's tensors belong to the CURRENT stream, as every other tensor of a run does (the caching allocator knows a
        # block by the stream it was allocated on).  Only the copies into them run on a stream of their own: they are sizeable
        # blocking copies, which must not go over the legacy default stream between two recordings (dp.StepGraph).
        flat = [(key, name, np.ascontiguousarray(a)) for key in SIDES for name, a in host[key].items()]
        flat += [(None, name, np.ascontiguousarray(host[name])) for name in ("counts", "subs", "sub_ptr")]
        with torch.cuda.device(device):
            made = [torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device=device) for _, _, a in flat]
            cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                for t, (_, _, a) in zip(made, flat):
                    t.copy_(torch.from_numpy(a))
            cur.wait_stream(side)
        self.store = {key: {} for key in SIDES}
        for t, (key, name, _) in zip(made, flat):
            (self.store if key is None else self.store[key])[name] = t
        self._sides = (_abi.dmp_resident_side * 2)()
        for side, key in enumerate(SIDES):
            for name, t in self.store[key].items():
                setattr(self._sides[side], name, _lib.ptr(t))
        self.uploads = 0                                            # plans sent so far: one per device-built batch

    @property
    def nbytes(self):
        """Device bytes of the store."""
        flat = [t for key in SIDES for t in self.store[key].values()] + [self.store[k] for k in ("counts", "subs", "sub_ptr")]
        return int(sum(t.numel() * t.element_size() for t in flat))

    def subset(self, indices):
        return PairDataset.subset(self, indices).resident(self.device)

    def resident(self, device):
        return self if torch.device(device) in (self.device, torch.device("cuda")) else PairDataset.resident(self, device)

    def plan(self, indices, pad=None, subs=None):
        """``resident_plan`` of a batch of this dataset."""
        return resident_plan(self.sizes, indices, pad=pad, subs=subs, n_vlabels=self.shape.get("n_vlabels", 1),
                             n_elabels=self.shape.get("n_elabels", 1))

    def alloc_outputs(self, info, padded, subs=None):
        """Uninitialised output tensors of a batch in ``batch_arrays``' order (the launch writes every element)."""
        dev, P = self.device, info["slots"]
        i64 = lambda n: torch.empty(n, dtype=torch.int64, device=dev)
        out = []
        for side in (0, 1):
            N, E = info["nodes"][side], info["edges"][side]
            out += [i64(E), i64(E), i64(P), i64(P), i64(N), i64(N), i64(E), i64(E), torch.empty(E, dtype=torch.bool, device=dev)]
        out.append(torch.empty((P, 1), dtype=torch.float32, device=dev))
        if padded:
            out.append(torch.empty((P, 1), dtype=torch.float32, device=dev))
        if subs is not None:
            out += [i64(int(subs)), i64(P + 1)]
        return out

    def launch(self, plan, info, out, padded, subs=None):
        """``dmp_collate_resident``: ``plan`` (the device copy of ``resident_plan``'s array) -> the tensors of ``out``
        (``alloc_outputs``' layout).  Raises ``DmpError`` (DMP_ERR_UNSUPPORTED above the slot limit)."""
        lib = _lib.load()
        _lib.require_gpu(plan, *out)
        if plan.dtype != torch.int64 or plan.numel() != PLAN_HEAD + 6 * info["slots"] + 5 or not plan.is_contiguous():
            raise _lib.DmpError("collate_resident: the plan does not have the layout of %d slots" % info["slots"])
        if max(info["nodes"] + info["edges"]) >= 2 ** 31:
            raise _lib.DmpError("collate_resident: a batch of 2^31 nodes or edges")
        batch = (_abi.dmp_resident_batch * 2)()
        n = self.ARRAYS_PER_GRAPH
        for side in (0, 1):
            src, dst, nn_, ne_, nid, vlabel, eid, elabel, rev = out[side * n:(side + 1) * n]
            b = batch[side]
            b.src, b.dst, b.num_nodes, b.num_edges, b.nid = _lib.ptr(src), _lib.ptr(dst), _lib.ptr(nn_), _lib.ptr(ne_), _lib.ptr(nid)
            b.vlabel, b.eid, b.elabel, b.rev = _lib.ptr(vlabel), _lib.ptr(eid), _lib.ptr(elabel), _lib.ptr(rev)
        tail = out[2 * n + 1 + (1 if padded else 0):]
        sub_flat, sample_ptr = tail if subs is not None else (None, None)
        moved = 16 * sum(info["nodes"]) + 37 * sum(info["edges"]) + (8 * int(subs) if subs is not None else 0)
        with _lib.timed("collate_resident[slots=%d]", (info["slots"],), moved):
            _lib.check(lib.dmp_collate_resident(self._sides, _lib.ptr(self.store["counts"]), _lib.ptr(self.store["subs"]),
                                                _lib.ptr(self.store["sub_ptr"]), _lib.ptr(plan), info["slots"], info["real"], batch,
                                                _lib.ptr(out[2 * n]), _lib.ptr(out[2 * n + 1]) if padded else None, _lib.ptr(sub_flat),
                                                int(subs) if subs is not None else 0, info["sub_total"], _lib.ptr(sample_ptr),
                                                _lib.stream_ptr()), "dmp_collate_resident")

    def _here(self, device):
        device = torch.device(device)
        return device.type == "cuda" and (self.device.index if device.index is None else device.index) == self.device.index

    def batch_arrays(self, indices, device, pad=None, subs=None):
        """``PairDataset.batch_arrays``, built on the device: the plan (host, numpy; every ``ValueError`` of the host path is
        raised here, before anything is launched), its upload on the current stream, one launch."""
        if len(indices) == 0 or not self._here(device):
            return PairDataset.batch_arrays(self, indices, device, pad=pad, subs=subs)
        meta, plan, info = self.plan(indices, pad=pad, subs=subs)
        if info["slots"] > _abi.DMP_RESIDENT_MAX_SLOTS:
            return PairDataset.batch_arrays(self, indices, device, pad=pad, subs=subs)
        with torch.cuda.device(self.device):
            # a pageable copy, as the host path's uploads are: it has left ``plan`` when ``.to`` returns, so no staging buffer
            # is rewritten under a copy in flight (dp.StepGraph: keep sizeable blocking copies off the default stream --
            # fit(graph=True) runs the loop on the recordings' side stream; a plan of 128 slots is 6 KiB)
            plan_dev = torch.from_numpy(plan).to(self.device)
            self.uploads += 1
            out = self.alloc_outputs(info, pad is not None, subs)
            self.launch(plan_dev, info, out, pad is not None, subs)
        return meta, out
