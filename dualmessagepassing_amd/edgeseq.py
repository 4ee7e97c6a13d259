"""Edge-sequence input of the sequence rep-nets (CNN): every graph as a sorted sequence of 5-tuples ``(u, v, ul, el, vl)``
(``SubgraphCountingMatching/dataset.py:111-770, 885-1052``).

Per sample (host, numpy, once when the dataset is prepared):

* ``from_graph``          -- codes ``(nid[u], nid[v], nl[u], el[e], nl[v])`` sorted by ``(u, v, ul, el, vl)``;
* ``add_reversed_edges``  -- ``(v, u, vl, el + max_ngel, ul)`` appended with ``is_reversed = 1``, the whole sequence then
                             ordered by ``(u, v, el)`` (tuples equal in those three keys are equal in all five);
* ``edge_weights``        -- ``compute_edgeseq_subisoweights`` (dataset.py:69-108) on the forward sequences, and
                             ``map_reversed_weights`` -- the forward-to-reversed mapping of ``add_reversed_edges``.

Per batch (device): ``EdgeSeq.batch`` uploads the concatenated codes once and scatters them into pre-padded ``[B, L]``
rows (live tuples at the end of each row), with index ops only.  ``in_degrees`` / ``out_degrees`` are the pre-padded
per-node degrees of the reference's ``EdgeSeq`` (its quirks included: a sample without tuples counts its padding row)."""
import numpy as np
import torch as th

from .constants import REVFLAG

KEYS = ("u", "v", "ul", "el", "vl")


def from_graph(src, dst, nid, nlabel, elabel):
    """One graph -> its code ``[E, 5]`` int64 sorted by (u, v, ul, el, vl) (dataset.py:504-522)."""
    src, dst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    nid, nlabel, elabel = np.asarray(nid, np.int64), np.asarray(nlabel, np.int64), np.asarray(elabel, np.int64)
    code = np.stack([nid[src], nid[dst], nlabel[src], elabel, nlabel[dst]], axis=-1).reshape(-1, 5)
    order = np.lexsort(tuple(code[:, k] for k in (4, 3, 2, 1, 0)))
    return np.ascontiguousarray(code[order])


def add_reversed_edges(code, max_nel):
    """dataset.py:930-980 with ``EdgeSeq.add_tuples`` (421-495): (code [2E, 5], is_reversed [2E] bool, order [2E]) where
    ``order`` maps every output position to its row of ``[code | reversed code]``."""
    code = np.asarray(code, np.int64).reshape(-1, 5)
    rev = np.stack([code[:, 1], code[:, 0], code[:, 4], code[:, 3] + max_nel, code[:, 2]], axis=-1)
    both = np.concatenate([code, rev], axis=0)
    flag = np.concatenate([np.zeros(len(code), bool), np.ones(len(code), bool)])
    order = np.lexsort((both[:, 3], both[:, 1], both[:, 0]))
    return np.ascontiguousarray(both[order]), flag[order], order


def _compact_ids(u, v):
    ids = np.unique(np.concatenate([u, v]))
    return np.searchsorted(ids, u), np.searchsorted(ids, v)


def edge_weights(p_code, g_code, subisomorphisms, counts):
    """``calculate_edge_weights`` (dataset.py:903-928): per tuple of ``g_code``, the number of (subisomorphism, pattern
    tuple) pairs that map onto it -- endpoints equal after the subisomorphism and edge labels equal.  Node ids are first
    compacted to the ids the tuples use, as the reference does."""
    g_code = np.asarray(g_code, np.int64).reshape(-1, 5)
    p_code = np.asarray(p_code, np.int64).reshape(-1, 5)
    out = np.zeros(len(g_code), np.int64)
    if counts == 0 or len(g_code) == 0 or len(p_code) == 0:
        return out
    subs = np.asarray(subisomorphisms, np.int64)
    if subs.size == 0:
        return out
    subs = subs.reshape(-1, subs.shape[-1])                  # [number of subisomorphisms, pattern nodes]
    p_u, p_v = _compact_ids(p_code[:, 0], p_code[:, 1])
    g_u, g_v = _compact_ids(g_code[:, 0], g_code[:, 1])
    mod = int(max(p_u.max(), p_v.max(), g_u.max(), g_v.max())) + 1
    g_key = g_u * mod + g_v
    p_key = p_u * mod + p_v
    for key in np.unique(p_key):
        p_els = p_code[p_key == key, 3]
        u, v = divmod(int(key), mod)
        s_key = subs[:, u] * mod + subs[:, v]
        hits = np.searchsorted(np.sort(s_key), g_key, side="right") - np.searchsorted(np.sort(s_key), g_key, side="left")
        same = (g_code[:, 3][:, None] == p_els[None, :]).sum(axis=1)
        out += hits * same
    return out


def map_reversed_weights(g_code_rev, is_reversed, fwd_weights, max_ngel):
    """dataset.py:964-976: the weights of the forward tuples ([E], in forward-sequence order) spread over a sequence
    with its reversed tuples: ``(u, v, el)`` and ``(v, u, el + max_ngel)`` both take the weight of forward ``(u, v, el)``."""
    g_code_rev = np.asarray(g_code_rev, np.int64).reshape(-1, 5)
    is_reversed = np.asarray(is_reversed, bool)
    fwd = g_code_rev[~is_reversed]
    mapping = {}
    for (u, v, el), w in zip(fwd[:, (0, 1, 3)].tolist(), np.asarray(fwd_weights, np.int64).tolist()):
        mapping[(u, v, el)] = w
        mapping[(v, u, el + max_ngel)] = w
    return np.array([mapping[k] for k in map(tuple, g_code_rev[:, (0, 1, 3)].tolist())], np.int64)


class EdgeSeq:
    """A pre-padded batch of edge sequences on one device: ``tdata[k]`` [B, L] for k in (u, v, ul, el, vl) and, with
    reversed tuples, ``is_reversed`` [B, L] bool; ``lens`` [B] (host list and device tensor)."""

    def __init__(self, tdata, lens, num_nodes):
        self.tdata = tdata
        self._lens = [int(x) for x in lens]
        self._num_nodes = [int(x) for x in num_nodes]        # per sample: max node id + 1 (0 without tuples)
        self._len_dev = None

    @property
    def batch_size(self):
        return len(self._lens)

    @property
    def device(self):
        return self.tdata["u"].device

    u = property(lambda self: self.tdata["u"])
    v = property(lambda self: self.tdata["v"])
    ul = property(lambda self: self.tdata["ul"])
    el = property(lambda self: self.tdata["el"])
    vl = property(lambda self: self.tdata["vl"])

    def batch_num_tuples(self):
        if self._len_dev is None:
            self._len_dev = th.tensor(self._lens, dtype=th.long, device=self.device)
        return self._len_dev

    def number_of_tuples(self):
        return sum(self._lens)

    def batch_num_nodes(self):
        """dataset.py:238-247: max(u, v) + 1 over each padded row (1 for a sample without tuples when L > 0)."""
        B = self.batch_size
        if self.number_of_tuples() == 0:
            return th.zeros((B,), dtype=th.long, device=self.device)
        return th.maximum(self.u.max(dim=1)[0], self.v.max(dim=1)[0]) + 1

    def _degrees(self, key):
        """Pre-padded bincount of ``key`` over each live row, at least as long as the other endpoint's padded maximum + 1
        (dataset.py:299-355); a row without tuples counts its whole padding row (the reference's ``x[i, -0:]``)."""
        name = "_deg_" + key
        if name in self.tdata:
            return self.tdata[name]
        B, L = self.u.shape
        dev = self.device
        if self.number_of_tuples() == 0:
            deg = th.zeros((B, 0), dtype=th.long, device=dev)
        else:
            widths = [max(n, 1) for n in self._num_nodes]       # max(bincount length, other max + 1) == max node id + 1
            W = max(widths)
            lens = th.tensor([n if n > 0 else L for n in self._lens], dtype=th.long, device=dev)
            col = th.arange(L, device=dev).view(1, L)
            live = col >= (L - lens).view(B, 1)
            shift = th.tensor([W - w for w in widths], dtype=th.long, device=dev).view(B, 1)
            idx = (th.arange(B, device=dev).view(B, 1) * W + shift + self.tdata[key]).masked_select(live)
            deg = th.zeros(B * W, dtype=th.long, device=dev)
            deg.index_put_((idx,), th.ones_like(idx), accumulate=True)
            deg = deg.view(B, W)
        self.tdata[name] = deg
        return deg

    def in_degrees(self):
        return self._degrees("v")

    def out_degrees(self):
        return self._degrees("u")

    @staticmethod
    def batch(codes, device, flags=None, extra=None):
        """``EdgeSeq.batch(..., pre_pad=True)`` (dataset.py:638-711): ``codes`` a list of [n_i, 5] int64 arrays (sorted
        samples), ``flags`` the matching ``is_reversed`` arrays or None, ``extra`` a list of per-tuple int64 arrays to pad
        the same way (e.g. edge weights).  One upload, then index ops on the device.  Returns (EdgeSeq, padded extras)."""
        lens = np.array([len(c) for c in codes], np.int64)
        B, L = len(codes), int(lens.max(initial=0))
        allc = np.concatenate([np.asarray(c, np.int64).reshape(-1, 5) for c in codes], axis=0) if B else np.zeros((0, 5), np.int64)
        nn_ = [int(c[:, :2].max()) + 1 if len(c) else 0 for c in codes]
        dev = th.device(device)
        row = np.repeat(np.arange(B), lens)
        col = (L - lens)[row] + (np.arange(len(allc)) - np.repeat(np.cumsum(lens) - lens, lens))
        pos = th.from_numpy(row * L + col).to(dev)
        up = th.from_numpy(allc).to(dev)

        def pad(vals, dtype=th.long):
            out = th.zeros(B * L, dtype=dtype, device=dev)
            out[pos] = vals.to(dtype)
            return out.view(B, L)

        tdata = {k: pad(up[:, i]) for i, k in enumerate(KEYS)}
        if flags is not None:
            tdata[REVFLAG] = pad(th.from_numpy(np.concatenate([np.asarray(f, bool) for f in flags])).to(dev), th.bool)
        outs = [pad(th.from_numpy(np.concatenate([np.asarray(a, np.int64) for a in arrs])).to(dev)) for arrs in (extra or [])]
        return EdgeSeq(tdata, lens, nn_), outs

    def to(self, device):
        if device is None or self.device == th.device(device):
            return self
        out = EdgeSeq({k: v.to(device) for k, v in self.tdata.items()}, self._lens, self._num_nodes)
        return out
