"""The dead-row conditions of a joint pass (dualmessagepassing_amd/fused.py: ``has_row_mask``, ``dead_h1_rows``, ``dead_edge_rows``,
``kept_node_path``, ``l0_row_list``, ``kept_incidence_sums``) as a truth table: a row that one launch leaves unwritten under a zero
of a ScalarFilter gate (basemodel.py:1515-1531) must be left out by every reader, so the forward, the backward, ``l0_dead_inputs``
and the side-stream prefetch all ask these host functions -- on CPU tensors here, against a stand-in index."""
import functools
import itertools
import types

import torch as th

SWITCHES = ("USE_ROW_MASKS", "USE_MASKED_SUMS", "USE_LIVE_TILES", "USE_NODE_ROWS", "USE_PLAIN_ATB", "SKIP_DEAD_ROWS")
GATES = ("none", "unmarked", "binary", "zero_rows", "zero_rows_view", "dense")


@functools.lru_cache(maxsize=None)
def _gate(kind, n):
    from dualmessagepassing_amd import gatememo
    if kind == "none":
        return None
    g = (th.arange(n) % 3 != 0).float()
    if kind != "unmarked":
        gatememo.mark(g, binary=True, zero_rows=kind != "binary", dense=kind == "dense")
    return g.view(-1, 1) if kind == "zero_rows_view" else g        # (a layer hands its kernels reshaped views of its gate)


def _expect(on, kind, N, E, H, own, start):
    """(a) .. (d), (f) from the switches and marks, stated independently of fused.py."""
    a = kind not in ("none", "dense") and on["USE_ROW_MASKS"]
    typed = H in (64, 128)
    zero_rows = a and kind in ("zero_rows", "zero_rows_view") and on["USE_MASKED_SUMS"]
    b = a and typed and on["SKIP_DEAD_ROWS"]
    c = b and zero_rows and on["USE_LIVE_TILES"] and own and E > 0
    d = zero_rows and typed and on["USE_NODE_ROWS"] and on["USE_PLAIN_ATB"] and N >= 4096 and E > 0 and start % 32 == 0
    return a, b, c, d, d and b and zero_rows


def _grid(fused, on, seen):
    coef = th.zeros(1)
    for kind, N, E, H, own, start, venc in itertools.product(GATES, (4095, 4096), (0, 40000), (64, 96, 128), (True, False), (0, 32, 8),
                                                             (False, True)):
        ix = types.SimpleNamespace(num_nodes=N, num_edges=E, _coef_deg=(coef if own else th.zeros(1), None))
        vg, eg = _gate(kind, N), _gate(kind, max(E, 1))
        # the first layer's stand-in: the pattern's table over the target's, whose node rows start at ``start``
        l0 = fused.Layer0Codes(None, 4, th.zeros(8, 1), esplit=min(64, E), nsplit=start, venc=th.zeros(1) if venc else None)
        a, b = fused.has_row_mask(eg), fused.dead_h1_rows(ix, H, eg)
        c, d = fused.dead_edge_rows(ix, H, eg, coef), fused.kept_node_path(ix, H, vg, l0)
        f = fused.kept_incidence_sums(ix, H, eg, d)
        point = (sorted(k for k in on if not on[k]), kind, N, E, H, own, start)
        assert (a, b, c, d, f) == _expect(on, kind, N, E, H, own, start), point
        assert a == fused.has_row_mask(vg) and (not c or b) and (not f or (d and b and fused.zero_rows_gate(eg))), point
        assert fused.l0_dead_inputs(ix, H, vg, eg, l0, coef) == (c, d and venc), point
        assert fused.l0_dead_inputs(ix, H, vg, eg, None, coef) == (False, False), point
        assert fused.kept_node_path(ix, H, vg) == _expect(on, kind, N, E, H, own, 0)[3], point        # (an inner layer: no tables)
        if kind in ("none", "dense") or H == 96:
            # (an UNMARKED gate has a row mask, and its H1e rows are dead -- the masked kernels test the gate's value, the forward's
            # ``dead_gate`` never asked for a mark; what needs the 0 / 1 mark and wiped input rows is (c), (d) and (f))
            assert not (b or c or d or f) and (H == 96 or not a), point
        if kind == "unmarked":
            assert not (c or d or f), point
        if N == 4095 or start == 8:
            assert not d and not f, point
        if not own:
            assert not c, point
        if all(on.values()) and kind in ("zero_rows", "zero_rows_view") and N == 4096 and E > 0 and H != 96 and own and start != 8:
            assert a and b and c and d and f, point
            seen.append(point)
        if not on["USE_ROW_MASKS"]:             # DMP_ROW_MASKS=0 takes all of it out
            assert not (a or b or c or d or f), point
        if not on["USE_NODE_ROWS"]:             # ... DMP_NODE_ROWS=0 the kept-node path and what hangs on it, nothing else
            assert (a, b, c, d, f) == _expect(dict(on, USE_NODE_ROWS=True), kind, N, E, H, own, start)[:3] + (False, False), point


def test_the_dead_row_conditions_as_a_truth_table():
    from dualmessagepassing_amd import fused
    saved = {k: getattr(fused, k) for k in SWITCHES}
    seen = []
    try:
        for off in (None,) + SWITCHES:
            for k in SWITCHES:
                setattr(fused, k, k != off)
            _grid(fused, {k: k != off for k in SWITCHES}, seen)
    finally:
        for k, v in saved.items():
            setattr(fused, k, v)
    assert len(seen) == 2 * 2 * 2 * 2             # two gate forms, H 64 / 128, tables at node 0 / 32, with and without node codes


def test_the_two_panel_kernels_limits_lie_inside_the_class_typed_kernels():
    """``mfma_ok(ix, H)`` implies ``typed_ok(ix, H)``: the fused layer asks ``typed_ok`` alone, no two-panel route stands behind its
    failure (H = 128 is an admitted width, N * 3H * 4 < 2^32 gives N < 2^31, E * 4 < 2^32 is E < 2^30)."""
    from dualmessagepassing_amd import fused
    rows = (1 << 32) // 1536
    both = []
    for N, E, H in itertools.product((0, 4096, rows - 1, rows, rows + 1, (1 << 31) - 1, 1 << 31), (0, (1 << 30) - 1, 1 << 30),
                                     (32, 64, 96, 128, 256)):
        ix = types.SimpleNamespace(num_nodes=N, num_edges=E)
        if fused.mfma_ok(ix, H):
            assert fused.typed_ok(ix, H), (N, E, H)
            both.append((N, E, H))
    assert (4096, 0, 128) in both


def test_a_first_layer_row_range_walks_a_list_from_an_aligned_start_and_a_minimum_of_rows():
    from dualmessagepassing_amd import fused
    m = fused.L0_LIST_MIN_ROWS
    assert fused.l0_row_list(1536, m) and fused.l0_row_list(0, m + 1)
    assert not fused.l0_row_list(1536, m - 1) and not fused.l0_row_list(8, m) and not fused.l0_row_list(1537, 4 * m)
    saved = fused.USE_L0_ROW_LISTS
    fused.USE_L0_ROW_LISTS = False
    try:
        assert not fused.l0_row_list(1536, m)
    finally:
        fused.USE_L0_ROW_LISTS = saved
