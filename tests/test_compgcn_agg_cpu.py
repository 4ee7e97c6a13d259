"""CPU checks of what ``test_gpu_compgcn_agg_fp64.py`` leans on: the float64 yardstick ``util_fp64_compagg.compagg_fp64``
against the oracle's composition and segment sum (in double, 1e-12), ``compgcn.dft_matrices`` against the library's real FFT
(the matrices are stored in fp32: one rounding per entry, at most 6e-8 of scale at the widths below when evaluated in double;
the figure here is 1e-6), and the case list's own claims: which lane group, which kernel, which degrees and which grids
every case reaches."""
import pytest
import torch as th

import dmp_oracle as O
import util_fp64_compagg as C

H_DFT = (1, 2, 3, 6, 7, 16, 64, 127, 128, 254, 256, 512)


def _rel(a, ref):
    err, scale = C.dist(a, ref)
    return err / scale


def _halves(msg, gr):
    """[sum over rev = 0 | sum over rev = 1] of per-edge rows with the oracle's segment sum."""
    rev = th.zeros(gr["E"], dtype=th.bool) if gr["rev"] is None else gr["rev"]
    lo = O.seg_sum(msg.masked_fill(rev.view(-1, 1), 0.0), gr["dst"], gr["N"])
    hi = O.seg_sum(msg.masked_fill(~rev.view(-1, 1), 0.0), gr["dst"], gr["N"])
    return lo, hi


@pytest.mark.parametrize("rev", ["mixed", "none", "all"])
@pytest.mark.parametrize("G", [16, 32, 64])
def test_compagg_fp64_matches_the_oracle(G, rev):
    gr = C.ladder_graph(G, 0, rev)
    g = th.Generator().manual_seed(G)
    h = 12
    x = th.randn(gr["N"], h, generator=g).double()
    z = th.randn(gr["E"], h, generator=g).double()
    norm = (th.rand(gr["E"], generator=g) + 0.1).double()
    for comp in ("sub", "mult"):
        for nrm in (norm, None):
            msg = O.compgcn_comp(x[gr["src"]], z, comp)
            if nrm is not None:
                msg = msg * nrm.view(-1, 1)
            got = C.compagg_fp64(x, z, gr["src"], gr["dst"], gr["rev"], nrm, gr["N"], comp)
            assert _rel(got, th.cat(_halves(msg, gr), 1)) <= 1e-12, comp
    # conj-multiply of the transforms: the inverse transform of the sum is the sum of the time-domain correlations
    for h in (12, 7):
        x, z = x[:, :h], z[:, :h]
        fx = th.view_as_real(th.fft.rfft(x, dim=-1)).reshape(gr["N"], -1)
        fz = th.view_as_real(th.fft.rfft(z, dim=-1)).reshape(gr["E"], -1)
        got = C.compagg_fp64(fx, fz, gr["src"], gr["dst"], gr["rev"], norm, gr["N"], "cmul")
        w = fx.size(1)
        back = [th.fft.irfft(th.view_as_complex(got[:, k * w:(k + 1) * w].reshape(gr["N"], -1, 2).contiguous()), n=h, dim=-1)
                for k in (0, 1)]
        lo, hi = _halves(O.compgcn_comp(x[gr["src"]], z, "corr") * norm.view(-1, 1), gr)
        assert _rel(back[0], lo) <= 1e-12 and _rel(back[1], hi) <= 1e-12, h
    if rev == "none":
        assert float(got[:, w:].abs().max()) == 0.0


def test_tensor_op_yardstick_is_the_same_operation():
    """The fp32 yardstick's arithmetic, run in double, is ``compagg_fp64`` (it is a second statement: no complex views)."""
    for name in ("G16-H20-sub", "G32-H68-cmul-rev_none-norm1","G64-H132-mult", "n1-self-H64-cmul", "n5-e0-H64-sub"):
        c = C.compagg_cases()[name]
        gr, X, Z, norm, _ = C.case_inputs(name)
        a = C.compagg_fp64(X.double(), Z.double(), gr["src"], gr["dst"], gr["rev"], None if norm is None else norm.double(),
                           gr["N"], c["comp"])
        b = C._compagg_tensor_ops(X.double(), Z.double(), gr["src"], gr["dst"], gr["rev"],
                                  None if norm is None else norm.double(), gr["N"], c["comp"])
        assert a.shape == b.shape == (gr["N"], 2 * c["H"]) and _rel(b, a) <= 1e-12, name


@pytest.mark.parametrize("h", H_DFT)
def test_dft_matrices_are_the_real_fft(h):
    from dualmessagepassing_amd.compgcn import _cmul_conj, dft_matrices
    D, Dinv = dft_matrices(h, "cpu")
    bins = h // 2 + 1
    w = (2 * bins + 3) // 4 * 4
    assert w % 4 == 0 and 2 * bins <= w < 2 * bins + 4
    assert D.dtype == th.float32 and tuple(D.shape) == (h, w) and tuple(Dinv.shape) == (w, h)
    assert float(D[:, 2 * bins:].abs().sum()) == 0.0 and float(Dinv[2 * bins:].abs().sum()) == 0.0
    D, Dinv = D.double(), Dinv.double()
    g = th.Generator().manual_seed(h)
    x = th.randn(9, h, generator=g).double()
    r = th.randn(1, h, generator=g).double()
    z = th.randn(9, h, generator=g).double()
    fx = x @ D
    want = th.zeros(9, w, dtype=th.float64)
    want[:, :2 * bins] = th.view_as_real(th.fft.rfft(x, dim=-1)).reshape(9, -1)
    assert _rel(fx, want) <= 1e-6
    assert float(fx[:, 2 * bins:].abs().max()) == 0.0 if w > 2 * bins else True
    # the inverse ignores the imaginary parts of the DC bin and (even h) of the Nyquist bin, as the library's irfft does
    assert float(Dinv[1].abs().max()) == 0.0
    if h % 2 == 0:                  # sin(pi j) / h in double: j ulp(pi) / h <= 4.5e-16 off zero, not exactly zero
        assert float(Dinv[2 * bins - 1].abs().max()) <= 1e-15
    assert _rel(fx @ Dinv, x) <= 1e-6
    for rel in (r, z):
        assert _rel(_cmul_conj(fx, rel @ D) @ Dinv, O.compgcn_comp(x, rel.expand(9, h), "corr")) <= 1e-6


def test_dft_widths_select_the_lane_groups_the_gpu_module_names():
    from dualmessagepassing_amd.compgcn import dft_matrices
    got = {h: C.group_lanes(dft_matrices(h, "cpu")[0].size(1)) for h in (7, 16, 64, 127, 128, 254, 256)}
    assert got == {7: 16, 16: 16, 64: 32, 127: 32, 128: 64, 254: 64, 256: 64}
    assert dft_matrices(256, "cpu")[0].size(1) == 260 and dft_matrices(512, "cpu")[0].size(1) == 516


@pytest.mark.parametrize("G", [16, 32, 64])
def test_ladder_graph_reaches_every_chunk_count_and_an_uneven_grid(G):
    for rev in ("mixed", "none", "all"):
        gr = C.ladder_graph(G, 0, rev)
        C.check_ladder(gr)
        rpb = C.BLOCK // G
        assert C.blocks(gr["N"], rpb) == 11
        nb = C.blocks(gr["E"], rpb)
        assert nb > 8 and nb % 8 != 0 and gr["E"] % rpb == 1 and gr["E"] < 1000
        indeg = th.bincount(gr["dst"], minlength=gr["N"])
        chunks = {int(-(-d // G)) for d in indeg.tolist()}
        assert {0, 1, 2, 3} <= chunks
        tails = {int(d) % G % 2 for d in indeg.tolist() if d > G}                     # the last chunk's odd tail, and none
        assert tails == {0, 1}
        assert (gr["rev"] is None) == (rev == "none")
        if rev == "all":
            assert bool(gr["rev"].all())
        if rev == "mixed":
            assert 0 < int(gr["rev"].sum()) < gr["E"]
    assert th.equal(C.ladder_graph(G, 0, "mixed")["src"], C.ladder_graph(G, 0, "none")["src"])


def test_case_list_covers_what_it_claims():
    cases = C.compagg_cases()
    by = lambda **kw: [n for n, c in cases.items() if all(c[k] == v for k, v in kw.items())]
    for G, hs in {16: (4, 20, 64), 32: (68, 128), 64: (132, 256, 260, 516)}.items():
        for H in hs:
            assert C.group_lanes(H) == G
            for comp in C.COMPS:
                assert by(H=H, G=G, comp=comp, rev="mixed", norm=True, path="vec", xview=None, zview=None, graph="ladder"), (H, comp)
        for rev in ("none", "all"):
            assert by(G=G, rev=rev, path="vec", graph="ladder")
        assert by(G=G, norm=False, path="vec", graph="ladder")
        assert by(G=G, norm=False, rev="none", comp="cmul", path="vec")
        assert any(c["xview"] == (4, 2 * c["H"] + 8) for c in cases.values() if c["G"] == G and c["path"] == "vec")
    for H in (1, 3, 6, 130):
        for comp in ("sub", "mult"):
            assert by(H=H, comp=comp, path="scalar", xview=None, zview=None, graph="ladder")
    forced = [c for c in cases.values() if c["path"] == "scalar" and c["H"] == 64]
    assert {(c["xview"] or c["zview"]) for c in forced} == {(1, 68), (0, 66)}
    assert by(path="unsupported", comp="cmul", xview=(1, 68))
    assert by(graph="n1-self") and by(graph="n5-e0")
    assert len(cases) < 100
    for name, c in cases.items():
        if c["graph"] != "ladder":
            continue
        if c["path"] == "vec":
            assert C.vec_ok(c) and C.group_lanes(c["H"]) == c["G"], name
            for v in (c["xview"], c["zview"]):
                assert v is None or v[0] + c["H"] <= v[1]
        else:
            # four rows (edges) of 64 lanes per workgroup: the scalar kernels' grids are the G = 64 graph's
            assert not C.vec_ok(c) and c["G"] == 64, name
            assert (c["path"] == "unsupported") == (c["comp"] == "cmul"), name
        assert c["comp"] != "cmul" or c["H"] % 2 == 0
        if c["H"] > 256:
            assert c["G"] == 64 and -(-c["H"] // 256) in (2, 3)                         # a second, a third column pass
    assert {-(-c["H"] // 256) for c in cases.values() if c["path"] == "vec"} == {1, 2, 3}


def test_case_inputs_are_fp32_values_and_repeat():
    for name in ("G64-H516-cmul", "scalar-H64-sub-col1", "n5-e0-H64-mult"):
        a, b = C.case_inputs(name), C.case_inputs(name)
        for s, t in zip(a[1:], b[1:]):
            assert (s is None and t is None) or (s.dtype == th.float32 and th.equal(s, t))
        gr, X, Z, _, w = a
        c = C.compagg_cases()[name]
        assert tuple(X.shape) == (gr["N"], c["H"]) and tuple(Z.shape) == (gr["E"], c["H"]) and tuple(w.shape) == (gr["N"], 2 * c["H"])
    gen = th.Generator().manual_seed(0)
    t = th.randn(5, 8)
    wide = C.widen(t, (4, 24), gen)
    assert tuple(wide.shape) == (5, 24) and th.equal(wide[:, 4:12], t) and float(wide[:, :4].abs().min()) > 0.0


def test_reference_gradients_match_their_closed_forms():
    """Autograd on ``compagg_fp64`` against the header's formulas: g_e = norm_e w[dst e, half of e]; dZ_e = -g, g x, g x
    (complex product); the per-edge term of dX = g, g z, conj(g) z, summed by source."""
    for name in ("G16-H20-sub", "G16-H20-mult", "G16-H20-cmul"):
        c = C.compagg_cases()[name]
        gr, X, Z, norm, w = C.case_inputs(name)
        ref = C.reference(name)
        H, E = c["H"], gr["E"]
        X, Z, w, norm = X.double(), Z.double(), w.double(), norm.double()
        gsel = th.where(gr["rev"].view(-1, 1), w[gr["dst"], H:], w[gr["dst"], :H]) * norm.view(-1, 1)
        xs = X[gr["src"]]
        if c["comp"] == "sub":
            dz, dxe = -gsel, gsel
        elif c["comp"] == "mult":
            dz, dxe = gsel * xs, gsel * Z
        else:
            cx = lambda t: th.view_as_complex(t.reshape(E, H // 2, 2).contiguous())
            dz = th.view_as_real(cx(gsel) * cx(xs)).reshape(E, H)
            dxe = th.view_as_real(th.conj(cx(gsel)) * cx(Z)).reshape(E, H)
        assert _rel(ref["dZ"], dz) <= 1e-12, name
        assert _rel(ref["dX"], O.seg_sum(dxe, gr["src"], gr["N"])) <= 1e-12, name
