"""Float64 restatement of the CompGCN message aggregation (csrc/dmp_agg.hip: ``dmp_compgcn_agg`` and its backward), the
graphs that walk its lane groups' entry chunks, and the case list that ``test_compgcn_agg_cpu.py`` (which checks this
yardstick and what the cases reach) and ``test_gpu_compgcn_agg_fp64.py`` (which runs them) share.

    m_e    = comp(X[src e], Z[e]) * norm_e        comp: x - z, x * z, conj(x) * z over interleaved (re, im) pairs
    out[v] = [sum of m_e over the in-edges of v with rev_e = 0 | the same over rev_e = 1]

Written from that definition with ``index_add``; nothing of ``dualmessagepassing_amd`` runs here.  Gradients: autograd."""
import functools

import torch as th

from util_fp64 import close, dist, stable_seed  # noqa: F401  (the GPU module takes them from here)

COMPS = ("sub", "mult", "cmul")           # the kernels' comp 0, 1, 2 (ops.COMP_SUB, COMP_MULT, COMP_CMUL)
BLOCK = 256                               # kBlock of csrc/dmp_common.h: threads of a workgroup
XCDS = 8                                  # kXcds: a grid of up to 8 workgroups is left in dispatch order by xcd_remap
TOL = 1e-5                                # |delta| <= 1e-5 max(1, |ref|max), the layer figure


def group_lanes(H):
    """``group_lanes`` of csrc/dmp_agg.hip restated: the lanes that share one row."""
    return 16 if H <= 64 else (32 if H <= 128 else 64)


def compagg_fp64(X, Z, src, dst, rev, norm, N, comp):
    """X [N', H], Z [E, H] double; src, dst int64 [E]; rev bool [E] or None (no flag: every edge in the first half);
    norm [E] or None -> out [N, 2H]."""
    assert X.dtype == th.float64 and Z.dtype == th.float64
    E, H = Z.shape
    xs = X[src]
    if comp == "sub":
        m = xs - Z
    elif comp == "mult":
        m = xs * Z
    elif comp == "cmul":
        assert H % 2 == 0
        xc = th.view_as_complex(xs.reshape(E, H // 2, 2))
        zc = th.view_as_complex(Z.reshape(E, H // 2, 2))
        m = th.view_as_real(th.conj(xc) * zc).reshape(E, H)
    else:
        raise ValueError(comp)
    if norm is not None:
        m = m * norm.reshape(-1, 1)
    r = th.zeros(E, dtype=th.bool) if rev is None else rev.bool()
    zero = th.zeros((), dtype=th.float64)
    lo = th.zeros(N, H, dtype=th.float64).index_add(0, dst, th.where(r.view(-1, 1), zero, m))
    hi = th.zeros(N, H, dtype=th.float64).index_add(0, dst, th.where(r.view(-1, 1), m, zero))
    return th.cat([lo, hi], 1)


# ------------------------------------------------------------------------------------------------------------ the graphs

def ladder_degrees(G):
    return (0, 1, 2, G - 1, G, G + 1, 2 * G, 2 * G + 1)


def blocks(rows, rpb):
    return (rows + rpb - 1) // rpb


def grid_is_remapped_unevenly(rows, rpb):
    """More than one workgroup per XCD and not the same number on each: ``xcd_remap`` permutes, with a remainder."""
    nb = blocks(rows, rpb)
    return nb > XCDS and nb % XCDS != 0


@functools.lru_cache(maxsize=None)
def ladder_graph(G, seed=0, rev="mixed"):
    """dict(N, E, src, dst, rev (bool [E] or None), ladder: {in-degree: node}, self_loop, repeated, source_only) for the
    lane-group size G (RPB = 256 / G rows -- and edges, in the backward -- per workgroup).

    N = 10 RPB + 1: 11 workgroups, the last with one row.  Eight nodes carry the in-degrees 0, 1, 2, G - 1, G, G + 1, 2 G and
    2 G + 1 (none, one, two and three entry chunks; an even and an odd tail of the two-at-a-time body) -- the hub of 2 G + 1 is
    the last node, alone in its workgroup, and G + 1 is node 0 --; about 2 N random edges go to the other nodes, among them a
    self loop and a repeated (u, v); the node of in-degree 0 is a source.  Edges are added until E % RPB = 1 and the
    backward's grid has more than 8 workgroups and no multiple of 8.  The edge ids are shuffled."""
    assert rev in ("mixed", "none", "all")
    rpb = BLOCK // G
    N = 10 * rpb + 1
    g = th.Generator().manual_seed(1000 * G + seed)
    degs = ladder_degrees(G)
    spots = th.randperm(N - 2, generator=g)[:len(degs) - 2].add(1).tolist()       # six of the nodes 1 .. N - 2
    nodes = dict(zip([d for d in degs if d not in (G + 1, 2 * G + 1)], spots))
    nodes[G + 1], nodes[2 * G + 1] = 0, N - 1
    free = th.tensor(sorted(set(range(N)) - set(nodes.values())))
    pairs = []
    for d, v in nodes.items():
        pairs += [(int(u), v) for u in th.randint(0, N, (d,), generator=g)]
    k = 2 * N
    fu = th.randint(0, N, (k,), generator=g)
    fv = free[th.randint(0, free.numel(), (k,), generator=g)]
    pairs += list(zip(fu.tolist(), fv.tolist()))
    loop = int(free[0])
    rep = (int(free[1]), int(free[2]))
    pairs += [(loop, loop), rep, rep, (nodes[0], int(free[3]))]
    while len(pairs) % rpb != 1 or not grid_is_remapped_unevenly(len(pairs), rpb):
        pairs.append((int(th.randint(0, N, (1,), generator=g)), int(free[th.randint(0, free.numel(), (1,), generator=g)])))
    perm = th.randperm(len(pairs), generator=g)
    uv = th.tensor(pairs, dtype=th.int64)[perm]
    src, dst = uv[:, 0].contiguous(), uv[:, 1].contiguous()
    E = src.numel()
    flag = {"mixed": th.rand(E, generator=g) < 0.5, "none": None, "all": th.ones(E, dtype=th.bool)}[rev]
    out = dict(N=N, E=E, src=src, dst=dst, rev=flag, ladder=nodes, self_loop=loop, repeated=rep, source_only=nodes[0], G=G)
    check_ladder(out)
    return out


def check_ladder(gr):
    G, N, E, src, dst = gr["G"], gr["N"], gr["E"], gr["src"], gr["dst"]
    rpb = BLOCK // G
    indeg = th.bincount(dst, minlength=N)
    assert N == 10 * rpb + 1 and grid_is_remapped_unevenly(N, rpb) and N % rpb == 1
    assert E % rpb == 1 and grid_is_remapped_unevenly(E, rpb) and E < 1000
    assert sorted(gr["ladder"]) == sorted(ladder_degrees(G)) and len(set(gr["ladder"].values())) == 8
    for d, v in gr["ladder"].items():
        assert int(indeg[v]) == d, (d, v, int(indeg[v]))
    assert int(indeg.max()) == 2 * G + 1
    assert bool(((src == dst) & (src == gr["self_loop"])).any())
    u, v = gr["repeated"]
    assert int(((src == u) & (dst == v)).sum()) >= 2
    s = gr["source_only"]
    assert int(indeg[s]) == 0 and bool((src == s).any())
    assert not th.equal(dst, dst.sort().values), "the CSR order must differ from the edge order"
    if gr["rev"] is not None and not bool(gr["rev"].all()):
        hub = gr["rev"][dst == N - 1]
        assert bool(hub.any()) and not bool(hub.all())


def small_graph(kind):
    """"n1-self": one node with five self loops; "n5-e0": five nodes, no edge."""
    if kind == "n1-self":
        z = th.zeros(5, dtype=th.int64)
        return dict(N=1, E=5, src=z, dst=z.clone(), rev=th.tensor([False, True, True, False, True]), G=None)
    assert kind == "n5-e0"
    e = th.zeros(0, dtype=th.int64)
    return dict(N=5, E=0, src=e, dst=e.clone(), rev=th.zeros(0, dtype=th.bool), G=None)


# ------------------------------------------------------------------------------------------------------------- the cases

def compagg_cases():
    """ids -> dict(H, G (of the ladder graph; None: a small graph), comp, rev, norm, path ("vec", "scalar", "unsupported"),
    xview, zview ((first column, leading dimension) of the wider matrix the rows are a column slice of, or None), graph
    ("ladder", "n1-self", "n5-e0")).

    The scalar kernels take four rows per workgroup, as the 64-lane groups do: their cases run on the G = 64 graph."""
    cases = {}

    def add(name, H, G, comp, rev="mixed", norm=True, path="vec", xview=None, zview=None, graph="ladder"):
        assert name not in cases
        cases[name] = dict(H=H, G=G, comp=comp, rev=rev, norm=norm, path=path, xview=xview, zview=zview, graph=graph)

    widths = {16: (4, 20, 64), 32: (68, 128), 64: (132, 256, 260, 516)}
    for G, hs in widths.items():
        for H in hs:
            for comp in COMPS:
                add("G%d-H%d-%s" % (G, H, comp), H, G, comp)
    for G, H in ((16, 20), (32, 68), (64, 132), (64, 516)):
        for i, (rev, norm) in enumerate((("none", True), ("all", True), ("mixed", False), ("none", False))):
            comp = COMPS[(i + G // 16) % 3] if i < 3 else "cmul"          # rev none, norm off: the backward's two NULLs at once
            add("G%d-H%d-%s-rev_%s-norm%d" % (G, H, comp, rev, norm), H, G, comp, rev=rev, norm=norm)
    for H in (1, 3, 6, 130):
        for comp in ("sub", "mult"):
            add("scalar-H%d-%s" % (H, comp), H, 64, comp, path="scalar")
    add("scalar-H3-mult-rev_none-norm0", 3, 64, "mult", rev="none", norm=False, path="scalar")
    add("scalar-H64-sub-col1", 64, 64, "sub", path="scalar", xview=(1, 68))                 # a base 4 bytes off 16
    add("scalar-H64-mult-col1", 64, 64, "mult", path="scalar", zview=(1, 68))
    add("scalar-H64-sub-ld66", 64, 64, "sub", path="scalar", zview=(0, 66))                 # ld = H + 2
    add("scalar-H64-mult-ld66", 64, 64, "mult", path="scalar", xview=(0, 66))
    for G, H in ((16, 64), (32, 68), (64, 260)):
        for comp in COMPS:
            add("strided-G%d-H%d-%s" % (G, H, comp), H, G, comp, xview=(4, 2 * H + 8), zview=(8, 2 * H + 16))
    add("unsupported-H64-cmul-col1", 64, 64, "cmul", path="unsupported", xview=(1, 68))
    add("unsupported-H68-cmul-ld70", 68, 64, "cmul", path="unsupported", zview=(0, 70))
    for comp in COMPS:
        add("n1-self-H64-" + comp, 64, None, comp, graph="n1-self")
        add("n5-e0-H64-" + comp, 64, None, comp, graph="n5-e0")
    add("n5-e0-H3-sub", 3, None, "sub", graph="n5-e0", path="scalar")
    return cases


def vec_ok(c):
    """``vec_ok`` of csrc/dmp_agg.hip for a case: H, every leading dimension and every first column a multiple of 4 (torch's
    allocations start on 16 bytes and more; ``out`` and the gradients are dense, [., 2H] and [., H])."""
    ok = c["H"] % 4 == 0
    for v in (c["xview"], c["zview"]):
        if v is not None:
            ok = ok and v[0] % 4 == 0 and v[1] % 4 == 0
    return ok


def case_graph(c, seed=0):
    return ladder_graph(c["G"], seed, c["rev"]) if c["graph"] == "ladder" else small_graph(c["graph"])


def widen(t, view, gen):
    """``t`` as the column slice [first, first + H) of a wider matrix of random numbers with ``ld`` columns."""
    if view is None:
        return t
    first, ld = view
    wide = th.randn(t.size(0), ld, generator=gen, dtype=th.float32).to(t.dtype)
    wide[:, first:first + t.size(1)] = t
    return wide


def case_inputs(name):
    """(graph, X [N, H], Z [E, H], norm [E] or None, w [N, 2H]: the upstream weights of both halves) in float32 on the CPU
    (their doubles are the reference's inputs).  X, Z N(0, 1); norm in [0.1, 1.1)."""
    c = compagg_cases()[name]
    gr = case_graph(c)
    g = th.Generator().manual_seed(stable_seed(name))
    X = th.randn(gr["N"], c["H"], generator=g)
    Z = th.randn(gr["E"], c["H"], generator=g)
    norm = th.rand(gr["E"], generator=g) + 0.1 if c["norm"] else None
    w = th.randn(gr["N"], 2 * c["H"], generator=g)
    return gr, X, Z, norm, w


def reference(name, dtype=th.float64, device="cpu"):
    """dict(out, dX, dZ) of a case from ``compagg_fp64``'s arithmetic in ``dtype`` (float64 on the CPU: the reference;
    float32 on the GPU: the tensor-op yardstick -- the same gather, composition and ``index_add``)."""
    c = compagg_cases()[name]
    gr, X, Z, norm, w = case_inputs(name)
    cast = lambda t: None if t is None else t.detach().clone().to(device=device, dtype=dtype)
    Xd, Zd = cast(X).requires_grad_(True), cast(Z).requires_grad_(True)
    src, dst = gr["src"].to(device), gr["dst"].to(device)
    rev = None if gr["rev"] is None else gr["rev"].to(device)
    if dtype == th.float64:
        out = compagg_fp64(Xd, Zd, src, dst, rev, cast(norm), gr["N"], c["comp"])
    else:
        out = _compagg_tensor_ops(Xd, Zd, src, dst, rev, cast(norm), gr["N"], c["comp"])
    (out * cast(w)).sum().backward()
    dX = Xd.grad if Xd.grad is not None else th.zeros_like(Xd)
    dZ = Zd.grad if Zd.grad is not None else th.zeros_like(Zd)
    return dict(out=out.detach(), dX=dX, dZ=dZ)


def _compagg_tensor_ops(X, Z, src, dst, rev, norm, N, comp):
    """The same sum with the working precision's tensor ops: gather, compose, ``index_add_``."""
    E, H = Z.shape
    xs = X[src]
    if comp == "sub":
        m = xs - Z
    elif comp == "mult":
        m = xs * Z
    else:
        xr, xi, zr, zi = xs[:, 0::2], xs[:, 1::2], Z[:, 0::2], Z[:, 1::2]
        m = th.stack([xr * zr + xi * zi, xr * zi - xi * zr], dim=-1).reshape(E, H)
    if norm is not None:
        m = m * norm.reshape(-1, 1)
    col = th.zeros(E, dtype=th.int64, device=Z.device) if rev is None else rev.to(th.int64)
    out = th.zeros(2 * N, H, dtype=Z.dtype, device=Z.device)
    out = out.index_add(0, dst + N * col, m)
    return th.cat([out[:N], out[N:]], 1)
