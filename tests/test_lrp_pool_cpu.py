"""CPU-side checks of the pool kernels' yardstick and entry points (csrc/dmp_lrppool.hip; no GPU needed):

* the float64 loop restatement of ``util_fp64_lrp`` equals the reference's formulation -- the two selection matrices and
  ``einsum('dab,bca->dc')`` (lrp.py:66-73), built in double from ``PermIndex.from_graphs`` on the CPU, autograd for the
  gradients -- on every case the GPU module runs, to 1e-10 (the figure of test_fp64_refs_cpu.py);
* the built library exports the new entry points with the header's signatures and decides the admitted shapes on the host."""
import os

import pytest
import torch as th

import util_fp64 as U
import util_fp64_lrp as UL

CASES = UL.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_loop_restatement_equals_the_selection_matrix_form(name):
    from dualmessagepassing_amd.lrp import PermIndex
    c = CASES[name]
    L, L2 = c["L"], c["L"] * c["L"]
    perm = PermIndex.from_graphs(c["graphs"], th.device("cpu"), L)
    N, E, P = perm.num_nodes, perm.num_edges, perm.num_perms
    x, z, w, _, dout, _ = UL.inputs(name, N, E, P, L, c["fin"], c["hid"])
    got = UL.perm_product_fp64(perm.slot, N, E, L, x, z, w, dout)

    rows = th.arange(P * L2)
    n2p, e2p = th.zeros(P * L2, N, dtype=th.float64), th.zeros(P * L2, E, dtype=th.float64)
    is_node, is_edge = perm.slot < N, (perm.slot >= N) & (perm.slot < N + E)
    n2p[rows[is_node], perm.slot[is_node]] = 1.0
    e2p[rows[is_edge], perm.slot[is_edge] - N] = 1.0
    xd, zd, wd = (t.double().requires_grad_(True) for t in (x, z, w))
    out = th.einsum("dab,bca->dc", (n2p @ xd + e2p @ zd).view(P, L2, c["fin"]), wd)
    (out * dout.double()).sum().backward()
    for a, ref, what in zip(got, (out.detach(), xd.grad, zd.grad, wd.grad), ("out", "d node_feat", "d edge_feat", "d weight")):
        U.close(a, ref, 1e-10, name + " " + what)
    if P:
        assert int(is_node.sum()) >= P and float(out.detach().abs().max()) > 0          # slot (0, 0) of every permutation is its node


def test_library_exports_the_pool_entries_and_decides_shapes_on_the_host():
    from dualmessagepassing_amd import _abi, _lib
    lib = _lib.load()
    assert lib.dmp_abi_version() == 97 == _abi.ABI_VERSION
    for name in ("dmp_lrp_pool_supported", "dmp_lrp_pool_workspace_words", "dmp_lrp_pool_fwd", "dmp_lrp_pool_bwd"):
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (_abi.SIGNATURES[name][0], list(_abi.SIGNATURES[name][1])), name
    import util_header
    from conftest import ROOT
    h = util_header.read(os.path.join(ROOT, "include", "dmp_hip.h"))
    for name in ("dmp_lrp_pool_supported", "dmp_lrp_pool_workspace_words", "dmp_lrp_pool_fwd", "dmp_lrp_pool_bwd"):
        res, args = h.signature(_abi, name)
        assert _abi.SIGNATURES[name][0] is res and list(_abi.SIGNATURES[name][1]) == list(args), name
    for fin in (64, 128):
        for hid in (64, 128):
            for L in (1, 4, 6):
                assert lib.dmp_lrp_pool_supported(fin, hid, L) == 1, (fin, hid, L)
                # the panels' three bf16 planes and at least one partial of the weight gradient
                assert lib.dmp_lrp_pool_workspace_words(0, fin, hid, L) >= L * L * fin * hid * 5 // 2
    assert lib.dmp_lrp_pool_supported(96, 64, 4) == 0 and lib.dmp_lrp_pool_supported(64, 96, 4) == 0
    assert lib.dmp_lrp_pool_supported(64, 64, 0) == 0 and lib.dmp_lrp_pool_supported(64, 64, _abi.DMP_LRP_MAX_SEQ_LEN + 1) == 0
    assert lib.dmp_lrp_pool_workspace_words(100, 96, 64, 4) == 0
    # refused before any launch: null pointers, no stream, no GPU on this side
    assert lib.dmp_lrp_pool_fwd(None, None, None, None, 5, 3, 2, 96, 64, 4, None, None, None) == -2
    assert lib.dmp_lrp_pool_fwd(None, None, None, None, 5, 3, 2, 64, 64, 7, None, None, None) == -2
    assert lib.dmp_lrp_pool_bwd(None, None, None, None, None, None, None, 5, 3, 2, 64, 96, 4, None, None, None, None, None) == -2
    assert lib.dmp_lrp_pool_fwd(None, None, None, None, -1, 3, 2, 64, 64, 4, None, None, None) == -1
    assert lib.dmp_lrp_pool_fwd(None, None, None, None, 5, 3, 2, 64, 64, 4, None, None, None) == -1       # admitted shape, no arrays
