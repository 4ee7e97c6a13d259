"""The bf16x6 kernels that have no exact-fp32 form of their own -- each carries a hand-copied six-MFMA sequence over its own piece
layout (pieces staged in LDS, weight panels pre-split by a pack kernel, the codes k-group) and refuses ``dmp_dev_set_exact_fp32(1)``,
so tests/test_gpu_bf16x6.py's "3 x the exact form" cannot be pointed at them: ``bwd_h1_w`` with and without ``codes=``, ``bwd_z_w``,
``atb2`` (csrc/dmp_h1w.hip), ``out_fwd_typed_codes`` (csrc/dmp_typed.hip), ``edge_mlp_fwd`` (csrc/dmp_edgemlp.hip), the one-launch
``l0_edge_fwd(mlp=...)`` (csrc/dmp_l0mlp.hip), ``node_chain_fwd`` / ``node_chain_bwd`` with ``node_chain_panels`` (csrc/dmp_nodechain.hip),
``l0_node_fwd_mfma`` / ``l0_node_codes_bwd`` (csrc/dmp_l0node.hip: the 32x32x16 and the 16x16x32 sequence) and the LRP pooling product with
its three gradients (csrc/dmp_lrppool.hip).  The cases: tests/bf16x6_only_cases.py.

What is asserted, per kernel and output:

* the sparse ladder (tests/bf16x6_cases.py, proved in tests/test_bf16x6_ladder_cpu.py): every element within 2^-21 of fp64, exact zeros
  where fp64 is 0, the dead rows' sentinel bit for bit; every weight panel of every kernel is the dense ladder matrix once.  For a
  chained kernel the second stage is reached through a first stage that is an exact pass-through (a power-of-two permutation), whose
  stored output is checked ``torch.equal`` to the permuted ladder rows.  A single wrong first-order piece product is at least
  4 x 2^-21 off on every element;
* the adversarial scenarios: the error of the natural scale against the derived, order-independent fp32 bound
  ``sum over the stages of gamma_K + 2^-23`` -- a lost piece under a 120-binade spread or an overflow in the split costs 2^-16 of
  the dominating element's scale;
* where the kernel replaces launches that do have an exact form (``edge_mlp_fwd``: ``edge_fwd_typed`` + ``out_fwd_typed``; the node
  chain: ``typed_jobs`` / ``out_fwd_typed`` / ``bwd_h1_typed``; ``bwd_h1_w``: ``bwd_h1_typed`` + ``atb_typed(plain=True)``;
  ``out_fwd_typed_codes``: ``smallk_embed`` + ``out_fwd_typed``): at most 3 x their error under the switch on the same operands, with
  the floor 2^-24 (the factor of tests/test_gpu_bf16x6.py);
* ``tiny`` (magnitudes from 2^-118 up: ``bf16x6_only_cases.operands`` says why not N(0, 1) 2^-118 for sums of 12 to 40 terms): finite
  and within 2^-16 of the natural scale.

Every measured ratio is printed; the values of an MI355X run are recorded in profiles/bf16x6_envelope.json (the asserted bounds are the
derived ones and do not depend on that file).

What the tests see that the kernels' own do not (an experiment on an MI355X, not committed): with ``hi x lo`` left out of both six-MFMA
sequences of csrc/dmp_l0node.hip the ladder tests of ``l0_node_fwd_mfma`` and ``l0_node_codes_bwd`` fail (7.6e-6 of the element against
2^-21 = 4.8e-7; the forward also misses the derived bound, 3.4e-6 against 2.5e-6) while all 90 kernel tests of
tests/test_gpu_l0_node_mfma.py (``-k "against_fp64 or code_sums"``) pass; with ``mid x mid`` issued twice in its place the ladder tests
fail at 2.1e-5 and 88 of those 90 pass."""
import pytest

pytestmark = pytest.mark.gpu

KERNELS = ["bwd_h1_w", "bwd_h1_w_codes", "bwd_z_w", "atb2", "out_fwd_typed_codes", "edge_mlp_fwd", "l0_edge_mlp", "node_chain", "l0_node_fwd_mfma",
           "l0_node_codes_bwd", "lrp_pool"]
SCENARIOS = ["normal", "element_binades", "row_binades", "cancel", "small", "huge"]
NO_CANCEL = ("edge_mlp_fwd", "node_chain", "atb2", "l0_node_codes_bwd", "lrp_pool")      # chains, and products contracted over the rows alone: no single product runs on ``cancel``
FLOOR = 2.0 ** -24
_MEASURED = {}


def _measured(kernel, gpu):
    """One kernel's records, made once and shared by its tests"""
    if kernel not in _MEASURED:
        from bf16x6_only_cases import run_only
        _MEASURED[kernel] = run_only(gpu, [kernel])[kernel]
    return _MEASURED[kernel]


def test_the_cases_cover_the_kernels_listed_here():
    from bf16x6_only_cases import ENVELOPE, KERNELS as CASES
    assert sorted(CASES) == sorted(KERNELS) and list(ENVELOPE) == SCENARIOS


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_piece_product_on_the_sparse_ladder(kernel, gpu):
    from bf16x6_cases import LADDER_BOUND
    outputs = _measured(kernel, gpu)["ladder"]
    assert outputs
    for output, r in outputs.items():
        print("%s %s on the sparse ladder: %.3g of the element (bound %.3g)%s" % (kernel, output, r["err"], LADDER_BOUND, "" if r["ok"] else "  NOT ok"))
    for output, r in outputs.items():
        assert r["ok"], "%s %s: not finite, not 0 where fp64 is 0, a dead row written, or a pass-through stage not bit for bit" % (kernel, output)
        assert r["err"] <= LADDER_BOUND, "%s %s: %.3g" % (kernel, output, r["err"])


@pytest.mark.parametrize("scenario", SCENARIOS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_inside_the_derived_fp32_bound_and_the_replaced_route(kernel, scenario, gpu):
    outputs = _measured(kernel, gpu).get(scenario, {})
    assert outputs or (scenario == "cancel" and kernel in NO_CANCEL), (kernel, scenario)
    for output, r in outputs.items():
        print("%s %s on %s: %.3g of the natural scale (bound %.3g%s)" % (kernel, output, scenario, r["err"], r["bound"],
                                                                        ", the replaced route on exact fp32 %.3g" % r["route"] if "route" in r else ""))
    for output, r in outputs.items():
        assert r["ok"], "%s %s on %s: not finite, or a dead row written" % (kernel, output, scenario)
        assert r["err"] <= r["bound"], "%s %s on %s: %.3g above %.3g" % (kernel, output, scenario, r["err"], r["bound"])
        if "route" in r:
            assert r["err"] <= max(3.0 * r["route"], FLOOR), "%s %s on %s: %.3g vs the replaced route's %.3g" % (kernel, output, scenario, r["err"], r["route"])


@pytest.mark.parametrize("kernel", KERNELS)
def test_below_its_range_degrades_to_two_pieces(kernel, gpu):
    outputs = _measured(kernel, gpu)["tiny"]
    assert outputs
    for output, r in outputs.items():
        print("%s %s on tiny: %.3g of the natural scale" % (kernel, output, r["err"]))
    for output, r in outputs.items():
        assert r["ok"], (kernel, output)
        assert r["err"] <= 2.0 ** -16, "%s %s: %.3g" % (kernel, output, r["err"])


def test_the_exact_switch_is_off_afterwards(gpu):
    from dualmessagepassing_amd import _lib
    assert not _lib.load().dmp_dev_get_exact_fp32()
