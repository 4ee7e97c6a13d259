"""The matching half of the step and of the evaluation on the CPU:

* ``harness.match_terms_tensor`` (the definition ``dmp_match_loss`` implements) in fp64 against ``harness._match_terms``
  -- the restatement of train.py:627-649 -- run on an fp32 copy: loss, regulariser and both gradients, the non-zero
  gradient at a masked position included; a padded batch (capacity columns in front, inert pairs) gives the real pairs'
  values and exact zeros elsewhere; no real pair gives zeros;
* ``harness.binary_auc`` against ``sklearn.metrics.roc_auc_score``;
* ``PairDataset.batch_arrays(subs=...)``: the subisomorphism rows at a fixed capacity;
* the committed fixtures of tests/golden/match/ equal a fresh run of ``scripts/make_golden_match.py`` (development
  container only: needs the reference checkout).

Tolerance: 1e-5 relative to max(1, |reference|) -- SURVEY §8(c)'s per-layer figure for fp32 against fp64.
"""
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dualmessagepassing_amd import harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATCH = os.path.join(ROOT, "tests", "golden", "match")
REFERENCE = "/root/reference/SubgraphCountingMatching"
TOL = 1e-5


def close(got, ref, tol=TOL):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return bool(((got - ref).abs() <= tol * ref.abs().clamp(min=1.0)).all())


def make_inputs(B, L, seed, holes=True):
    """An unpadded batch as the model hands it over: ``pred`` [B, L] fp64, int64 ``weights``, a pre-padding ``mask`` with
    row sizes that include 0, 1 and L (one row always has L: L is the batch's largest size), an interior hole where the
    row is long enough (the reversed edges of the edge head), ``pred_c`` of both signs."""
    g = torch.Generator().manual_seed(seed)
    sizes = [L, min(3, L), 0, min(5, L), 1][:B]
    mask = torch.arange(L).view(1, -1) >= (L - torch.tensor(sizes)).view(-1, 1)
    if holes and L >= 4:
        mask[0, L - 2] = False
    pred = torch.randn(B, L, generator=g, dtype=torch.float64) * 2.0
    weights = torch.randint(0, 6, (B, L), generator=g)
    pred_c = torch.randn(B, 1, generator=g, dtype=torch.float64)
    pred_c[0, 0] = -pred_c[0, 0].abs() - 0.1            # both signs, whatever the seed drew
    if B > 1:
        pred_c[1, 0] = pred_c[1, 0].abs() + 0.1
    return pred, weights, mask, pred_c


def reference_terms(pred, weights, mask, pred_c, coef, bp):
    """``_match_terms`` on an fp32 copy -> (total, loss, reg, dpred, dpred_c), as train_epoch combines them."""
    p = pred.float().clone().requires_grad_(True)
    c = pred_c.float().clone().requires_grad_(True)
    loss, reg = harness._match_terms(harness._CRIT[bp], p, weights.clone(), mask.clone(), c, coef[0])
    total = coef[1] * loss + coef[2] * reg
    total.backward()
    return total, loss, reg, p.grad, c.grad


def tensor_terms(pred, weights, mask, pred_c, coef, bp, pair_weights=None):
    p, c = pred.clone().requires_grad_(True), pred_c.clone().requires_grad_(True)
    total, loss, reg = harness.match_terms_tensor(p, weights, mask, c, coef, bp, pair_weights)
    total.backward()
    return total, loss, reg, p.grad, c.grad


CASES = list(itertools.product((1, 5), (1, 7), ("MSE", "MAE", "SMSE"), (0.0, 0.01, 1.0)))


@pytest.mark.parametrize("B,L,bp,slope", CASES)
def test_tensor_definition_equals_the_reference_restatement(B, L, bp, slope):
    coef = (slope, 0.7, 0.3)
    pred, weights, mask, pred_c = make_inputs(B, L, seed=100 * B + L)
    ref = reference_terms(pred, weights, mask, pred_c, coef, bp)
    got = tensor_terms(pred, weights, mask, pred_c, coef, bp)
    for name, a, b in zip(("total", "loss", "reg", "dpred", "dpred_c"), got, ref):
        assert close(b, a), (name, a, b)             # (the fp64 value is the reference of the comparison)
    assert torch.equal(pred, make_inputs(B, L, seed=100 * B + L)[0])        # match_terms_tensor leaves pred alone


def test_masked_window_position_passes_the_regulariser_gradient():
    """``masked_fill_`` under ``no_grad`` is invisible to autograd: a masked position inside the window is x = 0, and with
    pred_c < 0 the regulariser's relu(0 - pred_c) is live there -- its gradient reaches ``pred``."""
    pred, weights, mask, pred_c = make_inputs(5, 7, seed=3)
    coef = (0.01, 1.0, 0.5)
    ref, got = reference_terms(pred, weights, mask, pred_c, coef, "MSE"), tensor_terms(pred, weights, mask, pred_c, coef, "MSE")
    assert not mask[0, 0 + 5] and pred_c[0, 0] < 0
    want = 0.5 * 2.0 * float(-pred_c[0, 0]) / 5
    assert abs(float(got[3][0, 5]) - want) <= TOL and abs(float(ref[3][0, 5]) - want) <= TOL and want > 0
    assert float(got[3][1, 0]) == 0.0                  # row 1: pred_c > 0, masked: nothing


@pytest.mark.parametrize("bp,slope", list(itertools.product(("MSE", "MAE", "SMSE"), (0.0, 0.01, 1.0))))
def test_padded_batch_gives_the_real_pairs_values_and_exact_zeros(bp, slope):
    coef = (slope, 0.7, 0.3)
    B, L, front, inert = 5, 7, 4, 3
    pred, weights, mask, pred_c = make_inputs(B, L, seed=11)
    exact = tensor_terms(pred, weights, mask, pred_c, coef, bp)
    g = torch.Generator().manual_seed(12)
    P = torch.randn(B + inert, front + L, generator=g, dtype=torch.float64)      # noise everywhere outside the real block
    W = torch.randint(0, 6, (B + inert, front + L), generator=g)
    M = torch.zeros(B + inert, front + L, dtype=torch.bool)
    C = -torch.rand(B + inert, 1, generator=g, dtype=torch.float64) - 0.5          # inert pred_c < 0: their relu(-c) would be live
    P[:B, front:], W[:B, front:], M[:B, front:], C[:B] = pred, weights, mask, pred_c
    M[B:, 1:] = True                                                               # inert pairs: live rows LONGER than the real ones
    pw = torch.tensor([1.0] * B + [0.0] * inert, dtype=torch.float64)
    got = tensor_terms(P, W, M, C, coef, bp, pair_weights=pw)
    for k in range(3):
        assert close(got[k], exact[k], 1e-12), k
    assert close(got[3][:B, front:], exact[3], 1e-12) and close(got[4][:B], exact[4], 1e-12)
    assert bool((got[3][:B, :front] == 0).all()) and bool((got[3][B:] == 0).all()) and bool((got[4][B:] == 0).all())
    assert bool((exact[3] != 0).any())


def test_no_real_pair_gives_zeros():
    pred, weights, mask, pred_c = make_inputs(5, 7, seed=5)
    got = tensor_terms(pred, weights, mask, pred_c, (0.01, 1.0, 1.0), "MSE", pair_weights=torch.zeros(5, dtype=torch.float64))
    for t in got:
        assert bool((t == 0).all()) and bool(torch.isfinite(t).all())


def test_match_terms_on_the_cpu_is_the_tensor_definition():
    pred, weights, mask, pred_c = make_inputs(5, 7, seed=9)
    a = harness.match_terms(pred, weights, mask, pred_c, (0.01, 1.0, 0.01), "SMSE")
    b = harness.match_terms_tensor(pred, weights, mask, pred_c, torch.tensor([0.01, 1.0, 0.01], dtype=torch.float64), "SMSE")
    assert all(torch.allclose(x, y, rtol=1e-12, atol=0) for x, y in zip(a, b))


def test_binary_auc_is_sklearns_for_binary_vectors():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(0)
    for n in (2, 7, 64):
        for _ in range(20):
            t, p = rng.random(n) < 0.4, rng.random(n) < 0.5
            if t.all() or not t.any():
                continue
            assert abs(harness.binary_auc(torch.from_numpy(t), torch.from_numpy(p)) - metrics.roc_auc_score(t, p)) <= 1e-12


def test_binary_auc_of_one_class_is_nan():
    assert math.isnan(harness.binary_auc(torch.ones(4), torch.tensor([1.0, 0.0, 1.0, 0.0])))
    assert math.isnan(harness.binary_auc(torch.zeros(4), torch.tensor([1.0, 0.0, 1.0, 0.0])))
    assert harness.binary_auc(torch.tensor([1.0, 0.0]), torch.tensor([1.0, 0.0])) == 1.0


def _toy_dataset():
    """Six pairs with made-up subisomorphism rows of 0, 1, 2, 5, 3, 0 rows (pattern nodes 2 .. 4)."""
    rng = np.random.default_rng(7)
    samples = []
    for i, (pn, gn, rows) in enumerate([(2, 5, 0), (3, 6, 1), (2, 4, 2), (4, 9, 5), (3, 7, 3), (2, 5, 0)]):
        pu, pv = np.arange(pn - 1), np.arange(1, pn)
        gu, gv = np.arange(gn - 1), np.arange(1, gn)
        z = lambda n: np.zeros(n, np.int64)
        samples.append({"pattern": harness.PairDataset._with_rev(pu, pv, z(pn), z(pn - 1), 8, 1),
                        "graph": harness.PairDataset._with_rev(gu, gv, z(gn), z(gn - 1), 16, 1), "counts": rows,
                        "subisomorphisms": rng.integers(0, gn, (rows, pn)).astype(np.int64)})
    return harness.PairDataset(samples, dict(p_nodes=4, p_edges=3, g_nodes=9, g_edges=8, n_vlabels=1, n_elabels=1))


def test_batch_arrays_lays_the_subisomorphism_rows_out_at_the_capacity():
    ds = _toy_dataset()
    lens = sorted((x["subisomorphisms"].size for x in ds.samples), reverse=True)
    assert ds.sub_capacity(3) == sum(lens[:3]) == 20 + 9 + 4 and ds.sub_capacity(100) == sum(lens) and ds.sub_capacity(0) == 0
    cap, idx = ds.sub_capacity(3), [1, 3, 0]
    plain = ds.batch_arrays(idx, "cpu")
    meta, tensors = ds.batch_arrays(idx, "cpu", subs=cap)
    assert meta == plain[0] and len(tensors) == len(plain[1]) + 2
    assert all(torch.equal(a, b) for a, b in zip(tensors, plain[1]))           # the other tensors are untouched
    flat, ptr = tensors[-2], tensors[-1]
    assert flat.dtype == ptr.dtype == torch.int64 and flat.shape == (cap,) and ptr.tolist() == [0, 3, 23, 23]
    want = np.concatenate([ds.samples[i]["subisomorphisms"].reshape(-1) for i in idx])
    assert np.array_equal(flat[:23].numpy(), want) and bool((flat[23:] == 0).all())
    # a padded batch: inert pairs have empty ranges, the last entry is the real total
    pad = ds.pad_buckets(3, levels=2)
    meta_p, tensors_p = ds.batch_arrays(idx, "cpu", pad=pad, subs=cap)
    assert tensors_p[-1].tolist() == [0, 3, 23, 23, 23, 23, 23] and torch.equal(tensors_p[-2], flat)
    assert tensors_p[-3].view(-1).tolist() == [1.0] * 3 + [0.0] * 3              # the pair weights keep their place
    # every batch of the dataset has the same two shapes
    assert {tuple(ds.batch_arrays(b, "cpu", subs=cap)[1][-2].shape) for b in ([0, 1, 2], [3, 4, 5], [5])} == {(cap,)}
    with pytest.raises(ValueError):
        ds.batch_arrays([3, 4, 2], "cpu", subs=cap - 1)
    empty = ds.batch_arrays([0, 5], "cpu", subs=0)[1]
    assert empty[-2].numel() == 0 and empty[-1].tolist() == [0, 0, 0]


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="needs the reference checkout (development container only)")
def test_committed_match_fixtures_equal_a_fresh_run_of_the_reference(tmp_path):
    env = dict(os.environ, DMP_GOLDEN_MATCH_OUT=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_golden_match.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    fresh = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    have = sorted(f for f in os.listdir(MATCH) if f.endswith(".npz"))
    assert fresh == have == ["eval_dmpnn_node.npz", "eval_dmpnn_node_edge.npz"]
    for f in have:
        with np.load(os.path.join(MATCH, f), allow_pickle=False) as a, np.load(os.path.join(tmp_path, f), allow_pickle=False) as b:
            assert sorted(a.files) == sorted(b.files), f
            for k in a.files:
                x, y = a[k], b[k]
                assert x.shape == y.shape and x.dtype == y.dtype, (f, k)
                if x.dtype.kind in "fc":
                    if x.size:
                        scale = max(1.0, float(np.abs(x).max()))
                        assert float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) <= 1e-6 * scale, (f, k)
                else:
                    assert x.tobytes() == y.tobytes(), (f, k)
