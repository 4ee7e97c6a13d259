"""Emit the matching-evaluation fixtures under tests/golden/match/ by running the REFERENCE's own ``evaluate_epoch``.

Runs only in the development container (needs the reference checkout): the reference's ``train.py`` / ``dataset.py`` /
models are imported over the DGL / numba / igraph stand-ins of ``oracle/ref_standin.py`` (read-only use of ``oracle/``:
``make_golden``'s sample generator, ``_FixedLoader`` and seeds), single threaded with deterministic algorithms, as
``scripts/make_golden_mem.py`` runs.  Outputs are data only.

    python scripts/make_golden_match.py        # writes tests/golden/match/*.npz  (DMP_GOLDEN_MATCH_OUT: elsewhere)

Fixtures
  eval_dmpnn_node.npz        train.py:847-1061 over 24 ragged pairs in batches of 8: a seeded DMPNN (add_rev, hid 16,
  eval_dmpnn_node_edge.npz   SumPredictNet heads with ``pred_return_weights`` node / node,edge; the zero-initialised last
                             layers of the heads perturbed as ``make_golden_mem._perturb_heads`` does).  Stored: the
                             samples, the ``state_dict``, ``pred_c``, the flat ``pred_v`` / ``pred_e`` and
                             ``node_weights`` / ``edge_weights`` (every pair's live positions back to back), per-pair
                             AE / SE / NED / EED and MAE, MSE, RMSE, MNED, MEED, AUC.
The generator asserts that no ``|pred_c|`` is below 1e-3 and that both classes of ``counts > 0`` occur, so the AUC (a
comparison of signs) is exact for any implementation within the fixtures' tolerance.
"""
import json
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.environ.get("DMP_GOLDEN_MATCH_OUT") or os.path.join(ROOT, "tests", "golden", "match")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import make_golden as MG   # noqa: E402  (its helpers; importing it sets one thread and deterministic algorithms)
import make_golden_mem as MM   # noqa: E402  (_perturb_heads)

th.set_num_threads(1)
th.use_deterministic_algorithms(True)

NUM_PAIRS, BATCH = 24, 8
MAX_NE, MAX_NEL = 64, 2          # the offsets of the reversed copies (train.py:299-327): edge ids + MAX_NE, labels + MAX_NEL


def model_config(return_weights):
    return dict(max_ngv=20, max_ngvl=2, max_nge=2 * MAX_NE, max_ngel=2 * MAX_NEL, max_npv=20, max_npvl=2, max_npe=2 * MAX_NE,
                max_npel=2 * MAX_NEL, base=2, hid_dim=16, share_emb_net=True, share_enc_net=True, share_rep_net=True,
                rep_residual=True, enc_net="Multihot", emb_net="Orthogonal", filter_net="ScalarFilter", rep_net="DMPNN",
                rep_num_graph_layers=2, rep_num_pattern_layers=2, rep_dmpnn_num_mlp_layers=2, rep_dmpnn_batch_norm=False,
                rep_act_func="relu", rep_dropout=0.0, init_neigenv=6.0, init_eeigenv=5.0, pred_net="SumPredictNet",
                pred_hid_dim=16, pred_act_func="relu", pred_dropout=0.0, node_pred=True, edge_pred=True,
                pred_return_weights=return_weights)


def samples():
    """24 ragged pairs with their exact subisomorphisms (``make_golden._ref_sample``), reversed edges added and degrees
    cached by the reference's own preprocessing."""
    import dataset as ref_dataset
    import train as ref_train
    rng = np.random.default_rng(MG.seed_of("match-eval", "samples"))
    ds, raws = ref_dataset.GraphAdjDataset(), []
    for i in range(NUM_PAIRS):
        pn = int(rng.integers(3, 6)); pm = int(rng.integers(pn - 1, min(8, pn * (pn - 1)) + 1))
        gn = int(rng.integers(8, 21)); gm = int(rng.integers(2 * gn, min(MAX_NE, gn * (gn - 1)) + 1))
        x, raw = MG._ref_sample(rng, "eval-%d" % i, pn, pm, gn, gm, 2, 2)
        ds.data.append(x)
        raws.append(raw)
    for x in ds:
        x["g_len"], x["p_len"] = len(x["graph"]), len(x["pattern"])
    ref_train.add_reversed_edges(ds, MAX_NE, MAX_NEL, MAX_NE, MAX_NEL)
    ref_train.calculate_degrees(ds)
    return ds, raws


def _flat(x):
    return x.detach().reshape(-1) if th.is_tensor(x) else th.zeros(0)


def gen(tag, return_weights):
    import train as ref_train
    from models.dmpnn import DMPNN
    ds, raws = samples()
    config = model_config(return_weights)
    batches = [list(range(i, min(i + BATCH, NUM_PAIRS))) for i in range(0, NUM_PAIRS, BATCH)]
    run = {"eval_metric": "MAE", "train_epochs": 1}
    for salt in range(32):      # the first seed whose untrained model predicts counts on both sides of 0 (an AUC that says something)
        th.manual_seed(MG.seed_of("match-eval", tag, salt))
        model = DMPNN(**config)
        MM._perturb_heads(model.pred_net.values())
        _, res = ref_train.evaluate_epoch(model, "dev", MG._FixedLoader(ds, batches, return_weights), th.device("cpu"), run, 0, None, None)
        pred_c, counts = _flat(res["prediction"]["pred_c"]), _flat(res["data"]["counts"])
        if 4 <= int((pred_c > 0).sum()) <= NUM_PAIRS - 4 and float(pred_c.abs().min()) >= 1e-3:
            break
    assert float(pred_c.abs().min()) >= 1e-3, "a pred_c too close to 0 for an exact AUC"
    assert 0 < int((counts > 0).sum()) < NUM_PAIRS, "one class only: the AUC is undefined"
    assert 0 < int((pred_c > 0).sum()) < NUM_PAIRS, "every prediction on one side of 0: the AUC says nothing"
    d = {"config_json": np.array(json.dumps(config, sort_keys=True)), "match_weights": np.array(return_weights), "batch": BATCH,
         "rev_max_ne": MAX_NE, "rev_max_nel": MAX_NEL, "n": NUM_PAIRS, "seed_salt": salt, "ids": np.array(res["data"]["id"]),
         "pred_c": pred_c, "counts": counts, "AE": _flat(res["error"]["AE"]), "SE": _flat(res["error"]["SE"])}
    for k in ("MAE", "MSE", "RMSE", "AUC", "MNED", "MEED"):
        d[k] = np.float64(res["error"][k])
    d["NED"], d["EED"] = _flat(res["error"]["NED"]), _flat(res["error"]["EED"])
    for part, keys in (("data", ("node_weights", "edge_weights")), ("prediction", ("pred_v", "pred_e"))):
        for k in keys:
            d[k] = _flat(res[part][k])
    for k, v in model.state_dict().items():
        d["sd." + k] = v.clone()
    for i, r in enumerate(raws):
        for k, v in r.items():
            d["%d.%s" % (i, k)] = v
    np.savez_compressed(os.path.join(OUT, "eval_dmpnn_%s.npz" % tag), **MG.t2n(d))
    print("wrote eval_dmpnn_%s.npz  MAE %.4f AUC %.4f MNED %.4f MEED %.4f  positives %d / %d predicted %d" % (
        tag, d["MAE"], d["AUC"], d["MNED"], d["MEED"], int((counts > 0).sum()), NUM_PAIRS, int((pred_c > 0).sum())))


def main():
    os.makedirs(OUT, exist_ok=True)
    import ref_standin
    ref_standin.import_scm()
    gen("node", "node")
    gen("node_edge", "node,edge")


if __name__ == "__main__":
    main()
