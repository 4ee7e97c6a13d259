"""What the host side of a batch costs a training step, and what the device-resident dataset view saves of it.

The workload of scripts/kbench_train_ragged.py -- 1024 ragged pairs, 64 per batch, hid 64, 3 layers -- in two configurations:
``counts`` (its own random pairs, count loss only) and ``matching`` (``SmallLikePairs`` with every sample's subisomorphism
rows enumerated, both matching terms on: ``batch_arrays(subs=...)``).  In ONE process, per configuration, four kinds of run:

    host path  (``PairDataset.batch_arrays``: what the library did before the view)     eager | padded + replayed
    resident   (``PairDataset.resident``: one plan upload + one launch per batch)       eager | padded + replayed

The replayed runs are repeated three times, the two data paths alternating, so that their difference can be held against
their spread.  Per run: ms per step over epochs 1-3 (epoch 0 warms up and records), the wall time inside ``batch_arrays`` per
step (``perf_counter`` around the call; the device is synchronised before each epoch only, so this is host time plus whatever
the call's own blocking uploads wait for), uploads per step, the store's bytes.  Results: profiles/resident_kbench.json.

Run it under a time limit of its own, e.g. ``timeout -k 10 900 python scripts/kbench_train_resident.py``."""
import contextlib
import json
import os
import sys
import time

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dualmessagepassing_amd.basemodel import build_model                      # noqa: E402
from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync                  # noqa: E402
from dualmessagepassing_amd.harness import (GraphedTrainStep, PairDataset, SmallLikePairs, enumerate_subisomorphisms,  # noqa: E402
                                            train_epoch)
from dualmessagepassing_amd.tuning import enable_tuned_gemms                   # noqa: E402

S, B, EPOCHS, REPEATS = 1024, 64, 4, 3
NOTE = ("uploads_per_step_in_batch_arrays: on the view, the plans it sent (counted); on the host path, the number of tensors batch_arrays "
        "returns -- read off its code, where each of them is made by one .to(device) or one torch.tensor(device=...), not counted on the "
        "device.  An EAGER matching step uploads the batch's rows and their offsets once more in batchify (2 uploads, on both data paths).  "
        "The eager runs were made once each: they have no spread.")


def ragged_counts_pairs():
    """The dataset of scripts/kbench_train_ragged.py, sample for sample."""
    rng = np.random.default_rng(0)

    def er(n, m):
        pick = rng.choice(n * (n - 1), size=m, replace=False)
        u, r = pick // (n - 1), pick % (n - 1)
        return u.astype(np.int64), (r + (r >= u)).astype(np.int64)

    shape, samples = dict(p_nodes=8, p_edges=16, g_nodes=64, g_edges=256, n_vlabels=8, n_elabels=8), []
    for i in range(S):
        pn = int(rng.integers(3, 9)); pm = int(rng.integers(pn - 1, min(16, pn * (pn - 1)) + 1))
        gn = int(rng.integers(8, 65)); gm = int(rng.integers(gn, min(256, gn * (gn - 1)) + 1))
        pu, pv = er(pn, pm); gu, gv = er(gn, gm)
        samples.append({"id": "s%d" % i, "pattern": PairDataset._with_rev(pu, pv, rng.integers(0, 8, pn), rng.integers(0, 8, pm), 16, 8),
                        "graph": PairDataset._with_rev(gu, gv, rng.integers(0, 8, gn), rng.integers(0, 8, gm), 256, 8),
                        "counts": int(rng.integers(0, 5)), "subisomorphisms": np.zeros((0, pn), np.int64)})
    return PairDataset(samples, shape)


def ragged_matching_pairs(row_limit=512):
    """``SmallLikePairs`` with the rows of every sample (at most ``row_limit`` of them: a few planted patterns match tens of
    thousands of times, and the benchmark is about the batches, not about those)."""
    base, samples = SmallLikePairs(S, seed=0), []
    for x in base.samples:
        p, g = x["pattern"], x["graph"]
        pe, ge = len(p["src"]) // 2, len(g["src"]) // 2
        rows = enumerate_subisomorphisms(p["src"][:pe], p["dst"][:pe], p["vlabel"], p["elabel"][:pe],
                                         g["src"][:ge], g["dst"][:ge], g["vlabel"], g["elabel"][:ge], limit=row_limit)
        samples.append(dict(x, counts=len(rows), subisomorphisms=rows))
    return PairDataset(samples, base.shape)


class Clocked:
    """``dataset.batch_arrays`` with a host clock around it and a count of what it uploads."""

    def __init__(self, dataset):
        self.dataset, self.inner = dataset, dataset.batch_arrays
        self.seconds, self.calls, self.uploads = 0.0, 0, 0
        dataset.batch_arrays = self

    def __call__(self, *args, **kw):
        sent = getattr(self.dataset, "uploads", None)
        t0 = time.perf_counter()
        meta, tensors = self.inner(*args, **kw)
        self.seconds += time.perf_counter() - t0
        self.calls += 1
        # the view counts the plans it sends; the host path makes every tensor it returns by one upload of its own (read off its
        # code, not counted on the device: NOTE)
        self.uploads += len(tensors) if sent is None else self.dataset.uploads - sent
        return meta, tensors

    def reset(self):
        self.seconds, self.calls, self.uploads = 0.0, 0, 0

    def close(self):
        del self.dataset.batch_arrays


def run(dataset, matching, graphed, gpu):
    kw = dict(hid_dim=64, layers=3, rep_act_func="leaky_relu", pred_act_func="leaky_relu", emb_net="Equivariant")
    if matching:
        kw["pred_return_weights"] = "node,edge"
    th.manual_seed(0)
    model = build_model(**dataset.model_config(**kw)).to(gpu)
    sync = FlatGradSync(model)
    opt = FlatAdamW([sync.flatten_parameters()], lr=1e-3, weight_decay=1e-5, amsgrad=True, capturable=graphed)
    want = ("node", "edge") if matching else ()
    step = GraphedTrainStep(model, opt, sync, max_shapes=4, match_weights=want) if graphed else None
    coef = dict(match_loss_w=1.0, match_reg_w=0.01) if matching else {}
    clock, per_epoch, host_ms, uploads = Clocked(dataset), [], [], []
    try:
        with (step.steps.on_stream() if graphed else contextlib.nullcontext()):
            for epoch in range(EPOCHS):
                clock.reset()
                th.cuda.synchronize(); t0 = time.perf_counter()
                train_epoch(model, opt, dataset, B, gpu, sync=sync, neg_slp=0.01, order=np.random.default_rng(epoch).permutation(S),
                            match_weights=want, graph=step, **coef)
                th.cuda.synchronize(); dt = time.perf_counter() - t0
                per_epoch.append(dt / (S // B) * 1e3)
                host_ms.append(clock.seconds / max(1, clock.calls) * 1e3)
                uploads.append(clock.uploads / max(1, clock.calls))
    finally:
        clock.close()
    out = {"ms_per_step_by_epoch": [round(v, 4) for v in per_epoch], "ms_per_step": round(float(np.mean(per_epoch[1:])), 4),
           "batch_arrays_ms_per_step": round(float(np.mean(host_ms[1:])), 4), "uploads_per_step_in_batch_arrays": round(float(np.mean(uploads[1:])), 2)}
    if graphed:
        out["replays"], out["eager_calls"] = step.steps.replays, step.steps.eager_calls
    return out, step


def summarise(runs, name):
    """The summary of configuration ``name`` from its recorded runs: per data path and mode the mean over the repeats and their
    spread (largest minus smallest; None where a run was made once), then the replayed difference against both spreads."""
    pick = lambda path, mode, key: [r[key] for r in runs if r["config"] == name and r["path"] == path and r["mode"] == mode]
    summary = {"store_bytes": pick("resident", "eager", "store_bytes")[0]}
    for mode in ("eager", "padded+replayed"):
        for path in ("host", "resident"):
            ms = pick(path, mode, "ms_per_step")
            summary["%s %s" % (path, mode)] = {"ms_per_step": round(float(np.mean(ms)), 4), "runs": len(ms),
                                               "spread": round(float(max(ms) - min(ms)), 4) if len(ms) > 1 else None,
                                               "batch_arrays_ms_per_step": round(float(np.mean(pick(path, mode, "batch_arrays_ms_per_step"))), 4),
                                               "uploads_per_step_in_batch_arrays": pick(path, mode, "uploads_per_step_in_batch_arrays")[0]}
    h, v = summary["host padded+replayed"], summary["resident padded+replayed"]
    summary["replayed: host - resident ms_per_step"] = round(h["ms_per_step"] - v["ms_per_step"], 4)
    summary["replayed: difference exceeds both spreads"] = bool(abs(h["ms_per_step"] - v["ms_per_step"]) > max(h["spread"], v["spread"]))
    return summary


def main():
    """Many recorded runs in one process, so the process keeps to what ``dp.StepGraph`` asks of a loop that owns recordings,
    for its whole life: nothing runs on the default stream (the eager runs, the models' uploads and the recorded runs share ONE
    other stream, under which each run's ``on_stream()`` nests, as in ``harness.fit``), and no recording is destroyed while
    another is being made -- the cyclic collector is off (``fit`` freezes it), every run's step object is kept, and all of them
    are dropped at the end, after the device is idle."""
    import faulthandler
    import gc
    faulthandler.enable()
    enable_tuned_gemms()
    gpu = th.device("cuda:0")
    doc = {"workload": {"pairs": S, "batch": B, "hid_dim": 64, "layers": 3, "epochs_timed": "1-%d" % (EPOCHS - 1), "repeats": REPEATS},
           "note": NOTE, "runs": [], "summary": {}}
    sets = {"counts": ragged_counts_pairs(), "matching": ragged_matching_pairs()}
    kept = []
    with th.cuda.stream(th.cuda.Stream()):
        views = {name: ds.resident(gpu) for name, ds in sets.items()}
        gc.collect()
        gc.freeze()
        gc.disable()
        for name, ds in sets.items():
            paths = {"host": ds, "resident": views[name]}
            store = views[name].nbytes
            todo = [(path, False, 0) for path in paths] + [(path, True, repeat) for repeat in range(REPEATS) for path in paths]
            for path, graphed, repeat in todo:                                    # the replayed runs alternate: host, resident, host, ...
                res, step = run(paths[path], name == "matching", graphed, gpu)
                kept.append(step)
                r = dict(res, config=name, path=path, mode="padded+replayed" if graphed else "eager", repeat=repeat, store_bytes=store)
                doc["runs"].append(r)
                print(json.dumps(r), flush=True)
            summary = doc["summary"][name] = summarise(doc["runs"], name)
            print(json.dumps({name: summary}), flush=True)
    th.cuda.synchronize()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "resident_kbench.json")
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    del kept[:]
    gc.enable()
    gc.collect()
    th.cuda.synchronize()


if __name__ == "__main__":
    main()
