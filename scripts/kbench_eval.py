"""What a dev pass costs, launch by launch from Python and as recorded forwards (``harness.GraphedEvalStep``).

The bench's BASELINE configuration (bench.CFG: patterns of 8 nodes / 12 edges, targets of 64 nodes / 256 edges, reversed
edges added, the DMPNN of ``bench.model_config``: hid 128, 3 shared layers, node and edge heads) on a uniform dev set of 4096
random pairs, evaluated at 64-pair and at 1024-pair batches.  Per batch size, one ``evaluate_epoch`` pass in these forms:

    eager      (``evaluate_epoch`` as it was: ``batchify``, the model launch by launch, lists, one blocking copy)   plain | resident
    recorded   (``evaluate_epoch(graph=GraphedEvalStep)``: one graph replay per batch, one read at the end)         plain | resident
    recorded, collect=False   (the form ``fit(eval_graph=True)`` runs: the scalars only)                            plain | resident

and, with ``--parent TREE`` (a checkout of the parent commit with its library built), the eager pass on the plain dataset run
by the PARENT's package in a process of its own on the same box -- the figure the recorded pass is held against: it must be
no slower at either batch size.  Every time is the median of ``PASSES`` passes after ``WARMUP`` warm-up passes (which also make
the recordings), the device synchronised around each pass.  Results: profiles/eval_replay_kbench.json (``--out`` elsewhere).

Run it under a time limit of its own, e.g. ``timeout -k 10 600 python scripts/kbench_eval.py --parent ../parent``."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, BATCHES, WARMUP, PASSES = 4096, (64, 1024), 3, 21


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def dev_pairs(cfg, PairDataset):
    """``S`` uniform pairs at the bench's sizes: directed ER graphs, uniform labels, random small counts (the pass is timed,
    not scored)."""
    rng = np.random.default_rng(0)

    def er(n, m):
        pick = rng.choice(n * (n - 1), size=m, replace=False)
        u, r = pick // (n - 1), pick % (n - 1)
        return u.astype(np.int64), (r + (r >= u)).astype(np.int64)

    pn, pm, gn, gm, nl = cfg["p_nodes"], cfg["p_edges"], cfg["g_nodes"], cfg["g_edges"], cfg["p_labels"]
    shape, samples = dict(p_nodes=pn, p_edges=pm, g_nodes=gn, g_edges=gm, n_vlabels=nl, n_elabels=nl), []
    for i in range(S):
        pu, pv = er(pn, pm)
        gu, gv = er(gn, gm)
        samples.append({"id": "s%d" % i, "pattern": PairDataset._with_rev(pu, pv, rng.integers(0, nl, pn), rng.integers(0, nl, pm), pm, nl),
                        "graph": PairDataset._with_rev(gu, gv, rng.integers(0, nl, gn), rng.integers(0, nl, gm), gm, nl),
                        "counts": int(rng.integers(0, 5)), "subisomorphisms": np.zeros((0, pn), np.int64)})
    return PairDataset(samples, shape)


def median_ms(fn, th):
    times = []
    for k in range(WARMUP + PASSES):
        th.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        th.cuda.synchronize()
        if k >= WARMUP:
            times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3), "passes": len(times)}


def worker(tree, forms):
    """The measurements of ``forms`` with the package of ``tree``; one JSON line per (batch size, form)."""
    sys.path.insert(0, tree)
    import torch as th
    import bench
    from dualmessagepassing_amd import harness
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.tuning import enable_tuned_gemms
    import gc
    enable_tuned_gemms()
    gpu = th.device("cuda:0")
    cfg = dict(bench.CFG)
    ds = dev_pairs(cfg, harness.PairDataset)
    kept = []
    # nothing on the default stream, no recording destroyed while another is made (dp.StepGraph; kbench_train_resident.py)
    with th.cuda.stream(th.cuda.Stream()):
        th.manual_seed(0)
        model = build_model(**bench.model_config(cfg)).to(gpu)
        sets = {"plain": ds}
        if any("resident" in f for f in forms):
            sets["resident"] = ds.resident(gpu)
        gc.collect()
        gc.freeze()
        gc.disable()
        for B in BATCHES:
            for form in forms:
                kind, path = form.rsplit(" ", 1)
                data = sets[path]
                if kind == "eager":
                    fn = lambda: harness.evaluate_epoch(model, data, B, gpu)
                else:
                    step = harness.GraphedEvalStep(model)
                    kept.append(step)
                    collect = kind == "recorded"
                    fn = lambda: harness.evaluate_epoch(model, data, B, gpu, graph=step, collect=collect)
                res = dict(median_ms(fn, th), batch=B, form=form)
                if kind != "eager":
                    res["replays"], res["eager_calls"] = step.steps.replays, step.steps.eager_calls
                print("RESULT " + json.dumps(res), flush=True)
    th.cuda.synchronize()
    del kept[:]
    gc.enable()


def main():
    if "--worker" in sys.argv:
        return worker(arg("--tree"), arg("--forms").split(","))
    forms = ["eager plain", "eager resident", "recorded plain", "recorded resident", "recorded-scalars plain", "recorded-scalars resident"]
    jobs = [("this commit", ROOT, forms)]
    if arg("--parent"):
        jobs.insert(0, ("parent commit", os.path.abspath(arg("--parent")), ["eager plain"]))
    doc = {"workload": {"pairs": S, "batches": list(BATCHES), "config": "bench.CFG / bench.model_config (hid 128, 3 layers)",
                        "warmup_passes": WARMUP, "timed_passes": PASSES, "statistic": "median of the timed passes, ms per pass"},
           "runs": [], "condition": {}}
    for name, tree, fs in jobs:                    # one process after the other: the box is theirs alone in turn
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--tree", tree, "--forms", ",".join(fs)],
                             cwd=tree, stdout=subprocess.PIPE, text=True, check=True).stdout
        for line in out.splitlines():
            if line.startswith("RESULT "):
                doc["runs"].append(dict(json.loads(line[7:]), tree=name))
                print(json.dumps(doc["runs"][-1]), flush=True)
    pick = lambda tree, form, B: next((r["median_ms"] for r in doc["runs"] if (r["tree"], r["form"], r["batch"]) == (tree, form, B)), None)
    for B in BATCHES:
        against = "parent commit" if arg("--parent") else "this commit"
        eager = pick(against, "eager plain", B)
        rec = {f: pick("this commit", f, B) for f in forms if f.startswith("recorded")}
        doc["condition"]["batch %d" % B] = {
            "eager pass held against": against, "eager_ms": eager, "recorded_ms": rec,
            "recorded no slower than the eager pass": {f: bool(v <= eager) for f, v in rec.items()},
            "eager / recorded": {f: round(eager / v, 3) for f, v in rec.items()}}
    doc["condition"]["met"] = all(all(c["recorded no slower than the eager pass"].values()) for c in doc["condition"].values())
    print(json.dumps(doc["condition"]), flush=True)
    with open(arg("--out", os.path.join(ROOT, "profiles", "eval_replay_kbench.json")), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
