"""The joint counting-and-matching training step on the GPU: ``train_epoch``'s eager branch against the recorded step
(``GraphedTrainStep(match_weights=("node",))``) on the same batches in one process, and ``dmp_match_loss`` alone.

    python scripts/kbench_match.py                          # the step: eager against replayed, alternating windows
    python scripts/kbench_match.py --only replay --windows 2  # what a rocprofv3 --kernel-trace run counts launches on
    python scripts/kbench_match.py --kernel                 # dmp_match_loss at three shapes (event-timed; profile this run)
    python scripts/kbench_match.py --kernel --trace DIR     # kernel time and share of the HBM peak from DIR/*kernel_trace.csv
    python scripts/kbench_match.py --count DIR --only replay --windows 2   # kernel dispatches per step from DIR/*kernel_stats.csv

The step (the reference's README commands in miniature: ``--node_pred True --match_weights node``, match_loss_w 1,
match_reg_w 0.01): hid 64, 64 pairs per batch, patterns of 8 nodes / 12 edges planted in graphs of 64 nodes / 256 edges,
reversed edges added, three DMPNN layers, SumPredictNet with the node weight head, FlatAdamW.  Both ways run
``train_epoch`` over the same window of batches, each on its own copy of the model; times are device events around
windows that end in a synchronise, windows alternate between the two ways, both are warmed first.  The spread is the
range of a way's window times.

The kernel: 17 bytes per element (pred 4, weights 8, mask 1 read, dpred 4 written) against the HBM peak of 8 TB/s
(about 6.3 TB/s is what a streaming copy reaches on this part)."""
import argparse
import copy
import csv
import glob
import json
import os
import re
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES = 8e12
KERNEL_SHAPES = [(64, 128), (1024, 64), (1024, 512)]
KERNEL_WARMUP, KERNEL_ITERS = 3, 20


def window(fn, steps):
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    th.cuda.synchronize()
    a.record()
    fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b) / steps


def planted_pairs(num, seed=0, pn=8, pe=12, gn=64, ge=256, n_vlabels=4):
    """Uniform pairs with matches: a random pattern (``pn`` nodes, ``pe`` edges), and a graph of ``gn`` nodes / ``ge`` edges
    of ER noise into which one copy of the pattern is planted (its node labels written over the noise's, its edges among
    the graph's).  Plain ER pairs of this size have either no match at all or, with one label, millions."""
    from dualmessagepassing_amd import harness
    rng = np.random.default_rng(seed)
    shape = dict(p_nodes=pn, p_edges=pe, g_nodes=gn, g_edges=ge, n_vlabels=n_vlabels, n_elabels=1)
    samples = []
    for _ in range(num):
        pu, pv = harness._er_edges(pn, pe, rng)
        pvl, gvl = rng.integers(0, n_vlabels, pn), rng.integers(0, n_vlabels, gn)
        where = rng.choice(gn, size=pn, replace=False)
        gvl[where] = pvl
        edges = set(zip(where[pu].tolist(), where[pv].tolist()))
        while len(edges) < ge:
            u, v = int(rng.integers(0, gn)), int(rng.integers(0, gn))
            if u != v:
                edges.add((u, v))
        gu, gv = (np.array(x, np.int64) for x in zip(*sorted(edges)))
        pel, gel = np.zeros(pe, np.int64), np.zeros(ge, np.int64)
        sub = harness.enumerate_subisomorphisms(pu, pv, pvl, pel, gu, gv, gvl, gel)
        samples.append({"pattern": harness.PairDataset._with_rev(pu, pv, pvl, pel, pe, 1),
                        "graph": harness.PairDataset._with_rev(gu, gv, gvl, gel, ge, 1), "counts": len(sub), "subisomorphisms": sub})
    return harness.PairDataset(samples, shape)


def bench_step(a, dev):
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
    from dualmessagepassing_amd.harness import GraphedTrainStep, train_epoch
    B = 64
    ds = planted_pairs(B * a.batches)
    th.manual_seed(0)
    base = build_model(**ds.model_config(hid_dim=64, layers=3, pred_return_weights="node"))
    kw = dict(neg_slp=0.01, match_weights=("node",), match_loss_w=1.0, match_reg_w=0.01)
    runs = {}
    for way in ("eager", "replay"):
        if a.only not in (way, "both"):
            continue
        model = copy.deepcopy(base).to(dev)
        sync = FlatGradSync(model)
        opt = FlatAdamW([sync.flatten_parameters()], lr=1e-4, weight_decay=1e-5, amsgrad=True, capturable=True)
        step = GraphedTrainStep(model, opt, sync, match_weights=("node",)) if way == "replay" else None
        runs[way] = (lambda model=model, opt=opt, sync=sync, step=step:
                     train_epoch(model, opt, ds, B, dev, sync=sync, graph=step, **kw), step)
    res = {"batch": B, "batches_per_window": a.batches, "windows": a.windows, "subisomorphism_rows": int(sum(x["counts"] for x in ds.samples))}
    times = {way: [] for way in runs}
    replay = runs.get("replay")
    ctx = replay[1].steps.on_stream() if replay else None
    if ctx is not None:
        ctx.__enter__()
    try:
        for way, (fn, _) in runs.items():                   # warm-up: first launches, the recording
            for _ in range(a.warmup):
                fn()
        for _ in range(a.windows):                          # alternating
            for way, (fn, _) in runs.items():
                times[way].append(window(fn, a.batches))
    finally:
        if ctx is not None:
            ctx.__exit__(None, None, None)
    for way, ts in times.items():
        res[way] = {"ms_per_step_median": float(np.median(ts)), "ms_per_step_min": min(ts), "ms_per_step_max": max(ts),
                    "steps": len(ts) * a.batches}
    if replay:
        res["replay"]["replays"], res["replay"]["eager_calls"] = replay[1].steps.replays, replay[1].steps.eager_calls
    if len(times) == 2:
        spread = max(max(ts) - min(ts) for ts in times.values())
        res["spread_ms"] = spread
        res["speedup"] = res["eager"]["ms_per_step_median"] / res["replay"]["ms_per_step_median"]
        res["replay_not_slower"] = bool(res["replay"]["ms_per_step_median"] <= res["eager"]["ms_per_step_median"] + spread)
    return res


def kernel_inputs(B, Lc, dev):
    g = th.Generator(device=dev).manual_seed(B + Lc)
    sizes = th.randint(Lc // 2, Lc + 1, (B,), generator=g, device=dev)
    sizes[0] = Lc
    mask = th.arange(Lc, device=dev).view(1, -1) >= (Lc - sizes).view(-1, 1)
    pred = th.randn(B, Lc, generator=g, device=dev)
    weights = th.randint(0, 50, (B, Lc), generator=g, device=dev)
    return pred, weights, mask, th.randn(B, 1, generator=g, device=dev)


def bench_kernel(dev):
    from dualmessagepassing_amd.harness import match_terms
    coef = th.tensor([0.01, 1.0, 0.01], device=dev)
    out = []
    for B, Lc in KERNEL_SHAPES:
        pred, weights, mask, pred_c = kernel_inputs(B, Lc, dev)
        with th.no_grad():
            fn = lambda: match_terms(pred, weights, mask, pred_c, coef, "MSE")
            for _ in range(KERNEL_WARMUP):
                fn()
            ms = window(lambda: [fn() for _ in range(KERNEL_ITERS)], KERNEL_ITERS)
        out.append({"B": B, "Lc": Lc, "bytes": 17 * B * Lc, "call_us_events": ms * 1e3, "launches_per_call": 3})
    return out


def kernel_trace(trace_dir):
    """rocprofv3 --kernel-trace of a ``--kernel`` run: the ``match_*`` dispatches in start order are, per shape,
    (warm-up + timed) calls of three kernels each; the timed calls' summed kernel time against 17 B Lc bytes."""
    path = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    if not path:
        raise SystemExit("no *kernel_trace.csv under %s" % trace_dir)
    with open(path[-1]) as f:
        rows = [r for r in csv.DictReader(f) if "match_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per_shape = 3 * (KERNEL_WARMUP + KERNEL_ITERS)
    if len(rows) != per_shape * len(KERNEL_SHAPES):
        raise SystemExit("expected %d match_* dispatches, found %d" % (per_shape * len(KERNEL_SHAPES), len(rows)))
    out = []
    for k, (B, Lc) in enumerate(KERNEL_SHAPES):
        timed = rows[k * per_shape + 3 * KERNEL_WARMUP:(k + 1) * per_shape]
        by = {}
        for r in timed:
            name = re.search(r"match_\w+", r["Kernel_Name"]).group(0)
            by.setdefault(name, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        us = {name: float(np.median(v)) / 1e3 for name, v in by.items()}
        total = sum(us.values())
        out.append({"B": B, "Lc": Lc, "bytes": 17 * B * Lc, "kernel_us": us, "kernel_us_per_call": total,
                    "share_of_hbm_peak": 17 * B * Lc / PEAK_BYTES / (total * 1e-6) if total > 0 else None})
    return out


def dispatches_per_step(stats_dir, steps):
    """rocprofv3 --kernel-trace --stats of a ``--only eager`` / ``--only replay`` run: every kernel dispatch of the process
    (a replayed graph's kernel nodes are dispatches too) over the steps it ran, warm-up included."""
    path = sorted(glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not path:
        raise SystemExit("no *kernel_stats.csv under %s" % stats_dir)
    with open(path[-1]) as f:
        calls = sum(int(r["Calls"]) for r in csv.DictReader(f))
    return {"kernel_dispatches": calls, "steps": steps, "dispatches_per_step": calls / steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["eager", "replay", "both"], default="both")
    ap.add_argument("--batches", type=int, default=25, help="batches (steps) per window")
    ap.add_argument("--windows", type=int, default=8, help="timed windows per way")
    ap.add_argument("--warmup", type=int, default=2, help="warm-up windows per way")
    ap.add_argument("--kernel", action="store_true", help="time dmp_match_loss alone")
    ap.add_argument("--trace", help="directory of a rocprofv3 --kernel-trace run of `--kernel`")
    ap.add_argument("--count", help="directory of a rocprofv3 --kernel-trace --stats run with the same --only / --windows / --warmup")
    a = ap.parse_args()
    if a.count:
        print(json.dumps(dict(way=a.only, **dispatches_per_step(a.count, (a.warmup + a.windows) * a.batches))))
        return
    if a.kernel and a.trace:
        for r in kernel_trace(a.trace):
            print(json.dumps(r))
        return
    dev = th.device("cuda:0")
    if a.kernel:
        for r in bench_kernel(dev):
            print(json.dumps(r), flush=True)
        return
    print(json.dumps(bench_step(a, dev)), flush=True)


if __name__ == "__main__":
    main()
