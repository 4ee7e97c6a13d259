"""What labelling costs: the host pool (``harness.count_subisomorphisms_batch`` at 16 threads, the path every dataset here was
labelled by) against the device search (``subiso.label_pairs``: range checks, the image in numpy, one upload, the launches,
one read, and the host fallback for pairs that come back incomplete), counts only and counts plus both weights.

Inputs:
    small       the raw pairs of ``SmallLikePairs(4096)`` (patterns of 3 / 4 / 8 nodes, graphs of 8 .. 64 nodes)
    large-like  ``--large N`` pairs (default 96): patterns of 3 / 4 / 8 / 16 nodes (a spanning tree plus extra edges, as
                SmallLikePairs draws them), graphs of 128 / 256 / 512 nodes with 4 edges per node, 8 labels, 0 .. 4 planted copies;
                measured one pattern size at a time, the host pool in a child under ``--host-limit`` seconds (default 60): the
                search places pattern nodes in id order, and at 8 / 16 nodes one pair can keep the host busy for minutes
    saturation  2048 pairs of 64 one-label nodes / 1536 edges with an 8-node path: one chunk of 64 items per pair, a full
                launch (131072 items) in which EVERY item spends its whole budget -- the launch the default budget is sized by

Every time is the median of the timed passes after warm-up passes, the device synchronised around each (the device path ends
in its own blocking read).  The trial rate is the difference of the trials of two saturation launches (a large and a small
budget) over the difference of their times, so that the upload and the read cancel; the budget default derived from it is the
largest power of two with  budget * 131072 items <= rate * 1 s.  The result file is rewritten after every stage, so a run
that is cut short leaves what it had measured.

    timeout -k 10 900 python scripts/kbench_subiso.py [--out profiles/subiso_device_kbench.json] [--large 96] [--host-limit 60]
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
THREADS, WARMUP, PASSES = 16, 2, 7


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def large_like(num, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(num):
        pn = int(rng.choice([3, 4, 8, 16]))
        pe = int({3: rng.choice([2, 4]), 4: rng.choice([4, 8]), 8: 8, 16: 16}[pn])
        gn = int(rng.choice([128, 256, 512]))
        ge, nl = 4 * gn, 8
        perm = rng.permutation(pn)
        pairs = set()
        for k in range(1, pn):
            a, b = int(perm[k]), int(perm[rng.integers(0, k)])
            pairs.add((a, b) if rng.random() < 0.5 else (b, a))
        while len(pairs) < pe:
            a, b = int(rng.integers(0, pn)), int(rng.integers(0, pn))
            if a != b:
                pairs.add((a, b))
        pu, pv = (np.array(x, np.int64) for x in zip(*sorted(pairs)))
        pvl, pel = rng.integers(0, nl, pn), rng.integers(0, nl, len(pu))
        gvl = rng.integers(0, nl, gn)
        edges = {}
        for _c in range(int(rng.integers(0, 5))):
            where = rng.choice(gn, size=pn, replace=False)
            gvl[where] = pvl
            for u, v, l in zip(pu, pv, pel):
                edges[(int(where[u]), int(where[v]))] = int(l)
        while len(edges) < ge:
            a, b = int(rng.integers(0, gn)), int(rng.integers(0, gn))
            if a != b and (a, b) not in edges:
                edges[(a, b)] = int(rng.integers(0, nl))
        keys = sorted(edges)[:ge]
        gu, gv = (np.array(x, np.int64) for x in zip(*keys))
        out.append((pu, pv, pvl, pel, gu, gv, gvl, np.array([edges[k] for k in keys], np.int64)))
    return out


def saturation_pairs(num=2048, seed=0):
    rng = np.random.default_rng(seed)
    z = lambda n: np.zeros(n, np.int64)
    out = []
    for _ in range(num):
        pick = rng.choice(64 * 63, size=1536, replace=False)
        u, r = pick // 63, pick % 63
        out.append((np.arange(7), np.arange(1, 8), z(8), z(7), u.astype(np.int64), (r + (r >= u)).astype(np.int64), z(64), z(1536)))
    return out


def timed(fn, sync, warmup=WARMUP, passes=PASSES):
    times, last = [], None
    for k in range(warmup + passes):
        sync()
        t0 = time.perf_counter()
        last = fn()
        sync()
        if k >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(times)), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3),
            "passes": len(times)}, last


def host_worker():
    """The host pool alone on the large-like pairs of one pattern size, in a process of its own (the parent limits its time)."""
    from dualmessagepassing_amd import harness
    pairs = [p for p in large_like(int(arg("--large"))) if len(p[2]) == int(arg("--pn"))]
    t0 = time.perf_counter()
    counts = harness.count_subisomorphisms_batch(pairs, THREADS)
    print(json.dumps({"ms": round((time.perf_counter() - t0) * 1e3, 3), "counts": counts.tolist()}), flush=True)


def main():
    if "--host-worker" in sys.argv:
        return host_worker()
    import torch as th
    from dualmessagepassing_amd import harness, subiso
    if not th.cuda.is_available():
        raise SystemExit("kbench_subiso.py measures on the GPU: none is visible")
    gpu = th.device("cuda:0")
    out_path = arg("--out", os.path.join(ROOT, "profiles", "subiso_device_kbench.json"))
    doc = {"workload": {"host_threads": THREADS, "warmup_passes": WARMUP, "timed_passes": PASSES,
                        "statistic": "median of the timed passes, ms per pass; device times include the range checks, the image, "
                                     "the upload, the final read and the host fallback", "device": th.cuda.get_device_name(0)},
           "budget_in_use": subiso.DEFAULT_BUDGET, "stages": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    sync = th.cuda.synchronize
    # ---- the launch the budget is sized by: every item spends its whole budget
    sat = saturation_pairs()
    image = subiso.build_image(*subiso._flatten(sat))
    items = int(image["num_chunks"]) * 64
    rates = {}

    def saturated(b0):
        walls = []
        for k in range(1 + 3):                       # one warm-up, three timed
            sync()
            t0 = time.perf_counter()
            res = subiso.launch(image, gpu, (), b0)
            if k:
                walls.append((time.perf_counter() - t0) * 1e3)
        rates[b0] = {"wall_ms": round(float(np.median(walls)), 3), "trials": int(res["trials"].sum()),
                     "incomplete_pairs": int((~res["complete"]).sum())}
        return rates[b0]

    lo, hi = saturated(256), saturated(4096)
    b_hi = 4096
    while hi["wall_ms"] - lo["wall_ms"] < 100.0 and b_hi < 65536:      # until the search itself is most of the difference
        b_hi *= 4
        hi = saturated(b_hi)
    rate = (hi["trials"] - lo["trials"]) / (max(hi["wall_ms"] - lo["wall_ms"], 1e-3) * 1e-3)
    budget = 1
    while budget * 2 * subiso.ITEMS_PER_LAUNCH <= rate and budget * 2 <= subiso.MAX_BUDGET:
        budget *= 2
    doc["stages"]["saturation"] = {"pairs": len(sat), "items": items, "launches": rates,
                                   "method": "wall time of upload + launches + read at the largest budget minus the same at budget 256 (the "
                                             "fixed costs cancel), over the difference of the trials made",
                                   "trials_per_second": round(rate), "derived_default_budget": budget,
                                   "full_launch_at_derived_budget_s": round(budget * subiso.ITEMS_PER_LAUNCH / rate, 3)}
    print(json.dumps(doc["stages"]["saturation"]), flush=True)
    save()

    def stage(name, pairs, passes=PASSES):
        st = {"pairs": len(pairs)}
        doc["stages"][name] = st
        for label, w in (("device counts", ()), ("device counts + weights", ("node", "edge"))):
            st[label], res = timed(lambda: subiso.label_pairs(pairs, gpu, weights=w, threads=THREADS), sync, passes=passes)
            st[label]["fallback_pairs"] = res["fallback"]
            st[label]["trials"] = int(res["trials"][res["complete"]].sum())
            print(name, label, json.dumps(st[label]), flush=True)
            save()
        st["device launch only (no fallback)"], raw = timed(lambda: subiso.launch(subiso.build_image(*subiso._flatten(pairs)), gpu, ()), sync,
                                                           passes=passes)
        save()
        st["host pool counts"], want = timed(lambda: harness.count_subisomorphisms_batch(pairs, THREADS), lambda: None, warmup=1, passes=passes)
        st["counts equal"] = bool(np.array_equal(want, res["counts"]))
        st["host / device (counts)"] = round(st["host pool counts"]["median_ms"] / st["device counts"]["median_ms"], 3)
        st["device wins"] = bool(st["device counts"]["median_ms"] < st["host pool counts"]["median_ms"])
        print(name, "host", json.dumps(st["host pool counts"]), "equal", st["counts equal"], flush=True)
        save()

    small = harness.SmallLikePairs(4096, seed=0, threads=THREADS)
    raw = []
    for x in small.samples:
        p, g = x["pattern"], x["graph"]
        h = lambda a: np.asarray(a[:len(a) // 2], np.int64)
        raw.append((h(p["src"]), h(p["dst"]), np.asarray(p["vlabel"], np.int64), h(p["elabel"]), h(g["src"]), h(g["dst"]),
                    np.asarray(g["vlabel"], np.int64), h(g["elabel"])))
    stage("small", raw)

    # ---- large-like, one pattern size at a time.  The search places the pattern's nodes in id order, which for these
    # patterns is not a connected order: at 8 and 16 nodes the host search of a single pair can run for minutes or longer,
    # and so would the fallback of a pair whose item ran out of budget.  So: the device launch alone first (bounded by the
    # budget), the whole of label_pairs only where no pair fell back, and the host pool in a child under a time limit.
    num, limit = int(arg("--large", "96")), float(arg("--host-limit", "60"))
    everything = large_like(num)
    for pn in (3, 4, 8, 16):
        pairs = [p for p in everything if len(p[2]) == pn]
        st = {"pairs": len(pairs), "pattern_nodes": pn}
        doc["stages"]["large-like pn=%d" % pn] = st
        image = subiso.build_image(*subiso._flatten(pairs))
        st["device launch only (no fallback)"], res = timed(lambda: subiso.launch(image, gpu, ()), sync, warmup=1, passes=3)
        st["incomplete_pairs"] = int((~res["complete"]).sum())
        st["trials_of_complete_pairs"] = int(res["trials"][res["complete"]].sum())
        save()
        if st["incomplete_pairs"] == 0:
            for label, w in (("device counts", ()), ("device counts + weights", ("node", "edge"))):
                st[label], full = timed(lambda: subiso.label_pairs(pairs, gpu, weights=w, threads=THREADS), sync, warmup=1, passes=3)
                st[label]["fallback_pairs"] = full["fallback"]
        else:
            st["device counts"] = st["device counts + weights"] = \
                "not measured: %d pairs ran out of budget and their host fallback is the host search below" % st["incomplete_pairs"]
        save()
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--host-worker", "--large", str(num), "--pn", str(pn)],
                                 stdout=subprocess.PIPE, text=True, timeout=limit, check=True).stdout
            host = json.loads(out.strip().splitlines()[-1])
            st["host pool counts"] = {"ms": host["ms"], "passes": 1}
            st["counts equal on complete pairs"] = bool(np.array_equal(np.array(host["counts"])[res["complete"]], res["counts"][res["complete"]]))
            if isinstance(st["device counts"], dict):
                st["host / device (counts)"] = round(host["ms"] / st["device counts"]["median_ms"], 3)
        except subprocess.TimeoutExpired:
            st["host pool counts"] = "not measured: the host pool at %d threads did not finish these %d pairs within %g s" % (THREADS, len(pairs), limit)
        print("large-like pn=%d" % pn, json.dumps(st), flush=True)
        save()
    print(json.dumps(doc), flush=True)


if __name__ == "__main__":
    main()
