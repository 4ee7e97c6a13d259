"""The type-constrained rank counts of the UNC link evaluation at PubMed's size (63,109 nodes; 20,000 triplets
ranked on both sides, Q = 40,000 queries), the twin of kbench_unc_rank.py.

    python scripts/kbench_unc_rank_typed.py                        # prints one JSON line
    python scripts/kbench_unc_rank_typed.py --out FILE             # ... and writes it to FILE
    python scripts/kbench_unc_rank_typed.py --parent_lib LIB.so    # ... with dmp_rank_counts of another build of the library

Per width, in one process, the arms taken in turn round after round, every call between its own pair of device events after
a warm-up of all of them, median / min / max over the rounds:

  (a) untyped            ``unc_eval.rank_counts`` (``dmp_rank_counts``), every node a candidate;
      untyped_parent     the same entry of ``--parent_lib`` (the library built from the parent commit), same buffers: the ratio
                         to (a) against the run-to-run spread of (a) itself says whether the typed kernel disturbed the untyped one;
  (b) typed_all          ``unc_eval.rank_counts_typed`` with every type admitted: what the mask path costs;
  (c) typed_one_of_four  four balanced types, every query admits one, candidates ordered by type and queries by mask as
                         ``link_ranks`` orders them: what stepping over the tiles of other types saves.  Its counts are
                         checked against (a)'s on the admitted quarter restated in tensor ops for a sample of the queries.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b), out


def spread(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=63109)
    ap.add_argument("--triplets", type=int, default=20000)
    ap.add_argument("--widths", type=int, nargs="+", default=[50, 64, 256])
    ap.add_argument("--types", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=9, help="rounds: timed calls per arm and width")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent_lib", help="a libdmp_hip.so built from the parent commit")
    ap.add_argument("--out")
    a = ap.parse_args()
    from dualmessagepassing_amd import _abi, _lib, unc_eval
    if not th.cuda.is_available():
        raise SystemExit("kbench_unc_rank_typed needs the GPU")
    dev = th.device("cuda:0")
    N, Q, T = a.nodes, 2 * a.triplets, a.types
    parent = None
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib)).dmp_rank_counts
        parent.restype, parent.argtypes = _abi.SIGNATURES["dmp_rank_counts"]
    res = {"nodes": N, "queries": Q, "types": T, "parent_lib": bool(parent), "widths": {}}
    for H in a.widths:
        gen = th.Generator(device=dev).manual_seed(H)
        query = th.randn(Q, H, device=dev, generator=gen)
        table = th.randn(N, H, device=dev, generator=gen)
        # candidates ordered by type, queries by mask: balanced types, a query admits the type of its target
        ctype = (th.arange(N, device=dev) * T // N).to(th.uint8)
        qtype = th.arange(Q, device=dev) * T // Q
        lo, hi = (qtype * N + T - 1) // T, ((qtype + 1) * N + T - 1) // T          # the nodes of type t: [ceil(t N / T), ceil((t + 1) N / T))
        target = lo + th.minimum((th.rand(Q, device=dev, generator=gen) * (hi - lo)).long(), hi - lo - 1)
        assert bool((ctype[target].long() == qtype).all())
        one, every = th.ones_like(qtype) << qtype, th.full_like(qtype, (1 << T) - 1)
        g0, e0 = th.empty(Q, dtype=th.int32, device=dev), th.empty(Q, dtype=th.int32, device=dev)
        arms = {"untyped": lambda: unc_eval.rank_counts(query, table, target),
                "typed_all": lambda: unc_eval.rank_counts_typed(query, table, target, ctype, every),
                "typed_one_of_four": lambda: unc_eval.rank_counts_typed(query, table, target, ctype, one)}
        if parent:
            arms["untyped_parent"] = lambda: _lib.check(parent(query.data_ptr(), table.data_ptr(), target.data_ptr(), None, None, 0, Q, N, H,
                                                               g0.data_ptr(), e0.data_ptr(), _lib.stream_ptr()), "parent dmp_rank_counts")
        for _ in range(a.warmup):
            for fn in arms.values():
                fn()
        th.cuda.synchronize()
        ms = {name: [] for name in arms}
        for _ in range(a.repeats):
            for name, fn in arms.items():
                t, out = timed(fn)
                ms[name].append(t)
                del out
        (g, e), (ga, ea, ca), (g1, e1, c1) = arms["untyped"](), arms["typed_all"](), arms["typed_one_of_four"]()
        sample = th.arange(0, Q, max(1, Q // 512), device=dev)
        gs, es, cs = unc_eval.rank_counts_typed_tensor(query[sample], table, target[sample], ctype, one[sample])
        entry = {name: spread(v) for name, v in ms.items()}
        base = entry["untyped"]["ms_median"]
        entry.update({
            "untyped_spread_max_over_min": entry["untyped"]["ms_max"] / entry["untyped"]["ms_min"],
            "typed_all_over_untyped": entry["typed_all"]["ms_median"] / base,
            "typed_one_of_four_over_untyped": entry["typed_one_of_four"]["ms_median"] / base,
            "admitted_fraction": float(c1.double().mean()) / (N - 1),
            "typed_all_equals_untyped": bool(th.equal(g, ga) and th.equal(e, ea) and bool((ca == N - 1).all())),
            # the tensor route rounds differently (the library's blocked product): compared, not asserted
            "sampled_queries": int(sample.numel()),
            "sampled_queries_with_other_counts": int(((g1[sample] != gs) | (e1[sample] != es)).sum()),
            "sampled_considered_equal": bool(th.equal(c1[sample], cs))})
        if parent:
            entry["untyped_over_parent"] = base / entry["untyped_parent"]["ms_median"]
            entry["parent_counts_equal"] = bool(th.equal(g, g0) and th.equal(e, e0))
        res["widths"][str(H)] = entry
        del query, table
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
