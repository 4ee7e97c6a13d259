"""The rank counts of the UNC link evaluation at PubMed's size (63,109 nodes): 20,000 triplets ranked on both
sides (Q = 40,000 queries) against every node, widths 50 (the shipped one), 64 and 256.

    python scripts/kbench_unc_rank.py                  # prints one JSON line
    python scripts/kbench_unc_rank.py --out FILE       # ... and writes it to FILE

Per width, in one process, alternating: the kernel (``unc_eval.rank_counts`` -> ``dmp_rank_counts``) and the tensor-op
restatement (``unc_eval.rank_counts_tensor`` with a 1 GiB score budget), every call between its own pair of device
events after a warm-up of both, median over the repeats.  The FLOP rate is 2 Q N H over the kernel's time against the
peak of its arithmetic, the f32-input MFMA (157.3 TFLOP/s, MI355X).  Peak extra memory: the rise of
``torch.cuda.max_memory_allocated`` over one call above what was allocated before it (the outputs included).  The two
routes round differently (one fmaf chain against the library's blocked product), so their counts are compared and the
number of queries that differ is reported, not asserted.  A second kernel timing carries a filter of ``--filter_avg`` known
candidates per query on average."""
import argparse
import json
import os
import sys

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TFLOPS = 157.3


def timed(fn):
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b), out


def peak_extra_mib(fn):
    th.cuda.synchronize()
    before = th.cuda.memory_allocated()
    th.cuda.reset_peak_memory_stats()
    out = fn()
    th.cuda.synchronize()
    peak = (th.cuda.max_memory_allocated() - before) / 2 ** 20
    del out
    return peak


def spread(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "repeats": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=63109)
    ap.add_argument("--triplets", type=int, default=20000)
    ap.add_argument("--widths", type=int, nargs="+", default=[50, 64, 256])
    ap.add_argument("--repeats", type=int, default=9, help="timed calls per route and width")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--budget_gib", type=float, default=1.0, help="score budget of the tensor route")
    ap.add_argument("--filter_avg", type=int, default=8)
    ap.add_argument("--out")
    a = ap.parse_args()
    from dualmessagepassing_amd import unc_eval
    if not th.cuda.is_available():
        raise SystemExit("kbench_unc_rank needs the GPU")
    dev = th.device("cuda:0")
    N, Q = a.nodes, 2 * a.triplets
    budget = int(a.budget_gib * 2 ** 30)
    res = {"nodes": N, "queries": Q, "tensor_budget_gib": a.budget_gib, "arithmetic": "f32-input MFMA (v_mfma_f32_32x32x2_f32)",
           "peak_tflops": F32_MFMA_PEAK_TFLOPS, "widths": {}}
    for H in a.widths:
        gen = th.Generator(device=dev).manual_seed(H)
        query = th.randn(Q, H, device=dev, generator=gen)
        table = th.randn(N, H, device=dev, generator=gen)
        target = th.randint(0, N, (Q,), device=dev, generator=gen)
        counts = th.randint(0, 2 * a.filter_avg + 1, (Q,), device=dev, generator=gen)
        ptr = th.zeros(Q + 1, dtype=th.int64, device=dev)
        ptr[1:] = th.cumsum(counts, 0)
        nnz = int(ptr[-1])
        rows = th.repeat_interleave(th.arange(Q, device=dev), counts, output_size=nnz)
        pairs = th.unique(rows * N + th.randint(0, N, (nnz,), device=dev, generator=gen))      # sorted by (row, candidate)
        idx = pairs % N
        ptr = th.searchsorted(pairs, th.arange(Q + 1, device=dev) * N)
        kernel = lambda: unc_eval.rank_counts(query, table, target)
        kernel_f = lambda: unc_eval.rank_counts(query, table, target, ptr, idx)
        tensor = lambda: unc_eval.rank_counts_tensor(query, table, target, budget_bytes=budget)
        for _ in range(a.warmup):
            kernel(), kernel_f(), tensor()
        th.cuda.synchronize()
        ms = {"kernel": [], "kernel_filtered": [], "tensor": []}
        for _ in range(a.repeats):
            for name, fn in (("kernel", kernel), ("kernel_filtered", kernel_f), ("tensor", tensor)):
                t, out = timed(fn)
                ms[name].append(t)
                del out
        (g, e), (g2, e2) = kernel(), tensor()
        flops = 2.0 * Q * N * H
        k_med = float(np.median(ms["kernel"]))
        entry = {"kernel": spread(ms["kernel"]), "kernel_filtered": spread(ms["kernel_filtered"]), "tensor": spread(ms["tensor"]),
                 "filter_entries": int(idx.numel()),
                 "kernel_tflops": flops / (k_med * 1e-3) / 1e12,
                 "kernel_share_of_f32_mfma_peak": flops / (k_med * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS,
                 "tensor_over_kernel": float(np.median(ms["tensor"])) / k_med,
                 "kernel_peak_extra_mib": peak_extra_mib(kernel), "tensor_peak_extra_mib": peak_extra_mib(tensor),
                 "queries_with_other_counts": int(((g != g2) | (e != e2)).sum()),
                 "largest_count_difference": int(th.maximum((g - g2).abs().max(), (e - e2).abs().max()))}
        res["widths"][str(H)] = entry
        del query, table, g, e, g2, e2
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
