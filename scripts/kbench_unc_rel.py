"""R-GCN / R-GIN relational conv (unc_rel, dmp_relconv.hip) against the per-type composition that ``rgnn`` gives (edges
sorted by type, the per-type counts read to the host, one library GEMM per type), at widths 50 (the reference's run.sh
n_hidden) and 256, on a sub-graph that the reference's sampler settings (run.sh: randomwalk, graph_batch_size 10000,
sample_depth 3, sample_width 10, split 0.5, negative_sample 5) cut from a synthetic graph of 20,000 nodes and 10 relation
types (R = 20 edge types with the reversed copies).

Rows (JSON lines):
  layer     one RelGraphConv (tanh) forward + backward: HIP vs composition (the TypedIndex build included: UNC samples a
            new sub-graph every step, so the composition pays its host sync every step)
  kernel    dmp_relconv_fwd / dmp_relconv_bwd alone, with the bytes each must move (from the shapes) and the share of the
            MI355X's 8 TB/s that this is
  step      one TrainModel(encoder) training step on the padded sub-graph: eager vs replayed (SampledStep)

    python scripts/kbench_unc_rel.py > profiles/unc_rel_kbench.jsonl
"""
import json
import os
import sys
import time

import numpy as np
import torch as th

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dualmessagepassing_amd import _lib, rgnn, unc_rel                       # noqa: E402
from dualmessagepassing_amd.unc_harness import graph_of                     # noqa: E402
from dualmessagepassing_amd.unc_sampling import generate_sampled_graph_and_labels_unsupervised  # noqa: E402

gpu = th.device("cuda:0")
HBM = 8.0e12


def timeit(f, it=20, warm=3):
    for _ in range(warm):
        f()
    th.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(it):
        f()
    th.cuda.synchronize()
    return (time.perf_counter() - t) / it * 1e3


def emit(**row):
    print(json.dumps(row), flush=True)


def sampled_sub(num_nodes=20000, num_rels=10, num_trip=120000, seed=0):
    rng = np.random.default_rng(seed)
    u, v = rng.integers(0, num_nodes, num_trip), rng.integers(0, num_nodes, num_trip)
    keep = u != v
    trip = np.stack([u[keep], rng.integers(0, num_rels, int(keep.sum())), v[keep]], 1)
    graph, trip_d = graph_of(trip, num_nodes, num_rels, gpu)
    gen = th.Generator(device=gpu).manual_seed(seed)
    sub, samples, labels = generate_sampled_graph_and_labels_unsupervised(graph, trip_d[:10000], 3, 10, 0.5, 5, generator=gen,
                                                                          sampler="randomwalk")
    return graph, trip_d, sub, samples, labels


def composition(m, g, x, et, norm):
    """What rgnn gives for the same layer: type-sorted edges (a host sync for the counts), one GEMM per type, a segment sum."""
    tix = rgnn.TypedIndex(g.index(), et, m.num_rels)
    agg = rgnn.typed_linear_agg(x, m.relation_weights(), tix, norm)
    return th.tanh(agg + m.h_bias + x @ m.loop_weight)


def bench_layer(sub, width, R):
    from dualmessagepassing_amd.graph import BatchedGraph
    N, E = sub.number_of_nodes(), sub.number_of_edges()
    src, dst = sub.all_edges(form="uv", order="eid")
    et, norm = sub.edata["type"], sub.edata["norm"]
    th.manual_seed(0)
    m = unc_rel.RelGraphConv(width, width, R, activation=th.nn.Tanh()).to(gpu)
    x = th.randn(N, width, device=gpu, requires_grad=True)

    def hip():
        g = BatchedGraph(src, dst, N)
        m(g, x, et, norm).sum().backward()

    def comp():
        g = BatchedGraph(src, dst, N)
        composition(m, g, x, et, norm).sum().backward()

    with th.no_grad():
        g = BatchedGraph(src, dst, N)
        d = float((m(g, x, et, norm) - composition(m, g, x, et, norm)).abs().max())
    emit(row="layer", width=width, R=R, N=N, E=E, hip_ms=timeit(hip), composition_ms=timeit(comp), max_abs_diff=d)

    # the two kernels alone
    lib = _lib.load()
    g = BatchedGraph(src, dst, N)
    ix = g.index()
    P = unc_rel.padded_width(width)
    Y = th.randn(N, (R + 1) * P, device=gpu)
    out = th.empty(N, width, device=gpu)
    dY = th.empty_like(Y)
    nrm = norm.reshape(-1).contiguous()
    etc = et.contiguous()
    s = _lib.stream_ptr()
    fwd = lambda: lib.dmp_relconv_fwd(Y.data_ptr(), ix.in_ptr.data_ptr(), ix.in_ent.data_ptr(), ix.src32.data_ptr(),  # noqa: E731
                                      etc.data_ptr(), nrm.data_ptr(), m.h_bias.data_ptr(), N, R, 1, width, P, 1, out.data_ptr(), s)
    bwd = lambda: lib.dmp_relconv_bwd(out.data_ptr(), out.data_ptr(), ix.out_ptr.data_ptr(), ix.out_ent.data_ptr(),  # noqa: E731
                                      ix.dst32.data_ptr(), etc.data_ptr(), nrm.data_ptr(), N, R, 1, width, P, 1, dY.data_ptr(), s)
    t_f, t_b = timeit(fwd, 50), timeit(bwd, 50)
    idx = E * (4 + 4 + 8 + 4) + (N + 1) * 4
    b_f = E * P * 4 + N * P * 4 + N * width * 4 + idx               # typed source rows, loop block, output
    b_b = 2 * E * width * 4 + N * (R + 1) * P * 4 + 2 * N * width * 4 + idx   # dOut / out per edge, dY written, g of the loop
    emit(row="kernel", width=width, R=R, N=N, E=E, fwd_us=t_f * 1e3, bwd_us=t_b * 1e3, fwd_bytes=b_f, bwd_bytes=b_b,
         fwd_hbm_share=b_f / (t_f * 1e-3) / HBM, bwd_hbm_share=b_b / (t_b * 1e-3) / HBM)


def bench_step(sub, samples, labels, encoder, width, num_rels, num_nodes):
    from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
    from dualmessagepassing_amd.unc import TrainModel
    from dualmessagepassing_amd.unc_harness import SampledStep
    th.manual_seed(0)
    model = TrainModel(None, num_nodes, width, num_rels, 0, num_hidden_layers=2, dropout=0.2, reg_param=0.01, encoder=encoder).to(gpu)
    sync = FlatGradSync(model)
    master = sync.flatten_parameters()
    opt = FlatAdamW([master], lr=1e-3, weight_decay=0.0, capturable=True)
    step = SampledStep(model, sync, opt, 1.0)
    et = sub.edata["type"]
    t_e = timeit(lambda: step.eager(sub, et, samples, labels), 10)
    with step.steps.on_stream():
        t_r = timeit(lambda: step(sub, et, samples, labels), 10)
    emit(row="step", encoder=encoder, width=width, N=sub.number_of_nodes(), E=sub.number_of_edges(), eager_ms=t_e, replayed_ms=t_r,
         replays=step.steps.replays)


def main():
    graph, trip, sub, samples, labels = sampled_sub()
    for width in (50, 256):
        bench_layer(sub, width, 20)
    for encoder in ("RGCN", "RGIN"):
        for width in (50, 256):
            bench_step(sub, samples, labels, encoder, width, 10, graph.number_of_nodes())


if __name__ == "__main__":
    main()
