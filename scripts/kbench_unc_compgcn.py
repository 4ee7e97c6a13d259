"""UNC CompGCN (unc_compgcn.TrainModel) on the setup of scripts/kbench_unc.py: one Cora-sized graph (N = 2,708, 5,429 edges ->
10,858 directed, 2 edge types), 2 layers, hid 256 and hid 50; the SAMPLED mini-batch step after the sampling, eager and
padded + replayed (unc_harness.SampledStep), on the kernel path (dmp_relcorr_weights_* + dmp_relconv_*) and with the same
module forced onto its tensor-op path (``unc_compgcn.kernels_admit`` answering no)."""
import os, sys, time
import numpy as np, torch as th
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dualmessagepassing_amd import unc_compgcn
from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
from dualmessagepassing_amd.tuning import enable_tuned_gemms
from dualmessagepassing_amd.unc import build_graph_from_triplets
from dualmessagepassing_amd.unc_harness import SampledStep
from dualmessagepassing_amd.unc_sampling import generate_sampled_graph_and_labels_unsupervised
enable_tuned_gemms()
gpu = th.device("cuda:0")
rng = np.random.default_rng(5)
n, m = 2708, 5429
pick = rng.choice(n * (n - 1), size=m, replace=False)
u = pick // (n - 1); r = pick % (n - 1); v = r + (r >= u)
trip = np.stack([u, np.zeros(m, np.int64), v], 1)
g = build_graph_from_triplets(n, 1, trip, gpu)
trip_dev = th.from_numpy(trip).to(gpu)
B = int(os.environ.get("UNC_BATCH", "2000"))
IT, WARM = int(os.environ.get("UNC_ITERS", "20")), 10
admit = unc_compgcn.kernels_admit


def bench(h, kernels):
    unc_compgcn.kernels_admit = admit if kernels else (lambda *a: False)
    th.manual_seed(0)
    model = unc_compgcn.TrainModel(None, n, h, 1, 0, num_hidden_layers=2, dropout=0.0, reg_param=0.01).to(gpu)
    sync = FlatGradSync(model)
    master = sync.flatten_parameters()
    gen = th.Generator(device=gpu).manual_seed(3)

    def draw():
        idx = th.randint(0, m, (B,), device=gpu, generator=gen)
        return generate_sampled_graph_and_labels_unsupervised(g, trip_dev[idx], 6, 128, 0.5, 5, generator=gen, sampler="neighbor")

    def loop(stepper, opt):
        total = 0.0
        for k in range(WARM + IT):
            sub, smp, lab = draw()
            th.cuda.synchronize(); t0 = time.perf_counter()
            if stepper is None:
                sync.detach_grads()
                emb, _ = model(sub, sub.ndata["_ID"], sub.edata["type"], sub.edata["norm"])
                loss = model.get_unsupervised_loss(sub, emb, sub.edata["type"], smp, lab)
                loss.backward(); sync.pack(); th.nn.utils.clip_grad_norm_([master], 1.0); opt.step()
            else:
                stepper(sub, sub.edata["type"], smp, lab)
            th.cuda.synchronize()
            if k >= WARM: total += time.perf_counter() - t0
        return total / IT * 1e3

    eager_ms = loop(None, FlatAdamW([master], lr=1e-3, weight_decay=0.0))
    st = SampledStep(model, sync, FlatAdamW([master], lr=1e-3, weight_decay=0.0, capturable=True), 1.0)
    try:
        with st.steps.on_stream():
            replay_ms = loop(st, None)
        note = "replays %d, eager %d, shapes %d" % (st.steps.replays, st.steps.eager_calls, len(st.steps._graphs))
    except Exception as exc:                               # a host sync inside the step cannot be recorded
        replay_ms, note = float("nan"), "could not be recorded: %s: %s" % (type(exc).__name__, str(exc)[:200])
    sub, _, _ = draw()
    print("UNC CompGCN hid=%d %s path, SAMPLED step (batch %d edges: ~%d nodes / ~%d edges) after the sampling: eager %.3f ms, "
          "padded + replayed %.3f ms (%s)" % (h, "kernel" if kernels else "tensor-op", B, sub.number_of_nodes(), sub.number_of_edges(),
                                            eager_ms, replay_ms, note), flush=True)


for h in (256, 50):
    for kernels in (True, False):
        bench(h, kernels)
