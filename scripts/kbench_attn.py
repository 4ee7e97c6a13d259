"""Attention prediction heads on the GPU: the HIP sparsemax attention (csrc/dmp_attn.hip) against the tensor-op path
(``attn.attention_tensor``: padded [B, Lq, Lk, heads] scores, sort-based sparsemax), in one process.

    python scripts/kbench_attn.py                         # every shape, both paths, and the DMPNN step
    python scripts/kbench_attn.py --only hip --shape edge2 --iters 3   # what a rocprofv3 run profiles
    python scripts/kbench_attn.py --stats DIR --shape edge2 --iters 3  # share of peak from DIR/*kernel_stats.csv

Shapes (SumAttnPredictNet forward + backward, pred_hid_dim 64, 4 heads, 3 inference steps, input width 128):
  node2  config 2's node head: B 1024, Lg 64, Lp 8
  edge2  config 2's edge head: B 1024, Lg 512, Lp 24, the reversed half of both sides masked
  node4  config 4's node head: B 1024, Lg 512, Lp 16
and a DMPNN step (bench.py's config 2 model: forward, count loss, backward) with SumAttnPredictNet against SumPredictNet.
Where the tensor-op path runs out of memory the line says so.  Kernel shares of peak: MFMA-rate FLOPs over 157 TF/s or
bytes over 8 TB/s, whichever bound is larger (fp32 vector and fp32 MFMA peaks are equal on gfx950)."""
import argparse
import glob
import json
import os
import sys

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS, PEAK_BYTES = 157e12, 8e12
SHAPES = {"node2": dict(B=1024, Lg=64, Lp=8, half=False), "edge2": dict(B=1024, Lg=512, Lp=24, half=True),
          "node4": dict(B=1024, Lg=512, Lp=16, half=False)}
D, HID, NH, STEPS = 128, 64, 4, 3


def inputs(shape, dev, seed=0):
    g = th.Generator(device=dev).manual_seed(seed)
    B, Lg, Lp = shape["B"], shape["Lg"], shape["Lp"]

    def mask(L):
        m = th.zeros(B, L, dtype=th.bool, device=dev)
        if shape["half"]:
            m[:, : L // 2] = True          # the edge head: forward edges live, their reversed copies masked
        else:
            lens = th.randint(L // 2, L + 1, (B,), generator=g, device=dev)
            m = th.arange(L, device=dev).unsqueeze(0) >= (L - lens).unsqueeze(1)    # pre_pad
        return m
    pm, gm = mask(Lp), mask(Lg)
    p = th.randn(B, Lp, D, generator=g, device=dev) * pm.unsqueeze(-1)
    x = th.randn(B, Lg, D, generator=g, device=dev) * gm.unsqueeze(-1)
    return p, pm, x, gm


def head_step(head, p, pm, x, gm):
    p, x = p.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y, _ = head(p, pm, x, gm)
    y.sum().backward()
    return [y.detach(), p.grad, x.grad] + [q.grad.clone() for q in head.parameters()]


def timed(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    th.cuda.synchronize()
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    th.cuda.synchronize()
    return a.elapsed_time(b) / iters


class tensor_path:
    """Route the attention through the tensor ops (``attn.kernel_ok`` -> False) inside the block."""

    def __enter__(self):
        from dualmessagepassing_amd import attn
        self.attn, self.orig = attn, attn.kernel_ok
        attn.kernel_ok = lambda *a: False

    def __exit__(self, *exc):
        self.attn.kernel_ok = self.orig
        return False


def max_rel_diff(a, b):
    return max(float((x - y).abs().max()) / max(1.0, float(y.abs().max())) for x, y in zip(a, b))


def attn_calls(shape):
    """(Lq, Lk) of every attention call of one head forward: infer_steps x (graph rows -> pattern rows, graph -> graph)."""
    return [(shape["Lg"], shape["Lp"]), (shape["Lg"], shape["Lg"])] * STEPS


def kernel_work(shape):
    """kernel -> (FLOPs, bytes) of one head forward + backward: fmaf work of csrc/dmp_attn.hip counted at 2 FLOPs.
    forward: q.k and p.v per (row, key) -> 4 dh; rows kernel: two passes of q.k and dO.v plus dS.k -> 10 dh;
    keys kernel: q.k, dO.v, dS.q, p.dO -> 8 dh (per head, row, key).  Bytes: the Q / K / V / O / gradient rows read and
    written once per launch."""
    B, dh = shape["B"], HID // NH
    out = {"attn_fwd_kernel": [0.0, 0.0], "attn_bwd_rows_kernel": [0.0, 0.0], "attn_bwd_keys_kernel": [0.0, 0.0]}
    for Lq, Lk in attn_calls(shape):
        pairs = B * NH * Lq * Lk * dh
        rows, keys = B * Lq * HID * 4, B * Lk * HID * 4
        out["attn_fwd_kernel"][0] += 4 * pairs
        out["attn_fwd_kernel"][1] += 2 * rows + 2 * keys
        out["attn_bwd_rows_kernel"][0] += 10 * pairs
        out["attn_bwd_rows_kernel"][1] += 3 * rows + 2 * keys
        out["attn_bwd_keys_kernel"][0] += 8 * pairs
        out["attn_bwd_keys_kernel"][1] += 2 * rows + 4 * keys
    return out


def bench_head(name, iters, only, dev):
    from dualmessagepassing_amd.pred import SumAttnPredictNet
    shape = SHAPES[name]
    th.manual_seed(0)
    head = SumAttnPredictNet(D, HID, num_heads=NH, infer_steps=STEPS).to(dev)
    with th.no_grad():
        head.pred_fc2.weight.uniform_(-0.3, 0.3)
    p, pm, x, gm = inputs(shape, dev)
    res = {"shape": name, **{k: v for k, v in shape.items()}, "hid": HID, "heads": NH, "infer_steps": STEPS}

    def run():
        head.zero_grad(set_to_none=True)
        return head_step(head, p, pm, x, gm)
    hip = run()
    res["hip_ms"] = timed(run, iters)
    if only != "hip":
        try:
            with tensor_path():
                ten = run()
                res["tensor_ms"] = timed(run, iters)
            # the count is continuous in the scores; gradients jump where fp32 rounding moves a key across a row's threshold
            res["max_rel_diff_count"] = max_rel_diff(hip[:1], ten[:1])
            res["max_rel_diff_grads"] = max_rel_diff(hip[1:], ten[1:])
            res["speedup"] = res["tensor_ms"] / res["hip_ms"]
            del ten
        except th.cuda.OutOfMemoryError as e:
            res["tensor_ms"] = None
            res["tensor_note"] = "tensor-op path does not fit in HBM: %s" % str(e).splitlines()[0][:160]
        th.cuda.empty_cache()
    work = kernel_work(shape)
    res["gflop_per_step"] = sum(w[0] for w in work.values()) / 1e9
    return res


def bench_step(iters, dev):
    import bench
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.collate import collate_device
    from dualmessagepassing_amd.harness import count_loss
    cfg = dict(bench.CFG)
    shard = bench.make_shard(cfg, 0, dev)
    graphs = {}
    for tag in ("p", "g"):
        s = shard[tag]
        graphs[tag] = collate_device(s["local_src"], s["local_dst"], s["num_nodes"], s["num_edges"], s["N"], s["E"], ndata=s["ndata"],
                                     edata=s["edata"], max_nodes=s["max_n"], max_edges=s["max_e"])
    out = {}
    for head in ("SumPredictNet", "SumAttnPredictNet"):
        mc = bench.model_config(cfg)
        mc.update(pred_net=head, pred_hid_dim=HID, pred_num_heads=NH, pred_infer_steps=STEPS)
        th.manual_seed(3)
        model = build_model(**mc).to(dev)

        def step():
            model.zero_grad(set_to_none=True)
            o = model(graphs["p"], graphs["g"])
            count_loss(o["pred_c"].view(-1), shard["counts"]).backward()
        out[head + "_ms"] = timed(step, iters, warmup=2)
        del model
        th.cuda.empty_cache()
    out["attn_over_pool"] = out["SumAttnPredictNet_ms"] / out["SumPredictNet_ms"]
    return out


def share_of_peak(stats_dir, name, iters):
    """Read rocprofv3's kernel stats of a ``--only hip --shape name --iters iters`` run (1 warm-up + 1 check + iters timed
    head steps) and rate every attention kernel against the larger of its FLOP and byte bounds."""
    path = sorted(glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not path:
        raise SystemExit("no *kernel_stats.csv under %s" % stats_dir)
    import csv
    steps = iters + 2
    work = kernel_work(SHAPES[name])
    rows = []
    with open(path[-1]) as f:
        for r in csv.DictReader(f):
            for k, (fl, by) in work.items():
                if k in r["Name"]:
                    ns = float(r["TotalDurationNs"])
                    per_step_ms = ns / steps / 1e6
                    t_fl, t_by = fl / PEAK_FLOPS * 1e3, by / PEAK_BYTES * 1e3
                    bound = "flops" if t_fl >= t_by else "bytes"
                    rows.append({"kernel": k, "calls": int(r["Calls"]), "ms_per_head_step": per_step_ms,
                                 "gflop": fl / 1e9, "gbyte": by / 1e9, "bound": bound,
                                 "share_of_peak": max(t_fl, t_by) / per_step_ms if per_step_ms > 0 else None})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--only", choices=["hip", "both"], default="both")
    ap.add_argument("--stats", help="directory of a rocprofv3 --stats run of the same --shape / --iters: print shares of peak")
    a = ap.parse_args()
    names = a.shape or list(SHAPES)
    if a.stats:
        for n in names:
            for r in share_of_peak(a.stats, n, a.iters):
                print(json.dumps(dict(shape=n, **r)))
        return
    dev = th.device("cuda:0")
    for n in names:
        print(json.dumps(bench_head(n, a.iters, a.only, dev)), flush=True)
    if a.only == "both" and a.shape is None:
        print(json.dumps({"dmpnn_step_config2": bench_step(a.iters, dev)}), flush=True)


if __name__ == "__main__":
    main()
