"""Memory heads on the GPU: the HIP memory initialisation (csrc/dmp_mem.hip) and sparsemax attention (csrc/dmp_attn.hip)
against the tensor-op paths (``mem.memory_tensor``, ``attn.attention_tensor``), in one process.

    python scripts/kbench_mem.py                          # every shape, both paths, and the DMPNN step
    python scripts/kbench_mem.py --only hip --shape edge2 --iters 3   # what a rocprofv3 run profiles
    python scripts/kbench_mem.py --stats DIR --shape edge2 --iters 3  # share of HBM peak from DIR/*kernel_stats.csv

Shapes (the inputs of scripts/kbench_attn.py: input width 128, pred_hid_dim 64, 4 heads, 3 inference steps, mem_len 4):
  node2  config 2's node head: B 1024, Lg 64, Lp 8
  edge2  config 2's edge head: B 1024, Lg 512, Lp 24, the reversed half of both sides masked
  node4  config 4's node head: B 1024, Lg 512, Lp 16
Per shape, DIAMNet and SumMemAttnPredictNet forward + backward three ways: all HIP ("hip_ms"), the memory on tensor ops
with the HIP attention ("tensor_mem_ms"), everything on tensor ops ("tensor_ms").  Then a DMPNN step (bench.py's config 2
model: forward, count loss, backward) with DIAMNet and with SumMemAttnPredictNet against one with SumPredictNet.
Where a tensor-op path runs out of memory the line says so.  The memory kernels are rated by bytes over 8 TB/s."""
import argparse
import glob
import json
import os
import sys

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from kbench_attn import D, HID, NH, SHAPES, STEPS, inputs, max_rel_diff, timed   # noqa: E402

PEAK_BYTES = 8e12
M = 4
HEADS = ("DIAMNet", "SumMemAttnPredictNet")


class tensor_path:
    """Route the memory (and with ``attention`` the attention) through the tensor ops inside the block."""

    def __init__(self, attention):
        self.attention = attention

    def __enter__(self):
        from dualmessagepassing_amd import attn, mem
        self.saved = [(mem, mem.kernel_ok)] + ([(attn, attn.kernel_ok)] if self.attention else [])
        for mod, _ in self.saved:
            mod.kernel_ok = lambda *a: False

    def __exit__(self, *exc):
        for mod, fn in self.saved:
            mod.kernel_ok = fn
        return False


def head_step(head, p, pm, x, gm):
    """Forward + backward of a head; DIAMNet without return weights leaves p_fc, g_fc and m_attn without gradients."""
    p, x = p.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y, _ = head(p, pm, x, gm)
    y.sum().backward()
    return [y.detach(), p.grad, x.grad] + [q.grad.clone() for q in head.parameters() if q.grad is not None]


def make_head(name, dev):
    from dualmessagepassing_amd import pred
    th.manual_seed(0)
    head = getattr(pred, name)(D, HID, num_heads=NH, infer_steps=STEPS, mem_len=M).to(dev)
    with th.no_grad():
        head.pred_fc2.weight.uniform_(-0.3, 0.3)
    return head


def bench_head(shape_name, head_name, iters, only, dev):
    shape = SHAPES[shape_name]
    head = make_head(head_name, dev)
    p, pm, x, gm = inputs(shape, dev)
    res = {"shape": shape_name, "head": head_name, **shape, "hid": HID, "heads": NH, "infer_steps": STEPS, "mem_len": M}

    def run():
        head.zero_grad(set_to_none=True)
        return head_step(head, p, pm, x, gm)
    hip = run()
    res["hip_ms"] = timed(run, iters)
    if only != "hip":
        for key, attention in (("tensor_mem_ms", False), ("tensor_ms", True)):
            try:
                with tensor_path(attention):
                    ten = run()
                    res[key] = timed(run, iters)
                res["max_rel_diff_count_" + key[:-3]] = max_rel_diff(hip[:1], ten[:1])
                del ten
            except th.cuda.OutOfMemoryError as e:
                res[key] = None
                res[key[:-3] + "_note"] = "tensor-op path does not fit in HBM: %s" % str(e).splitlines()[0][:160]
            th.cuda.empty_cache()
        if res.get("tensor_ms"):
            res["speedup"] = res["tensor_ms"] / res["hip_ms"]
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
    for head in ("SumPredictNet",) + HEADS:
        mc = bench.model_config(cfg)
        mc.update(pred_net=head, pred_hid_dim=HID, pred_num_heads=NH, pred_infer_steps=STEPS, pred_mem_len=M)
        th.manual_seed(3)
        model = build_model(**mc).to(dev)

        def step():
            model.zero_grad(set_to_none=True)
            o = model(graphs["p"], graphs["g"])
            count_loss(o["pred_c"].view(-1), shard["counts"]).backward()
        out[head + "_ms"] = timed(step, iters, warmup=2)
        del model
        th.cuda.empty_cache()
    for head in HEADS:
        out[head + "_over_pool"] = out[head + "_ms"] / out["SumPredictNet_ms"]
    return out


def call_bytes(mask, D, T, inclusive, mode):
    """(forward bytes, backward bytes) of one memory launch pair over ``mask`` [B, L]: every window row read once per
    slot, the outputs written; backward: dX written, dY (and the max index) read."""
    from dualmessagepassing_amd.mem import windows
    B, L = mask.shape
    _, _, cnt = windows(mask, M, False, inclusive)
    rows = float(cnt.sum())
    out = B * M * D * 4 * T * (2 if mode == "max" else 1)
    blocks = -(-T * M * (D // 4) // 64)
    fwd = rows * D * 4 * T + B * L * blocks + out + B * M + B * 8
    bwd = B * L * D * 4 * T + out + B * 8
    return fwd, bwd


def mem_work(shape_name, dev):
    """kernel -> bytes of one head forward + backward, per head: DIAMNet pools the target rows once (inclusive end, T 1,
    width D); SumMemAttnPredictNet pools pattern and target rows per inference step (T 2: keys and values, width HID)."""
    shape = SHAPES[shape_name]
    _, pm, _, gm = inputs(shape, dev)
    f, b = call_bytes(gm, D, 1, True, "mean")
    out = {"DIAMNet": {"mem_init_fwd_kernel": f, "mem_init_bwd_kernel": b}}
    fp, bp = call_bytes(pm, HID, 2, False, "sum")
    fg, bg = call_bytes(gm, HID, 2, False, "sum")
    out["SumMemAttnPredictNet"] = {"mem_init_fwd_kernel": STEPS * (fp + fg), "mem_init_bwd_kernel": STEPS * (bp + bg)}
    return out


def share_of_peak(stats_dir, shape_name, head_name, iters, dev):
    """Read rocprofv3's kernel stats of a ``--only hip --shape S --head H --iters N`` run (1 check + 1 warm-up + N timed
    head steps) and rate the memory kernels by bytes over the 8 TB/s HBM peak."""
    path = sorted(glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True))
    if not path:
        raise SystemExit("no *kernel_stats.csv under %s" % stats_dir)
    import csv
    steps = iters + 2
    work = mem_work(shape_name, dev)[head_name]
    rows = []
    with open(path[-1]) as f:
        for r in csv.DictReader(f):
            for k, by in work.items():
                if k in r["Name"]:
                    per_step_ms = float(r["TotalDurationNs"]) / steps / 1e6
                    rows.append({"kernel": k, "calls": int(r["Calls"]), "ms_per_head_step": per_step_ms, "gbyte": by / 1e9,
                                 "share_of_hbm_peak": by / PEAK_BYTES * 1e3 / per_step_ms if per_step_ms > 0 else None})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--shape", choices=sorted(SHAPES), action="append")
    ap.add_argument("--head", choices=HEADS, action="append")
    ap.add_argument("--only", choices=["hip", "both"], default="both")
    ap.add_argument("--no-step", action="store_true", help="skip the DMPNN step")
    ap.add_argument("--stats", help="directory of a rocprofv3 --stats run of the same --shape / --head / --iters: print shares")
    a = ap.parse_args()
    names = a.shape or list(SHAPES)
    heads = a.head or list(HEADS)
    dev = th.device("cuda:0")
    if a.stats:
        for n in names:
            for h in heads:
                for r in share_of_peak(a.stats, n, h, a.iters, dev):
                    print(json.dumps(dict(shape=n, head=h, **r)))
        return
    for n in names:
        for h in heads:
            print(json.dumps(bench_head(n, h, a.iters, a.only, dev)), flush=True)
    if a.only == "both" and not a.no_step:
        print(json.dumps({"dmpnn_step_config2": bench_step(a.iters, dev)}), flush=True)


if __name__ == "__main__":
    main()
