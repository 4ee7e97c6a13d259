"""The TXL relative-position attention on the GPU: the kernels of csrc/dmp_txl.hip against the reference's formulation in
torch ops (``txl.rel_attention_tensor`` with the pad-and-reshape shift), in one process on one device.

    python scripts/kbench_txl.py                 # (N 512, q 64, k 128, nh 1, dh 128) and (N 512, q 64, k 64, nh 4, dh 32)

Per shape: forward + backward of each path between device events (alternating the two paths, the median of --iters),
the kernels' own launch times from the project's launch timer (``_lib.timer``), the greatest difference between the two
paths' outputs, and the traffic time of the kernels: the bytes they must move (``txl.fwd_bytes`` / ``txl.bwd_bytes``) over
8 TB/s.  One JSON line per shape."""
import argparse
import json
import os
import sys

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES = 8e12
PEAK_FLOPS = 256 * 4 * 64 * 2.4e9
SHAPES = [(512, 64, 128, 1, 128), (512, 64, 64, 4, 32)]


def bench_shape(shape, iters, warmup, dev):
    from dualmessagepassing_amd import _lib, txl
    N, q, k, nh, dh = shape
    g = th.Generator().manual_seed(0)
    args = [th.randn(N, q, nh, dh, generator=g), th.randn(N, k, nh, dh, generator=g), th.randn(N, k, nh, dh, generator=g),
            th.randn(k, nh, dh, generator=g), 0.5 * th.randn(nh, dh, generator=g), 0.5 * th.randn(nh, dh, generator=g)]
    xs = [a.to(dev).requires_grad_(True) for a in args]
    do = th.randn(N, q, nh * dh, generator=g).to(dev)
    scale = dh ** -0.5
    assert txl.kernel_ok(*xs)
    paths = {"hip": lambda: txl.rel_attention(*xs, scale),
             "torch": lambda: txl.rel_attention_tensor(*xs, scale, shift=txl.rel_shift_pad)}

    def step(name):
        for x in xs:
            x.grad = None
        o = paths[name]()
        o.backward(do)
        return o

    outs = {name: step(name).detach() for name in paths}
    grads = {}
    for name in paths:
        step(name)
        grads[name] = [x.grad.clone() for x in xs]
    diff = max([float((outs["hip"] - outs["torch"]).abs().max())] +
               [float((a - b).abs().max() / max(1.0, float(b.abs().max()))) for a, b in zip(grads["hip"], grads["torch"])])
    for _ in range(warmup):
        for name in paths:
            step(name)
    th.cuda.synchronize()
    times = {name: [] for name in paths}
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    for _ in range(iters):
        for name in paths:
            a.record()
            step(name)
            b.record()
            th.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    med = {name: sorted(t)[len(t) // 2] for name, t in times.items()}
    _lib.timer.reset()
    _lib.timer.enabled, _lib.timer.only = True, "txl_attn"
    for _ in range(iters):
        step("hip")
    launches = _lib.timer.summary()
    _lib.timer.enabled, _lib.timer.only = False, None
    groups = _lib.load().dmp_txl_bwd_groups(N, nh)
    fb, bb = txl.fwd_bytes(N, q, k, nh, dh), txl.bwd_bytes(N, q, k, nh, dh, groups)
    flops_fwd = 2.0 * N * nh * q * k * dh * 3
    rec = {"N": N, "q": q, "k": k, "nh": nh, "dh": dh, "iters": iters, "hip_fwd_bwd_ms": round(med["hip"], 4),
           "torch_fwd_bwd_ms": round(med["torch"], 4), "torch_over_hip": round(med["torch"] / med["hip"], 3),
           "hip_spread_ms": [round(min(times["hip"]), 4), round(max(times["hip"]), 4)],
           "torch_spread_ms": [round(min(times["torch"]), 4), round(max(times["torch"]), 4)],
           "max_rel_diff": diff, "fwd_traffic_us": round(fb / PEAK_BYTES * 1e6, 2), "bwd_traffic_us": round(bb / PEAK_BYTES * 1e6, 2),
           "fwd_fp32_us": round(flops_fwd / PEAK_FLOPS * 1e6, 2), "bwd_fp32_us": round(3 * flops_fwd / PEAK_FLOPS * 1e6, 2)}
    for name, v in launches.items():
        rec[name.split(" ")[0] + "_us"] = round(v["avg_us"], 2)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not th.cuda.is_available():
        raise SystemExit("kbench_txl.py needs a GPU")
    dev = th.device("cuda:0")
    for shape in SHAPES:
        bench_shape(shape, args.iters, args.warmup, dev)


if __name__ == "__main__":
    main()
