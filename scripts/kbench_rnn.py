"""RNN rep-net layers on the GPU: the HIP recurrence kernels (csrc/dmp_rnn.hip) against the layer's own torch module
(nn.LSTM / nn.GRU / nn.RNN), forward and forward + backward per layer, and the whole 3-layer rep-net.

    python scripts/kbench_rnn.py                        # B 1024, L 512: LSTM uni / bi and GRU uni at H 128 and H 64
    python scripts/kbench_rnn.py --only hip --iters 3   # what a rocprofv3 run profiles

A ragged pre-padded gate, residual on, nonzero biases.  One JSON line per measurement.  Rated against the MI355X peaks
from the shapes alone: fp32 256 CU x 4 SIMD x 64 FLOP/clk x 2.4 GHz = 157 TFLOP/s, HBM 8 TB/s.  Forward FLOP per layer
2 B L D (G Hd) (Hin + Hd) (the input GEMM and the recurrence), bytes 4 B L (Hin + D G Hd (P, written and read) + 2 D Hd
(Y, H) + D NS Hd (the saved cell values)); backward FLOP twice the forward.  ``us_per_step``: the forward time over L."""
import argparse
import json
import os
import sys

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FLOPS = 256 * 4 * 64 * 2.4e9
PEAK_BYTES = 8e12


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    th.cuda.synchronize()
    a, b = th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        a.record()
        fn()
        b.record()
        th.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def bench_shape(args, cell, bi, H, dev):
    from dualmessagepassing_amd import rnn
    from dualmessagepassing_amd.seqmodel import RNNLayer
    B, L = args.B, args.L
    th.manual_seed(0)
    layers = [RNNLayer(cell, H, H, bidirectional=bi).to(dev) for _ in range(args.layers)]
    with th.no_grad():
        for layer in layers:
            for k, p in layer.named_parameters():
                if "bias" in k:
                    p.uniform_(-0.3, 0.3)
    lens = th.randint(L // 4, L + 1, (B,), device=dev)
    gate = (th.arange(L, device=dev).view(1, L) >= (L - lens).view(B, 1)).float()
    x0 = (th.randn(B, L, H, device=dev) * gate.unsqueeze(-1)).requires_grad_(True)
    D = 2 if bi else 1
    Hd = H // D
    G = rnn.CELLS[cell][1]
    flops = 2.0 * B * L * D * G * Hd * (H + Hd)
    nbytes = 4.0 * B * L * (H + 2 * D * G * Hd + 2 * D * Hd + D * rnn.SAVED[cell] * Hd)

    def module_layer(layer, x, g):
        return x + layer(x) * g.unsqueeze(-1)

    def hip_layer(layer, x, g):
        assert rnn.hip_layer_ok(layer, x, g)
        return rnn.rnn_layer_hip(layer, x, g, True)

    paths = {"hip": hip_layer, "module": module_layer}
    for name in ([args.only] if args.only else ["hip", "module"]):
        f = paths[name]
        layer = layers[0]
        xi = x0.detach().requires_grad_(True)
        dy = th.randn(B, L, H, device=dev)
        fwd = timed(lambda: f(layer, xi, gate), args.iters)
        both = timed(lambda: th.autograd.backward(f(layer, xi, gate), dy), args.iters)
        print(json.dumps({"path": name, "cell": cell, "bidirectional": bi, "B": B, "L": L, "H": H, "Hd": Hd,
                          "fwd_ms": round(fwd, 4), "fwd_bwd_ms": round(both, 4), "us_per_step": round(fwd * 1e3 / L, 3),
                          "fwd_frac_fp32_peak": round(flops / (fwd * 1e-3) / PEAK_FLOPS, 3),
                          "fwd_frac_hbm_peak": round(nbytes / (fwd * 1e-3) / PEAK_BYTES, 3),
                          "fwd_bwd_frac_fp32_peak": round(3 * flops / (both * 1e-3) / PEAK_FLOPS, 3)}), flush=True)

        def rep():
            x = x0
            for layer in layers:
                x = f(layer, x, gate)
            x.sum().backward()
        print(json.dumps({"path": name, "cell": cell, "bidirectional": bi, "H": H, "what": "rep_net_fwd_bwd",
                          "layers": len(layers), "ms": round(timed(rep, args.iters), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--H", type=int, nargs="+", default=[128, 64])
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--only", choices=["hip", "module"], default=None)
    args = ap.parse_args()
    dev = th.device("cuda:0")
    for H in args.H:
        for cell, bi in (("LSTM", False), ("LSTM", True), ("GRU", False)):
            bench_shape(args, cell, bi, H, dev)


if __name__ == "__main__":
    main()
