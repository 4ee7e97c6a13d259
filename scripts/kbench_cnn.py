"""CNN rep-net layers on the GPU: the HIP kernels (csrc/dmp_cnn.hip) against the tensor ops (F.conv1d, max-pool in the
reference's [B, H, L] layout), forward + backward, per layer and for the whole 3-layer rep-net.

    python scripts/kbench_cnn.py                       # config 2's edge-sequence size, both paths
    python scripts/kbench_cnn.py --only hip --iters 3  # what a rocprofv3 run profiles

Shape: B 1024 pairs, L 512 tuples (add_rev), H 128, 3 layers, kernel 2 (padding 1: every layer makes the rows 2 longer),
relu, no BatchNorm, a ragged gate.  One JSON line per measurement.  Rated against the MI355X peaks from the shapes alone:
fp32 MFMA 256 CU x 4 SIMD x 64 FLOP/clk x 2.4 GHz = 157 TFLOP/s, HBM 8 TB/s; forward FLOP 2 B Lc H H k and bytes
4 (B L H + B L' H) + B L' H (the arg-max byte), backward FLOP twice the forward."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--H", type=int, default=128)
    ap.add_argument("--k", type=int, default=2)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only", choices=["hip", "tensor"], default=None)
    args = ap.parse_args()
    from dualmessagepassing_amd import cnn
    from dualmessagepassing_amd.seqmodel import CNNLayer
    dev = th.device("cuda:0")
    B, L, H, k = args.B, args.L, args.H, args.k
    th.manual_seed(0)
    layers = [CNNLayer(H, H, kernel_size=k, batch_norm=False).to(dev) for _ in range(args.layers)]
    lens = th.randint(L // 4, L + 1, (B,), device=dev)
    gate = (th.arange(L, device=dev).view(1, L) >= (L - lens).view(B, 1)).float()
    x0 = (th.randn(B, L, H, device=dev) * gate.unsqueeze(-1)).requires_grad_(True)

    def tensor_layer(layer, x, g):
        o = layer(x.transpose(1, 2))
        g = layer.gate_next(g.unsqueeze(1)).squeeze(1)
        o = (o * g.unsqueeze(1)).transpose(1, 2)
        return (x + o if o.size() == x.size() else o), g

    def hip_layer(layer, x, g):
        assert cnn.hip_layer_ok(layer, x, g)
        return cnn.cnn_layer_hip(layer, x, g, True)

    paths = {"hip": hip_layer, "tensor": tensor_layer}
    for name in ([args.only] if args.only else ["hip", "tensor"]):
        f = paths[name]
        x, g = x0, gate
        for i, layer in enumerate(layers):
            xi = x.detach().requires_grad_(True)
            Lc = xi.size(1) + 2 * layer.conv.padding[0] - k + 1
            flops = 2.0 * B * Lc * H * H * k
            y, gn = f(layer, xi, g)
            Lo = y.size(1)
            nbytes = 4.0 * B * H * (xi.size(1) + Lo) + B * Lo * H
            dy = th.randn_like(y)
            fwd = timed(lambda: f(layer, xi, g), args.iters)
            both = timed(lambda: th.autograd.backward(f(layer, xi, g)[0], dy), args.iters)
            print(json.dumps({"path": name, "layer": i, "B": B, "L_in": xi.size(1), "L_out": Lo, "H": H, "k": k,
                              "fwd_ms": round(fwd, 4), "fwd_bwd_ms": round(both, 4),
                              "fwd_frac_fp32_mfma_peak": round(flops / (fwd * 1e-3) / PEAK_FLOPS, 3),
                              "fwd_frac_hbm_peak": round(nbytes / (fwd * 1e-3) / PEAK_BYTES, 3),
                              "fwd_bwd_frac_fp32_mfma_peak": round(3 * flops / (both * 1e-3) / PEAK_FLOPS, 3)}), flush=True)
            x, g = y.detach(), gn

        def rep():
            x, g = x0, gate
            for layer in layers:
                x, g = f(layer, x, g)
            x.sum().backward()
        print(json.dumps({"path": name, "what": "rep_net_fwd_bwd", "layers": len(layers), "ms": round(timed(rep, args.iters), 4)}),
              flush=True)


if __name__ == "__main__":
    main()
