#!/usr/bin/env python3
"""Dev aid: the kept-node product chain (csrc/dmp_nodechain.hip) -- forward, backward with dx, backward without dx -- and the
three-launch chain it replaces, timed with HIP events at bench.py's shape of a layer 1-2 pass (73,728 union node rows, a random
29,686 of them kept = 928 tiles) and at one tile.  Median of 30 launches after 5; writes profiles/nodechain_kbench.json."""
import json
import os
import sys

import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H = 128
SLOPE = 1.0 / 5.5
SHAPES = {"step": (73728, 29686), "one_tile": (73728, 32)}


def make_case(N, kept, dev, seed=7):
    """Operands as the layer hands them over (column blocks of wider buffers), a sorted random kept list as ``NodeRows.tiles``."""
    g = th.Generator(device=dev).manual_seed(seed)
    r = lambda *s: th.randn(*s, device=dev, generator=g)
    idx = th.randperm(N, device=dev, generator=g)[:kept].sort().values
    bound = (N + 31) // 32
    slot = th.full((bound * 32,), -1, dtype=th.int32, device=dev)
    slot[:kept] = idx.to(th.int32)
    tiles = (slot, th.zeros(bound, device=dev), th.tensor([(kept + 31) // 32], dtype=th.int32, device=dev), bound)
    c = dict(N=N, kept=idx, tiles=tiles, x=r(N, H), S=r(N, 2 * H), dxn=r(N, H), dXP=r(N, 3 * H), H1=r(N, H),
             Wx=r(H, 3 * H) / (3 * H) ** 0.5, Bn=r(2 * H, H) / (3 * H) ** 0.5, W2=r(H, H) / H ** 0.5, bn=r(H), b2=r(H))
    return c


def outputs(c, dev):
    N = c["N"]
    z = lambda w: th.zeros(N, w, device=dev)
    return dict(H1n=z(H), XP=z(3 * H), xn=z(H), dXP=c["dXP"].clone(), dS=z(2 * H), dx=z(H))


def chain_fwd(fused, c, o, panels):
    return fused.node_chain_fwd(c["x"], c["S"], panels[0], c["bn"], c["b2"], True, SLOPE, c["tiles"], o["H1n"], o["XP"][:, H:], o["xn"])


def chain_bwd(fused, c, o, panels, with_dx=True):
    """(inside ``fused.deferred_reductions()``: the launch alone, its partial rows reduced by the caller's block or dropped)"""
    return fused.node_chain_bwd(c["dxn"], c["H1"], o["dXP"][:, H:], panels[1], True, SLOPE, c["tiles"], o["dXP"][:, :H], o["dS"],
                                o["dx"] if with_dx else None)


def three_fwd(fused, c, o, T1):
    x, S, Wx, Bn, T = c["x"], c["S"], c["Wx"], c["Bn"], c["tiles"]
    fused.typed_jobs([dict(a=x, W=Wx[:, :H], bias=c["bn"], out=o["XP"][:, :H]), dict(a=S[:, :H], W=Bn[:H], out=T1),
                      dict(a=x, W=Wx[:, H:2 * H], out=o["XP"][:, H:2 * H]), dict(a=x, W=Wx[:, 2 * H:], out=o["XP"][:, 2 * H:])], T)
    fused.out_fwd_typed(S[:, H:], Bn[H:], None, o["XP"][:, :H], T, out=o["H1n"], slope=SLOPE, prev2=T1)
    fused.out_fwd_typed(o["H1n"], c["W2"], c["b2"], x, T, out=o["xn"], w_in_out=False)


def three_bwd(fused, c, o, oU):
    dxn, Wx, Bn, T, dXP = c["dxn"], c["Wx"], c["Bn"], c["tiles"], o["dXP"]
    fused.bwd_h1_typed(dxn, c["W2"], c["H1"], T, SLOPE, out=dXP[:, :H])
    fused.typed_jobs([dict(a=dXP[:, :H], W=Bn[:H], w_in_out=False, out=o["dS"][:, :H]), dict(a=dXP[:, :H], W=Bn[H:], w_in_out=False, out=o["dS"][:, H:]),
                      dict(a=dXP[:, :H], W=Wx[:, :H], w_in_out=False, prev=dxn, out=oU[:, :H]),
                      dict(a=dXP[:, H:2 * H], W=Wx[:, H:2 * H], w_in_out=False, out=oU[:, H:])], T)
    fused.out_fwd_typed(dXP[:, 2 * H:], Wx[:, 2 * H:], None, oU[:, :H], T, out=o["dx"], w_in_out=False, prev2=oU[:, H:])


def timeit(fn, reps=30):
    """Median µs of ``reps`` launches (HIP events around each), after 5 unmeasured ones."""
    for _ in range(5):
        fn()
    th.cuda.synchronize()
    ev = [(th.cuda.Event(enable_timing=True), th.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    th.cuda.synchronize()
    t = sorted(a.elapsed_time(b) * 1e3 for a, b in ev)
    return round(t[len(t) // 2], 1)


def bench_case(fused, c, dev, three=True):
    o = outputs(c, dev)
    panels = fused.node_chain_panels(c["Bn"], c["Wx"], c["W2"])
    res = {"chain_fwd_us": timeit(lambda: chain_fwd(fused, c, o, panels))}
    with fused.deferred_reductions() as dr:
        res["chain_bwd_dx_us"] = timeit(lambda: chain_bwd(fused, c, o, panels))
        res["chain_bwd_nodx_us"] = timeit(lambda: chain_bwd(fused, c, o, panels, with_dx=False))
        dr.jobs = []
    if three:
        T1, oU = th.zeros(c["N"], H, device=dev), th.zeros(c["N"], 2 * H, device=dev)
        res["three_launches_fwd_us"] = timeit(lambda: three_fwd(fused, c, o, T1))
        res["three_launches_bwd_dx_us"] = timeit(lambda: three_bwd(fused, c, o, oU))
    return res


def main():
    from dualmessagepassing_amd import _lib, fused
    dev = th.device("cuda:0")
    lib = _lib.load()
    res = {"device": th.cuda.get_device_name(0)}
    for name, (N, kept) in SHAPES.items():
        c = make_case(N, kept, dev)
        tiles = (kept + 31) // 32
        res[name] = dict(rows=N, kept=kept, tiles=tiles, workgroups=int(lib.dmp_node_chain_blocks(c["tiles"][3])), **bench_case(fused, c, dev))
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "nodechain_kbench.json")
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
