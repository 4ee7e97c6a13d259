"""The memory kernels (csrc/dmp_mem.hip) and the memory heads on the GPU.

* kernel forward (memory and memory mask) and backward against an fp64 restatement (``mem.memory_tensor`` in double)
  over a sweep of lengths, widths, memory lengths, pooling modes, circular extension, both end rules and mask shapes
  (front padding, interior holes, masked last positions, all-masked and single-live pairs), one and two tensors;
* max pooling where rows tie (rows of -1 / 0 / 1): kernels and the device's tensor-op route against the explicit-loop
  restatement of tests/test_mem_ties_cpu.py -- the value and the gradient go to the window's first maximum;
* bitwise reproducibility, every output written (DMP_POISON_DEAD_ROWS), the dispatch to the tensor-op path;
* the fixtures of scripts/make_golden_mem.py (the reference's own runs) with the tensor-op memory and attention paths
  monkeypatched to raise: init_memory, MemDotAttention, the four heads standalone, DMPNN + DIAMNet and RGIN +
  MaxMemAttnPredictNet (OutputDict, pred_v / pred_e, parameter gradients);
* a recorded training step (harness.GraphedTrainStep) of DMPNN + DIAMNet and of DMPNN + SumMemAttnPredictNet replays
  what the eager step computes.
Tolerances: the kernels against fp64 1e-5; fixtures as tests/test_mem_heads_cpu.py."""
import copy
import glob
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch as th

from conftest import GOLDEN, load_golden

pytestmark = pytest.mark.gpu
MEM = os.path.join(GOLDEN, "mem")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INLINE = os.environ.get("DMP_MEM_TESTS_INLINE") == "1"
inner = pytest.mark.skipif(not INLINE, reason="runs in a child process started by its test_* wrapper")
outer = pytest.mark.skipif(INLINE, reason="wrapper: the child process runs the inner case")


def _t(a):
    return th.from_numpy(np.asarray(a))


def _close(got, ref, tol, what):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu() if th.is_tensor(ref) else _t(ref).double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert not th.isnan(got).any(), what
    scale = max(1.0, float(ref.abs().max())) if ref.numel() else 1.0
    err = float((got - ref).abs().max()) if ref.numel() else 0.0
    assert err <= tol * scale, "%s: max err %g (scale %g)" % (what, err, scale)


# ----------------------------------------------------------------------------- kernels against fp64
def _masks(B, L, g):
    """Random holes after a random front padding and before a masked tail; pair 0 all masked, pair 1 one live position,
    pair 2 fully live (B >= 4)."""
    m = th.rand(B, L, generator=g) > 0.3
    s = th.randint(0, max(1, L // 3), (B,), generator=g)
    e = th.randint(0, L, (B,), generator=g)
    idx = th.arange(L).view(1, L)
    m &= (idx >= s.view(B, 1)) & (idx <= th.maximum(s, e).view(B, 1))
    m[:, 0] |= th.rand(B, generator=g) > 0.7
    m[0] = False
    m[1] = False
    m[1, L // 2] = True
    m[2] = True
    return m


def _case(B, L, D, seed, two):
    g = th.Generator().manual_seed(seed)
    xs = [th.randn(B, L, D, generator=g, dtype=th.float64).float().double() for _ in range(2 if two else 1)]
    return xs, _masks(B, L, g), th.Generator().manual_seed(seed + 1)


def _run(xs, mask, M, mem_init, inclusive, dys, dev):
    from dualmessagepassing_amd.mem import memory_init
    xg = [x.float().to(dev).requires_grad_(True) for x in xs]
    ys, mm = memory_init(xg, mask.to(dev), M, mem_init, inclusive_end=inclusive)
    th.autograd.backward(ys, [d.float().to(dev) for d in dys])
    th.cuda.synchronize()
    return ys, mm, [x.grad for x in xg]


def _ref(xs, mask, M, mem_init, inclusive, dys):
    from dualmessagepassing_amd.mem import memory_tensor, parse_mem_init
    mode, circular = parse_mem_init(mem_init)
    xd = [x.clone().requires_grad_(True) for x in xs]
    ys, mm = memory_tensor(xd, mask, M, mode, circular, inclusive)
    th.autograd.backward(ys, dys)
    return ys, mm, [x.grad for x in xd]


SWEEP = [(6, 1, 4, 1, False), (5, 7, 8, 4, True), (4, 40, 64, 4, True), (8, 64, 16, 3, False), (4, 300, 132, 4, True),
         (5, 513, 64, 7, False), (4, 33, 4, 2, True)]          # (B, L, D, M, two tensors)


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("mem_init", ["mean", "sum", "max", "circular_mean", "circular_sum", "circular_max"])
def test_kernel_matches_fp64(mem_init, inclusive, gpu):
    from dualmessagepassing_amd import mem
    for B, L, D, M, two in SWEEP:
        xs, mask, g = _case(B, L, D, zlib.crc32(repr((B, L, D, M, mem_init, inclusive)).encode()), two)
        assert mem.kernel_ok([x.float().to(gpu) for x in xs])
        dys = [th.randn(B, M, D, generator=g, dtype=th.float64).float().double() for _ in xs]
        ys, mm, dxs = _run(xs, mask, M, mem_init, inclusive, dys, gpu)
        rys, rmm, rdxs = _ref(xs, mask, M, mem_init, inclusive, dys)
        what = "%s L%d D%d M%d" % (mem_init, L, D, M)
        assert th.equal(mm.cpu(), rmm), what + " memory mask"
        for y, ry, dx, rdx in zip(ys, rys, dxs, rdxs):
            _close(y, ry, 1e-5, what + " memory")
            _close(dx, rdx, 1e-5, what + " dX")


TIE_SWEEP = [(4, 40, 8, 3, True), (4, 33, 4, 1, False), (5, 7, 8, 4, True), (4, 300, 12, 4, False)]   # (B, L, D, M, two tensors)


def _tied_windows(mem_init, inclusive, gpu, width=None):
    """Rows of -1 / 0 / 1 (tests/test_mem_ties_cpu.py): a window's value and gradient belong to its first maximum in
    extended-row order.  Memory and memory mask bitwise (a maximum of exact integers is exact), dX at the file's 1e-5.
    ``width``: that many columns instead of the case's."""
    from test_mem_ties_cpu import TIED_SHARE, tie_case, tie_grads, tie_reference
    long_cells = long_tied = 0
    for B, L, D, M, two in TIE_SWEEP:
        D = width or D
        xs, g = tie_case(B, L, D, two, zlib.crc32(repr((B, L, D, M, mem_init, inclusive)).encode()))
        mask = _masks(B, L, g)
        dys = tie_grads(xs, M, g)
        rys, rmm, rdxs, counts = tie_reference(xs, mask, M, mem_init, inclusive, dys)
        ys, mm, dxs = _run(xs, mask, M, mem_init, inclusive, dys, gpu)
        what = "%s L%d D%d M%d" % (mem_init, L, D, M)
        print("MEMTIES %s inclusive %d: tied %d of %d cells with two or more rows, %d of %d with 14 or more"
              % (what, inclusive, counts[1], counts[0], counts[3], counts[2]))
        long_cells, long_tied = long_cells + counts[2], long_tied + counts[3]
        assert th.equal(mm.cpu(), rmm), what + " memory mask"
        for y, ry, dx, rdx in zip(ys, rys, dxs, rdxs):
            assert th.equal(y.detach().cpu().double(), ry), what + " memory"
            _close(dx, rdx, 1e-5, what + " dX")
    # windows of 14 rows and more give each of the four waves several rows: ties inside a wave and between waves
    assert long_cells > 0 and long_tied >= TIED_SHARE * long_cells, (long_tied, long_cells)


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("mem_init", ["max", "circular_max"])
def test_kernel_gives_a_tied_window_to_its_first_maximum(mem_init, inclusive, gpu, monkeypatch):
    from dualmessagepassing_amd import mem
    calls = []
    orig = mem.MemInit.apply
    monkeypatch.setattr(mem.MemInit, "apply", lambda *a: (calls.append(1), orig(*a))[1])
    monkeypatch.setattr(mem, "memory_tensor", None)                    # (not callable: the tensor-op route would raise)
    _tied_windows(mem_init, inclusive, gpu)
    assert len(calls) == len(TIE_SWEEP), "the kernels were not taken"


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("mem_init", ["max", "circular_max"])
def test_tensor_op_route_on_the_device_gives_a_tied_window_to_its_first_maximum(mem_init, inclusive, gpu, monkeypatch):
    """Width 6 is no multiple of 4: ``mem.memory_tensor`` on the device."""
    from dualmessagepassing_amd import mem
    calls = []
    orig = mem.memory_tensor
    monkeypatch.setattr(mem, "memory_tensor", lambda *a: (calls.append(1), orig(*a))[1])
    _tied_windows(mem_init, inclusive, gpu, width=6)
    assert len(calls) == len(TIE_SWEEP), "the tensor-op route was not taken"


def test_kernel_is_bitwise_reproducible(gpu):
    for mem_init in ("mean", "circular_max", "sum"):
        xs, mask, g = _case(16, 300, 64, 3, True)
        dys = [th.randn(16, 4, 64, generator=g, dtype=th.float64) for _ in xs]
        a = _run(xs, mask, 4, mem_init, False, dys, gpu)
        b = _run(xs, mask, 4, mem_init, False, dys, gpu)
        for x, y in zip(a[0] + [a[1]] + a[2], b[0] + [b[1]] + b[2]):
            assert th.equal(x, y), mem_init


def test_every_output_is_written(gpu, monkeypatch):
    from dualmessagepassing_amd import fused
    from dualmessagepassing_amd.mem import MemInit
    monkeypatch.setattr(fused, "POISON_DEAD_ROWS", True)
    for mem_init, two in (("max", True), ("circular_mean", False), ("sum", True)):
        xs, mask, g = _case(6, 50, 12, 4, two)
        xg = [x.float().to(gpu).requires_grad_(True) for x in xs]
        outs = MemInit.apply(mask.to(gpu), 4, mem_init.split("_")[-1], mem_init.startswith("circular"), False, *xg)
        ys, ymask = outs[:-1], outs[-1]
        assert set(ymask.unique().tolist()) <= {0, 1}
        th.autograd.backward(list(ys), [th.randn_like(y) for y in ys])
        th.cuda.synchronize()
        for t in list(ys) + [x.grad for x in xg]:
            assert not th.isnan(t).any(), mem_init


def test_dispatch_kernel_or_tensor_path(gpu, monkeypatch):
    """fp32 rows of a width divisible by 4 take the kernels (views with a row stride included); other widths and non-fp32
    inputs take the tensor-op path."""
    from dualmessagepassing_amd import mem
    calls = []
    orig = mem.memory_tensor
    monkeypatch.setattr(mem, "memory_tensor", lambda *a: (calls.append(1), orig(*a))[1])
    mask = _masks(4, 20, th.Generator().manual_seed(0)).to(gpu)
    wide = th.randn(4, 20, 24, device=gpu)
    for x, want_kernel in ((wide, True), (wide[..., 4:20], True), (wide[..., :6], False), (wide.double(), False)):
        assert mem.kernel_ok([x]) == want_kernel
        n = len(calls)
        (y,), mm = mem.memory_init([x], mask, 3, "mean")
        assert (len(calls) == n) == want_kernel
        (ry,), rmm = orig([x.double().cpu()], mask.cpu(), 3, "mean", False, False)
        _close(y, ry, 1e-5, "memory")
        assert th.equal(mm.cpu(), rmm)


# ----------------------------------------------------------------------------- the reference's fixtures on the HIP path
@pytest.fixture
def kernels_only(monkeypatch):
    """Fail instead of taking the tensor-op memory or attention path."""
    from dualmessagepassing_amd import attn, mem

    def no(*a, **k):
        raise AssertionError("a tensor-op path ran where the HIP kernels should")
    monkeypatch.setattr(attn, "attention_tensor", no)
    monkeypatch.setattr(mem, "memory_tensor", no)


def _sd(d, prefix):
    return {k[len(prefix):]: _t(v) for k, v in d.items() if k.startswith(prefix)}


def _files(prefix):
    return sorted(glob.glob(os.path.join(MEM, prefix + "*.npz")))


def _id(p):
    return os.path.basename(p)[:-4]


@pytest.mark.parametrize("path", _files("initmem_"), ids=_id)
def test_init_memory_fixture_on_gpu(path, gpu, kernels_only):
    from dualmessagepassing_amd.mem import memory_init
    d = load_golden(path)
    M, mode, mask = int(d["M"]), str(d["mode"]), _t(d["mask"]).to(gpu)
    for cls, inclusive in (("memattn", False), ("diam", True)):
        x = _t(d["x"]).to(gpu).requires_grad_(True)
        (m,), mm = memory_init([x], mask, M, mode, inclusive_end=inclusive)
        (m * _t(d[cls + ".w"]).to(gpu)).sum().backward()
        _close(m, d[cls + ".mem"], 1e-6, cls + " memory")
        assert th.equal(mm.cpu(), _t(d[cls + ".mem_mask"])), cls + " memory mask"
        _close(x.grad, d[cls + ".dx"], 1e-6, cls + " dx")


@pytest.mark.parametrize("path", _files("memattn_"), ids=_id)
def test_mem_dot_attention_fixture_on_gpu(path, gpu, kernels_only):
    from dualmessagepassing_amd.pred import MemDotAttention
    d = load_golden(path)
    dq, dk, hid, nh = int(d["dq"]), int(d["dk"]), int(d["hid"]), int(d["nh"])
    attn = MemDotAttention(dq, dk, dk, hid, hid, num_heads=nh, scale=1.0, mem_len=int(d["M"]), mem_init=str(d["mode"]),
                           pre_lnorm=True)
    attn.load_state_dict(_sd(d, "p."), strict=True)
    attn.to(gpu)
    query, key, value = (_t(d[k]).to(gpu).requires_grad_(True) for k in ("query", "key", "value"))
    out = attn(query, key, value, query_mask=_t(d["qmask"]).to(gpu), key_mask=_t(d["kmask"]).to(gpu))
    (out * _t(d["w"]).to(gpu)).sum().backward()
    _close(out, d["out"], 1e-5, "out")
    for k, t in (("dquery", query), ("dkey", key), ("dvalue", value)):
        _close(t.grad, d[k], 1e-4, k)
    for k, p in attn.named_parameters():
        _close(p.grad, d["g." + k], 2e-4, "grad " + k)


@pytest.mark.parametrize("path", _files("head_"), ids=_id)
def test_head_fixture_on_gpu(path, gpu, kernels_only):
    from test_mem_heads_cpu import _load_head, run_head
    d = load_golden(path)
    run_head(_load_head(d, path).to(gpu), d, gpu)


def _graph(d, t, dev):
    from dualmessagepassing_amd.graph import BatchedGraph
    g = BatchedGraph(_t(d[t + "_src"]).to(dev), _t(d[t + "_dst"]).to(dev), int(d[t + "_num_nodes"]),
                     _t(d[t + "_bnn"]).to(dev), _t(d[t + "_bne"]).to(dev))
    for k, v in d.items():
        if k.startswith(t + "_ndata."):
            g.ndata[k.split(".", 1)[1]] = _t(v).to(dev)
        if k.startswith(t + "_edata."):
            g.edata[k.split(".", 1)[1]] = _t(v).to(dev)
    return g


@pytest.mark.parametrize("path", _files("model_"), ids=_id)
def test_model_fixture_on_gpu(path, gpu, kernels_only):
    from dualmessagepassing_amd.basemodel import build_model
    from test_mem_heads_cpu import model_state
    d = load_golden(path)
    config = {str(k): eval(str(v)) for k, v in zip(d["config_keys"], d["config_vals"])}
    model = build_model(**config)
    missing, unexpected = model.load_state_dict(model_state(d), strict=True)
    assert not missing and not unexpected
    model.to(gpu)
    out = model(_graph(d, "p", gpu), _graph(d, "g", gpu))
    for k in ("p_v_mask", "p_e_mask", "g_v_mask", "g_e_mask"):
        if "out." + k in d:
            assert th.equal(out[k].cpu(), _t(d["out." + k])), k
    for k in ("p_v_rep", "p_e_rep", "g_v_rep", "g_e_rep", "pred_c"):
        if "out." + k in d:
            _close(out[k], d["out." + k], 1e-4, k)
    total = out["pred_c"].sum()
    for k in ("pred_v", "pred_e"):
        if "out." + k in d:
            _close(out[k], d["out." + k], 1e-4, k)
            total = total + out[k].sum()
        else:
            assert out[k] is None
    total.backward()
    for k, p in model.named_parameters():
        if "grad." + k in d:
            _close(p.grad, d["grad." + k], 2e-4, "grad " + k)


# ----------------------------------------------------------------------------- recorded training step
def _isolated(node):
    env = dict(os.environ, DMP_MEM_TESTS_INLINE="1")
    r = subprocess.run([sys.executable, "-X", "faulthandler", "-m", "pytest", "%s::%s" % (os.path.abspath(__file__), node), "-q", "-x",
                        "-p", "no:cacheprovider"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    tail = "\n".join((r.stdout + r.stderr).splitlines()[-25:])
    assert r.returncode == 0 and " passed" in r.stdout, "child exited with %s:\n%s" % (r.returncode, tail)


@outer
@pytest.mark.parametrize("head", ["DIAMNet", "SumMemAttnPredictNet"])
def test_graphed_training_with_memory_head(head, gpu):
    _isolated("test_inner_graphed_training_with_memory_head[%s]" % head)


@inner
@pytest.mark.parametrize("head", ["DIAMNet", "SumMemAttnPredictNet"])
def test_inner_graphed_training_with_memory_head(head, gpu):
    """Two epochs of count-loss training of DMPNN + the head (4 heads, 3 inference steps for the memory-attention head),
    eager vs HIP-graph replay from the same initial state: same losses, same parameters."""
    from dualmessagepassing_amd.basemodel import build_model
    from dualmessagepassing_amd.dp import FlatAdamW, FlatGradSync
    from dualmessagepassing_amd.harness import GraphedTrainStep, SyntheticPairs, train_epoch
    ds = SyntheticPairs(56, 3, 2, 8, 16, 2, 1, seed=11)
    th.manual_seed(5)
    steps = 3 if head == "SumMemAttnPredictNet" else 1
    base = build_model(**ds.model_config(hid_dim=64, layers=2, pred_net=head, pred_num_heads=4, pred_infer_steps=steps)).to(gpu)
    runs = []
    for graphed in (False, True):
        model = copy.deepcopy(base)
        sync = FlatGradSync(model)
        master = sync.flatten_parameters()
        start = master.detach().clone()
        opt = FlatAdamW([master], lr=2e-3, weight_decay=1e-5, amsgrad=True, capturable=graphed)
        step = GraphedTrainStep(model, opt, sync) if graphed else None
        trace = []
        for epoch in range(2):
            train_epoch(model, opt, ds, 16, gpu, sync=sync, neg_slp=0.01, order=np.random.default_rng(epoch).permutation(len(ds)),
                        trace=trace, graph=step)
        th.cuda.synchronize()
        runs.append((th.stack([t[0] for t in trace]).cpu(), master.detach().clone(), step))
    (l0, p0, _), (l1, p1, step) = runs
    assert step.steps.replays >= 2 * 4 - 4, (step.steps.replays, step.steps.eager_calls)
    assert th.allclose(l0, l1, rtol=1e-5, atol=1e-6), (l0 - l1).abs().max()
    assert float((p0 - p1).abs().max()) <= 1e-5 * float(p0.abs().max()), float((p0 - p1).abs().max())
    assert float((p0 - start).abs().max()) > 1e-3
