"""Max pooling of the memory initialisation where rows tie (representations after a ReLU carry exact zeros): the value and
the gradient of a window belong to its FIRST maximum in extended-row order (F.max_pool1d, pred.py:648-775).

``first_max_memory`` restates that rule with explicit loops, from the semantics in the docstring of
``dualmessagepassing_amd/mem.py`` and none of its code; ``tests/test_gpu_mem.py`` holds the kernels and the device's tensor-op
route to it as well.  Inputs are drawn from {-1, 0, 1} and upstream gradients from multiples of 1/4, so a maximum and every
sum of gradients are exact in float32 and in double, in any order: the comparisons here are equalities."""
import numpy as np
import pytest
import torch as th

TIED_SHARE = 0.8            # of the pooled cells with a window of two or more rows (a condition on the inputs, asserted)


def tie_case(B, L, D, two, seed):
    """(xs: one or two [B, L, D] double tensors of -1 / 0 / 1, generator for the upstream gradients)."""
    g = th.Generator().manual_seed(seed)
    return [th.randint(-1, 2, (B, L, D), generator=g).double() for _ in range(2 if two else 1)], g


def tie_grads(xs, M, g):
    return [th.randint(-8, 9, (x.size(0), M, x.size(2)), generator=g).double() / 4 for x in xs]


def first_max_memory(x, mask, M, circular, inclusive, dy):
    """x [B, L, D], mask [B, L] bool, dy [B, M, D] (numpy) -> (memory [B, M, D], memory mask [B, M], dx [B, L, D], counts).

    Per pair: s / e the first / last live position (0, 0 without one), n = e - s (+ 1 with ``inclusive``) segment rows from s,
    extended in circular mode to n' = n + ceil((n + 1) / 2) - 1 rows (row p = segment row p mod n).  n' <= M: extended row p is
    slot M - n' + p, the slots before are zero with mask 0.  n' > M: stride = n' // M, k = n' - (M - 1) stride, slot i holds
    extended rows i stride .. i stride + k - 1.  Per (pair, slot, column) the first maximum in that order; dy goes to its row.
    counts: [cells with a window of >= 2 rows, of those with the maximum on >= 2 distinct segment rows, the same two for windows
    of >= 14 rows]."""
    B, L, D = x.shape
    y, mm, dx = np.zeros((B, M, D)), np.zeros((B, M), dtype=bool), np.zeros((B, L, D))
    counts = [0, 0, 0, 0]
    for b in range(B):
        live = [l for l in range(L) if mask[b, l]]
        s, e = (live[0], live[-1]) if live else (0, 0)
        n = e - s + 1 if inclusive else e - s
        ext = n + (n + 2) // 2 - 1 if circular else n
        for i in range(M):
            if ext <= M:
                window = [i - (M - ext)] if i - (M - ext) >= 0 else []
            else:
                stride = ext // M
                window = list(range(i * stride, i * stride + ext - (M - 1) * stride))
            rows = [s + p % n for p in window]
            mm[b, i] = any(mask[b, r] for r in rows)
            for c in range(D):
                if not rows:
                    continue
                best = rows[0]
                for r in rows[1:]:
                    if x[b, r, c] > x[b, best, c]:
                        best = r
                y[b, i, c] = x[b, best, c]
                dx[b, best, c] += dy[b, i, c]
                tied = len({r for r in rows if x[b, r, c] == x[b, best, c]}) >= 2
                for at, least in ((0, 2), (2, 14)):
                    if len(rows) >= least:
                        counts[at] += 1
                        counts[at + 1] += tied
    return y, mm, dx, counts


def tie_reference(xs, mask, M, mem_init, inclusive, dys):
    """``first_max_memory`` per tensor: (memories, memory mask, dxs) as double tensors, the counts summed."""
    circular = mem_init.startswith("circular_")
    ys, dxs, total = [], [], [0, 0, 0, 0]
    for x, dy in zip(xs, dys):
        y, mm, dx, counts = first_max_memory(x.numpy(), mask.numpy(), M, circular, inclusive, dy.numpy())
        ys.append(th.from_numpy(y))
        dxs.append(th.from_numpy(dx))
        total = [a + b for a, b in zip(total, counts)]
    return ys, th.from_numpy(mm), dxs, total


@pytest.mark.parametrize("inclusive", [False, True])
@pytest.mark.parametrize("mem_init", ["max", "circular_max"])
def test_memory_tensor_gives_a_tied_window_to_its_first_maximum(mem_init, inclusive):
    from dualmessagepassing_amd.mem import memory_tensor, parse_mem_init
    from test_gpu_mem import _masks
    B, L, D, M = 4, 40, 8, 3
    xs, g = tie_case(B, L, D, True, 5)
    mask = _masks(B, L, g)
    dys = tie_grads(xs, M, g)
    rys, rmm, rdxs, (cells, tied, _, _) = tie_reference(xs, mask, M, mem_init, inclusive, dys)
    print("MEMTIES %s inclusive %d: %d of %d cells with a window of two or more rows tie" % (mem_init, inclusive, tied, cells))
    assert cells >= 2 * M * D and tied >= TIED_SHARE * cells, (tied, cells)      # (at least the fully live pair's, both tensors)
    mode, circular = parse_mem_init(mem_init)
    leaves = [x.clone().requires_grad_(True) for x in xs]
    ys, mm = memory_tensor(leaves, mask, M, mode, circular, inclusive)
    th.autograd.backward(ys, dys)
    assert th.equal(mm, rmm)
    for y, ry, x, rdx in zip(ys, rys, leaves, rdxs):
        assert th.equal(y.detach(), ry), "memory"
        assert th.equal(x.grad, rdx), "dX"


def test_the_restatement_agrees_with_max_pool1d_on_a_full_segment():
    """The rule's source: ``F.max_pool1d(kernel k, stride)`` over a fully live pair's rows, as ``init_mem`` calls it; its
    ``return_indices`` are the rows the restatement sends dy to."""
    L, D, M = 23, 4, 4
    (x,), g = tie_case(1, L, D, False, 9)
    mask = th.ones(1, L, dtype=th.bool)
    dy = tie_grads([x], M, g)[0]
    y, mm, dx, _ = first_max_memory(x.numpy(), mask.numpy(), M, False, True, dy.numpy())
    stride = L // M
    k = L - (M - 1) * stride
    py, idx = th.nn.functional.max_pool1d(x.transpose(1, 2), kernel_size=k, stride=stride, return_indices=True)
    assert th.equal(py.transpose(1, 2), th.from_numpy(y)) and bool(mm.all())
    want = th.zeros(1, D, L, dtype=th.float64).scatter_add(2, idx, dy.transpose(1, 2)).transpose(1, 2)
    assert th.equal(want, th.from_numpy(dx))
