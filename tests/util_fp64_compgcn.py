"""fp64 restatements for the CompGCN tests: the relation-typed weight former of ``unc_compgcn`` (``dmp_relcorr_weights_*``) written
out with explicit circulant matrices, and its gradient formulas written out as sums -- no FFT, no autograd, numpy only."""
import numpy as np


def circulant_fp64(t):
    """``C[i, k] = t[(i + k) mod I]``."""
    t = np.asarray(t, dtype=np.float64).reshape(-1)
    i = np.arange(t.shape[0])
    return t[(i[:, None] + i[None, :]) % t.shape[0]]


def corr_fp64(a, t):
    """``corr(a, t)[k] = sum_i a[i] t[(i + k) mod I]`` for the rows of ``a``."""
    return np.asarray(a, dtype=np.float64) @ circulant_fp64(t)


def _blocks(T, loop_rel, Win, Wloop):
    T = np.asarray(T, dtype=np.float64)
    rows = [T[b] for b in range(T.shape[0])] + [np.asarray(loop_rel, dtype=np.float64).reshape(-1)]
    mats = [np.asarray(Win, dtype=np.float64)] * T.shape[0] + [np.asarray(Wloop, dtype=np.float64)]
    return rows, mats


def relcorr_weights_fp64(T, loop_rel, Win, Wloop, P, scale):
    """``Wcat [I, (R + 1) P]``: block b is ``scale C(t_b) @ W_b``, zero in the columns H .. P - 1."""
    rows, mats = _blocks(T, loop_rel, Win, Wloop)
    n, H = rows[0].shape[0], mats[0].shape[1]
    out = np.zeros((n, len(rows), P), dtype=np.float64)
    for b, (t, W) in enumerate(zip(rows, mats)):
        out[:, b, :H] = scale * (circulant_fp64(t) @ W)
    return out.reshape(n, -1)


def relcorr_weights_bwd_fp64(dWcat, T, loop_rel, Win, Wloop, P, scale):
    """``(dT [R, I], dloop_rel [I], dWin [I, H], dWloop [I, H])`` from ``dWcat [I, (R + 1) P]``:
    ``dt_b[j] = scale sum_{i, o} d_b[i, o] W_b[(j - i) mod I, o]``, ``dW_b[k, o] = scale sum_i t_b[(i + k) mod I] d_b[i, o]``,
    ``dWin`` the sum of ``dW_b`` over b < R."""
    rows, mats = _blocks(T, loop_rel, Win, Wloop)
    n, H, R = rows[0].shape[0], mats[0].shape[1], len(rows) - 1
    d = np.asarray(dWcat, dtype=np.float64).reshape(n, R + 1, P)[:, :, :H]
    dts, dWs = [], []
    for b, (t, W) in enumerate(zip(rows, mats)):
        G = d[:, b] @ W.T                                           # G[i, s] = sum_o d_b[i, o] W_b[s, o]
        i = np.arange(n)
        dts.append(scale * G[i[:, None], (i[None, :] - i[:, None]) % n].sum(0))     # [i, j] -> G[i, (j - i) mod I], summed over i
        dWs.append(scale * (circulant_fp64(t).T @ d[:, b]))
    return np.stack(dts[:R]), dts[R], sum(dWs[:R]), dWs[R]
