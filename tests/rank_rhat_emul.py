"""Restatement of the rank-normalised, folded split-R-hat as include/linna_hip.h defines it, shared by
tests/test_rank_rhat_host.py and tests/test_gpu_rank_rhat.py (not a test module).  Plain loops over parameters and split
chains, straight from the definition, in float64, with scipy's ``rankdata(method="average")`` and ``ndtri``: no sort of its
own, no inverse normal of its own.

* ``pooled(x)``: x[N, nw, nd] -> the pooled rows [2 n, nw, nd] as float32, n = N // 2: rows [0, n) and [N - n, N) (the middle
  row of an odd N is dropped), -0 turned into +0.
* ``fold(v)``: the pooled values of ONE parameter -> (zeta, med): med the float64 mean of the two middle sorted values,
  zeta = float32(|float64(v) - med|).
* ``ranks2(v)``: 2 x average rank, int64 (exact).
* ``rhat_of_ranks(r2, n, nw)``: z = ndtri((r - 3/8) / (S + 1/4)); per split chain mean and variance (ddof 1) of z, taken
  relative to the chain's first z (a constant chain has exactly no variance); W, B / n, var+, R-hat; NaN where W = 0.
* ``rank_rhat(x)`` -> out[nd, 4] = max(bulk, tail), bulk, tail, med; (r2bulk, r2fold)[nd, 2 n, nw].  A parameter with a
  value that is not finite in its halves: NaN for the three R-hats.
* ``wide_chains(seed)``: the fixture of the stopping rule: 64 chains of 400 rows, N(0, 1) in float32, the first 3 scaled by 3.
"""
import math

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata


def pooled(x):
    x = np.asarray(x, np.float32)
    N = len(x)
    n = N // 2
    if n < 2:
        raise ValueError("two halves of at least 2 rows")
    return np.concatenate([x[:n], x[N - n:]]) + np.float32(0.0)


def fold(v):
    v = np.asarray(v, np.float32).reshape(-1)
    s = np.sort(v).astype(np.float64)
    S = len(s)
    med = 0.5 * (s[S // 2 - 1] + s[S // 2])
    with np.errstate(over="ignore", invalid="ignore"):
        return np.abs(v.astype(np.float64) - med).astype(np.float32), med


def ranks2(v):
    r = rankdata(np.asarray(v, np.float32).reshape(-1), method="average")
    r2 = np.rint(2.0 * r).astype(np.int64)
    assert np.array_equal(r2, 2.0 * r)
    return r2


def rhat_of_ranks(r2, n, nw):
    S = 2 * n * nw
    z = ndtri((0.5 * np.asarray(r2, np.float64) - 0.375) / (S + 0.25)).reshape(2 * n, nw)
    means, variances = [], []
    for j in range(nw):
        for half in (z[:n, j], z[n:, j]):
            rel = half - half[0]
            m = float(np.sum(rel)) / n
            means.append(half[0] + m)
            variances.append(float(np.sum((rel - m) ** 2)) / (n - 1))
    nc = 2 * nw
    W = sum(variances) / nc
    gm = sum(means) / nc
    Bn = sum((m - gm) ** 2 for m in means) / (nc - 1)
    vp = (n - 1.0) / n * W + Bn
    return math.sqrt(vp / W) if W > 0 and np.isfinite(vp) else float("nan")


def rank_rhat(x):
    p = pooled(x)
    rows, nw, nd = p.shape
    n = rows // 2
    out = np.full((nd, 4), np.nan)
    r2b = np.zeros((nd, rows, nw), np.int64)
    r2f = np.zeros((nd, rows, nw), np.int64)
    for d in range(nd):
        v = p[:, :, d].reshape(-1)
        zeta, med = fold(v)
        out[d, 3] = med
        if not np.all(np.isfinite(v)):
            continue
        r2b[d] = ranks2(v).reshape(rows, nw)
        r2f[d] = ranks2(zeta).reshape(rows, nw)
        bulk, tail = rhat_of_ranks(r2b[d], n, nw), rhat_of_ranks(r2f[d], n, nw)
        out[d, :3] = (float("nan") if math.isnan(bulk) or math.isnan(tail) else max(bulk, tail)), bulk, tail
    return out, (r2b, r2f)


def wide_chains(seed, nw=64, nt=400, nwide=3, scale=3.0):
    x = np.random.default_rng(seed).standard_normal((nt, nw, 1)).astype(np.float32)
    y = x.copy()
    y[:, :nwide] *= np.float32(scale)
    return x, y
