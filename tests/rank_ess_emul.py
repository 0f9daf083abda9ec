"""Restatement of the rank-normalised bulk-ESS and tail-ESS as include/linna_hip.h defines them, shared by
tests/test_rank_ess_host.py and tests/test_gpu_rank_ess.py (not a test module).  Independent of the product code: scipy's
``rankdata(method="average")`` and ``ndtri``, lagged products as plain sums, a Geyer loop of its own, all in float64.

* ``series(v, n, nw)``: the pooled float32 values of ONE parameter ``v[2 n nw]`` (element i nw + w) -> the three series
  ``[3][n][C]``, C = 2 nw split chains (first halves, then second halves): float32(z) of the average ranks, I(x <= q_0.05),
  I(x <= q_0.95); the quantiles are type 7 with integer position arithmetic (Python integers).
* ``ess_of_series(y, kuse)``: y[n][C] -> (ESS, last pair, status, margin): the multi-chain estimator on the lags 0 .. kuse,
  every chain relative to its own first row.  ``margin``: the smallest |P_t| over the pairs up to and including the one that
  ends the sequence -- the discrete outputs (last pair, status) are compared only where it is well above rounding.
* ``rank_ess(x, kuse=None)`` -> (out[nd][8] as ``linna_chain_rank_ess`` reports it, margin[nd][3]); ``kuse`` None: n - 1, every
  lag (what a caller that adds lags while status is 1 ends with: the sequence's end does not depend on the lags behind it).
* ``sticky_tail(seed)``: N(0, 1) chains in which a value above 1.8 stays with probability 0.98.
"""
import math

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

from rank_rhat_emul import pooled

MARGIN = 1e-6


def series(v, n, nw):
    v = np.asarray(v, np.float32).reshape(-1)
    S = 2 * n * nw
    assert len(v) == S
    r = rankdata(v, method="average")
    z = ndtri((r - 0.375) / (S + 0.25)).astype(np.float32).astype(np.float64)
    s = np.sort(v).astype(np.float64)
    out = [z]
    for num in (1, 19):
        pos = num * (S - 1)
        j, rem = pos // 20, pos % 20
        q = s[j] + (rem / 20.0) * (s[min(j + 1, S - 1)] - s[j])
        out.append(np.where(v.astype(np.float64) <= q, 1.0, 0.0))
    return np.stack([np.concatenate([u.reshape(2 * n, nw)[:n], u.reshape(2 * n, nw)[n:]], axis=1) for u in out])


def ess_of_series(y, kuse):
    n, C = y.shape
    assert 1 <= kuse <= n - 1
    rel = y - y[0]
    m = rel.sum(axis=0) / n
    c = rel - m
    A = [float(np.sum(c[:n - k] * c[k:])) / (n * C) for k in range(kuse + 1)]
    xbar = y[0] + m
    gm = float(np.sum(xbar)) / C
    between = float(np.sum((xbar - gm) ** 2)) / (C - 1)
    W = n / (n - 1.0) * A[0]
    vp = (n - 1.0) / n * W + between
    if not (math.isfinite(W) and math.isfinite(vp) and vp > 0):
        return float("nan"), -1.0, 0.0, float("inf")
    npairs = (kuse + 1) // 2
    total, prev, tend, margin = 0.0, float("inf"), npairs, float("inf")
    for t in range(npairs):
        P = (1.0 - (W - A[2 * t]) / vp) + (1.0 - (W - A[2 * t + 1]) / vp)
        margin = min(margin, abs(P))
        if not P > 0:
            tend = t
            break
        prev = min(prev, P)
        total += prev
    tau = max(-1.0 + 2.0 * total, 1.0 / math.log10(C * n))
    status = 1.0 if tend == npairs and kuse < n - 1 else 0.0
    return C * n / tau, tend - 1.0, status, margin


def rank_ess(x, kuse=None):
    p = pooled(x)
    rows, nw, nd = p.shape
    n = rows // 2
    kuse = n - 1 if kuse is None else kuse
    out = np.full((nd, 8), np.nan)
    out[:, 4:7], out[:, 7] = -1.0, 0.0
    margin = np.full((nd, 3), np.inf)
    for d in range(nd):
        v = p[:, :, d].reshape(-1)
        if not np.all(np.isfinite(v)):
            continue
        for t, y in enumerate(series(v, n, nw)):
            e, last, status, margin[d, t] = ess_of_series(y, kuse)
            out[d, 0 if t == 0 else 1 + t], out[d, 4 + t] = e, last
            out[d, 7] = max(out[d, 7], status)
        out[d, 1] = float("nan") if math.isnan(out[d, 2]) or math.isnan(out[d, 3]) else min(out[d, 2], out[d, 3])
    return out, margin


def sticky_tail(seed, nt=1000, nw=64, level=1.8, stay=0.98):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((nt, nw))
    u = rs.random_sample((nt, nw))
    for t in range(1, nt):
        keep = (x[t - 1] > level) & (u[t] < stay)
        x[t, keep] = x[t - 1, keep]
    return x[:, :, None].astype(np.float32)
