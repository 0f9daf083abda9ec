"""numpy restatement of split-R-hat and the multi-chain effective sample size as include/linna_hip.h defines them, shared by
tests/test_rhat_host.py and tests/test_gpu_rhat.py (not a test module).  Plain loops over parameters, chains and lags,
straight from the definitions, in float64: no FFT, no running sums, no block moments.

* ``split_rhat(x)``: x[N, nw, nd]; n = N // 2; split chain 2j = rows [0, n) of walker j, 2j + 1 = rows [N - n, N); per
  parameter W = mean_c s2_c (ddof 1), B / n = var_c(xbar_c) (ddof 1), var+ = (n - 1) / n W + B / n, R-hat = sqrt(var+ / W);
  NaN where W = 0 or a row of the halves is not finite.  Returns [nd, 4] = R-hat, W, var+, grand mean of the split chains.
* ``multichain_ess(x)``: acov_j(k) = (1 / N) sum_t (x_t - xbar_j)(x_{t+k} - xbar_j), A_k = mean_j acov_j(k), W = N / (N - 1) A_0,
  var+ = (N - 1) / N W + var_j(xbar_j), rho_k = 1 - (W - A_k) / var+, the pairs P_t = rho_2t + rho_2t+1 while positive, made
  monotone, tau = max(-1 + 2 sum P_t, 1 / log10(nw N)), ESS = nw N / tau.  Returns (ESS[nd], last pair index[nd]).
* ``ar1``: the AR(1) chains of tests/test_gpu_autocorr.py in float64 (no GPU module is imported on the host).
"""
import math

import numpy as np


def ar1(nt, nw, rho, seed, mean=0.0, scale=1.0):
    rs = np.random.RandomState(seed)
    rho = np.asarray(rho, np.float64)
    x = np.zeros((nt, nw, len(rho)))
    e = rs.standard_normal((nt, nw, len(rho)))
    x[0] = e[0] / np.sqrt(1 - rho ** 2)
    for i in range(1, nt):
        x[i] = rho * x[i - 1] + e[i]
    return mean + scale * x


def split_rhat(x):
    x = np.asarray(x, np.float64)
    N, nw, nd = x.shape
    n = N // 2
    if n < 2:
        raise ValueError("two halves of at least 2 rows")
    out = np.empty((nd, 4))
    for d in range(nd):
        means, variances, finite = [], [], True
        for j in range(nw):
            for half in (x[:n, j, d], x[N - n:, j, d]):
                finite = finite and bool(np.all(np.isfinite(half)))
                with np.errstate(invalid="ignore", over="ignore"):
                    m = np.sum(half) / n
                    means.append(m)
                    variances.append(np.sum((half - m) ** 2) / (n - 1))
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            nc = 2 * nw
            W = sum(variances) / nc
            gm = sum(means) / nc
            Bn = sum((m - gm) ** 2 for m in means) / (nc - 1)
            vp = (n - 1.0) / n * W + Bn
            r = math.sqrt(vp / W) if finite and W > 0 and np.isfinite(vp) else float("nan")
        out[d] = r, W, vp, gm
    return out


def multichain_ess(x):
    x = np.asarray(x, np.float64)
    N, nw, nd = x.shape
    ess, last = np.full(nd, np.nan), np.full(nd, -1.0)
    for d in range(nd):
        y = x[:, :, d]
        if not np.all(np.isfinite(y)):
            continue
        xb = [np.sum(y[:, j]) / N for j in range(nw)]
        c = [y[:, j] - xb[j] for j in range(nw)]

        def A(k):
            return sum(np.sum(c[j][:N - k] * c[j][k:]) / N for j in range(nw)) / nw

        W = N / (N - 1.0) * A(0)
        gm = sum(xb) / nw
        between = sum((m - gm) ** 2 for m in xb) / (nw - 1) if nw > 1 else 0.0
        vp = (N - 1.0) / N * W + between
        if not (np.isfinite(W) and np.isfinite(vp) and vp > 0):
            continue
        total, prev, t = 0.0, float("inf"), 0
        while 2 * t + 1 <= N - 1:
            p = (1.0 - (W - A(2 * t)) / vp) + (1.0 - (W - A(2 * t + 1)) / vp)
            if not p > 0:
                break
            prev = min(p, prev)
            total += prev
            t += 1
        tau = max(-1.0 + 2.0 * total, 1.0 / math.log10(nw * N))
        ess[d], last[d] = nw * N / tau, t - 1
    return ess, last
