"""Exact integer chains and integer references for the chain-statistics kernels of csrc/autocorr.hip
(tests/test_chain_exact_host.py pins them on the CPU, tests/test_gpu_chain_stats.py runs the entries of include/linna_hip.h
against them through the C ABI).  Not a test module.

The technique of tests/entries_ref.py and tests/net_exact.py carried to chains.  Every chain value is a small integer stored
as float32 and so is row 0 of every series, hence x - x[0] (what every kernel of that file works on) is an integer in
float64.  With A = max |x - x[0]| and N the longest window, ``exact_ok`` requires N A^2 < 2^53: every product, every partial
sum of Ssum[k], Tsum, the head / tail sums and the block moments M is then an integer below 2^53 -- exact in float64, whatever
the order of summation and whether or not a multiply-add is fused -- and equals the int64 reference BIT FOR BIT.

A chain here is ``x[row][parameter][lane]`` int64: the layout of CT restricted to the lanes that hold series.  Every chain is
a pure function of its key.  The references are written from the definitions in include/linna_hip.h, not from the kernels:

 * ``sums_ref``, ``append_ref``, ``moments_ref``: integer, compared with ``np.array_equal``;
 * ``tau_ref``, ``ess_ref``, ``rhat_ref``, ``meanstd_ref``: they start from EXACT INTEGER numerators, e.g.
       N^2 acf_k = N^2 S_k - N T (2 T - tail_k - head_k) + (N - k) T^2,
   take ratios once (tau: in float64 per series, walker means with math.fsum, the cumulative sum in extended precision; the
   others: rational arithmetic down to one final rounding) and return with every output an ERROR BOUND FOR THE KERNEL'S
   FORMULA: u = 2^-53 times the sum of the absolute values of the terms the kernel adds, times the number of roundings on
   the way, derived in each docstring by reading the kernel (first order in u, so each bound carries the factor ``SLACK``
   for the second-order terms and the reference's own last roundings).  No GPU output enters a bound.
 * every discrete output comes with a MARGIN: the distance of the deciding quantity from its threshold less its bound, which
   the CPU test requires to be positive for every case the GPU test runs.
"""
import math
from fractions import Fraction

import numpy as np

from entries_ref import F, rng

U = 2.0 ** -53           # unit roundoff of float64
SLACK = 1.25             # second-order terms of the first-order bounds + the reference's own last roundings
BAR = 1e-9               # the bar tests/test_gpu_autocorr.py and tests/test_gpu_rhat.py hold the same outputs to
RB = 128                 # LINNA_RHAT_BLOCK
OFFSET = 30000           # the large common offset of every series (exact in float32)


# ----------------------------------------------------------------------------------------------- chains
def ar1_int(key, nt, nl, rho, amp=8):
    """Rounded AR(1): OFFSET + round(amp * z), z_t = rho z_t-1 + e_t started in its stationary law -> int64 [nt][nl]."""
    e = rng("ar1_int", key).standard_normal((nt, nl))
    z = np.empty((nt, nl))
    z[0] = e[0] / math.sqrt(1.0 - rho * rho)
    for t in range(1, nt):
        z[t] = rho * z[t - 1] + e[t]
    return OFFSET + np.rint(amp * z).astype(np.int64)


def const_int(nt, nl):
    """The walker that never moved, every walker at the same point: tau, ESS and R-hat are NaN for this parameter."""
    return np.full((nt, nl), OFFSET + 3, np.int64)


def alt_int(nt, nl):
    """x_t = OFFSET + a_j (-1)^t, a_j in 1..5: over an even window every chain has the same mean (no between-chain term) and
    acov(1) = -(N - 1) / N acov(0), so Geyer's first pair P_0 = 1 / N - 2 / (N - 1) is negative."""
    a = 1 + np.arange(nl) % 5
    s = np.where(np.arange(nt) % 2 == 0, 1, -1)
    return OFFSET + (s[:, None] * a[None, :]).astype(np.int64)


def chain(key, nt, nl, params):
    """x[nt][len(params)][nl] int64; params: ("ar", rho) | ("const",) | ("alt",).  rho close to 1 with few lags asked for is
    the status-1 chain (more lags needed), ("alt",) the chain whose first Geyer pair is not positive."""
    cols = []
    for i, p in enumerate(params):
        if p[0] == "ar":
            cols.append(ar1_int((key, i, p[1]), nt, nl, p[1]))
        elif p[0] == "const":
            cols.append(const_int(nt, nl))
        elif p[0] == "alt":
            cols.append(alt_int(nt, nl))
        else:
            raise ValueError(p)
    return np.ascontiguousarray(np.stack(cols, axis=1))


def ct_image(x, nwp, fill, rows=None):
    """The float32 image CT[rows][nd][nwp] of a chain: lanes past the chain's and rows past its end hold ``fill``."""
    nt, nd, nl = x.shape
    ct = np.full((nt if rows is None else rows, nd, nwp), fill, F)
    ct[:nt, :, :nl] = x
    assert np.array_equal(ct[:nt, :, :nl].astype(np.int64), x), "a chain value is not exact in float32"
    return ct


def with_nan_row(ct, row, d):
    """A copy of a CT image with one NaN row (all lanes) in parameter d: R-hat is NaN for that parameter only."""
    ct = ct.copy()
    ct[row, d, :] = np.nan
    return ct


def rel0(x):
    return x - x[:1]


def amplitude(x):
    return int(np.abs(rel0(x)).max())


def exact_ok(x, nmax):
    """The exactness condition: nmax A^2 < 2^53 (sums of at most nmax products of integers of magnitude <= A)."""
    a = amplitude(x)
    return nmax * a * a < 2 ** 53


def numerators_ok(x, nmax, nl):
    """The integer numerators of the derived references fit int64: |S_k| <= N A^2, |T|, |head|, |tail| <= N A, so
    |N^2 S_k| + |N T (2 T - tail - head)| + (N - k) T^2 <= 6 N^3 A^2 per series, summed over nl series: 6 nl N^3 A^2 < 2^62.
    (The sums over chains of the R-hat and mean / std references are smaller and taken in Python integers.)"""
    a = amplitude(x)
    return 6 * nl * nmax ** 3 * a * a < 2 ** 62


# ----------------------------------------------------------------------------------------------- integer references
def sums_ref(x, lo, hi, K):
    """Ssum[k][d][l] = sum_{t = lo+k}^{hi-1} y_t y_{t-k} (k < K), Tsum[d][l] = sum_{t = lo}^{hi-1} y_t, y = x - x[0]; int64, from
    scratch."""
    y = rel0(x)[lo:hi]
    n = hi - lo
    S = np.zeros((K,) + x.shape[1:], np.int64)
    for k in range(min(K, n)):
        S[k] = (y[k:] * y[:n - k]).sum(axis=0)
    return S, y.sum(axis=0)


def lane_order(nw, wstride):
    """Source walker of every lane: every wstride-th walker first, the others behind them in order."""
    return [w for w in range(nw) if w % wstride == 0] + [w for w in range(nw) if w % wstride != 0]


def append_ref(block, nw, ndim, wstride, nwp):
    """block[nsteps][nw][ldb] -> rows[nsteps][ndim][nwp]: lane l holds walker lane_order[l], lanes >= nw hold zero."""
    block = np.asarray(block, F)
    out = np.zeros((block.shape[0], ndim, nwp), F)
    out[:, :, :nw] = block[:, lane_order(nw, wstride), :ndim].transpose(0, 2, 1)
    return out


def moments_ref(x, b0, b1):
    """M[b - b0][0 | 1][d][l] = sum of y | y^2 over rows [b RB, (b + 1) RB), y = x - x[0]; int64."""
    y = rel0(x)
    M = np.empty((b1 - b0, 2) + x.shape[1:], np.int64)
    for b in range(b0, b1):
        blk = y[b * RB:(b + 1) * RB]
        assert len(blk) == RB
        M[b - b0, 0] = blk.sum(axis=0)
        M[b - b0, 1] = (blk * blk).sum(axis=0)
    return M


# ----------------------------------------------------------------------------------------------- tau
def _acf_numerators(x, lo, hi, kuse):
    """Per series and lag k <= kuse: the integer N^2 acf_k and, in float64, what the kernel's formula
    acf_k = S_k - m (2 T - tail_k - head_k) + (N - k) m^2, m = T / N, adds up in absolute value."""
    n = hi - lo
    y = rel0(x)[lo:hi]
    S, T = sums_ref(x, lo, hi, kuse + 1)
    zero = np.zeros((1,) + y.shape[1:], np.int64)
    head = np.concatenate([zero, np.cumsum(y[:kuse], axis=0)])            # head_k = the first k rows of the window
    tail = np.concatenate([zero, np.cumsum(y[::-1][:kuse], axis=0)])      # tail_k = the last k rows
    left = (n - np.arange(kuse + 1))[:, None, None]
    mid = 2 * T[None] - tail - head
    num = n * n * S - n * T[None] * mid + left * T[None] * T[None]
    m = T / float(n)
    terms = np.abs(S) + np.abs(m[None] * mid) + left * (m * m)[None]
    return num, terms, S, T


def tau_ref(x, lo, hi, kuse, nlive, c=5.0, pre=None):
    """emcee's estimate as include/linna_hip.h states it for linna_acorr_tau, on the first nlive lanes of x.

    Returns a dict of [nd] arrays: tau, window, status, bound (on tau), margin (of the window and the status).

    Reference: rho_k = (N^2 acf_k) / (N^2 acf_0) from the integer numerators, one division per series and lag; f_k =
    math.fsum over the walkers / nlive; tau_k = 2 cumsum(f)_k - 1 in extended precision; the window is the first M with
    not (M < c tau_M); none within kuse: kuse with status 1 when kuse < N - 1, else numpy's argmin of an all-true mask, 0
    (unreachable for N >= 2: the autocovariances of all N lags sum to acf_0 / 2, so tau_{N-1} = 0).  A NaN f (a constant
    series: 0 / 0) fails the comparison at lag 0: tau = NaN, window 0, status 0.

    Bound, reading acorr_rho_kernel, acorr_fmean_kernel and acorr_window_kernel (S, T, head, tail are exact integers):
     * acf_k: m = T / N (1 rounding), m * mid (1), (N - k) * m * m (2), two additions (2): at most 6 roundings, each at
       most u times the sum of the absolute terms:               d_acf_k <= 6 u (|S_k| + |m mid_k| + (N - k) m^2);
       acf_0 of the normalisation, S_0 - N m m, likewise:        d_acf0  <= 6 u (|S_0| + N m^2);
     * rho = acf / acf0:                                         d_rho <= (d_acf_k + |rho| d_acf0) / |acf0| + u |rho|;
     * the 64-lane butterfly adds in 6 levels, acorr_fmean adds nwc / 64 <= 16 partials and divides once:
                                                                 d_f_k <= (sum_w d_rho + 23 u sum_w |rho|) / nlive;
     * acorr_window adds f_0..f_k in segments: at most k additions of lags plus 256 of segment partials, then 2 x - 1:
                                                                 d_tau_k <= 2 (sum_{j<=k} d_f_j + (k + 256) u sum_{j<=k} |f_j|) + u |tau_k|.
    Margin: min over the lags k up to the decision of |k - c tau_k| - c d_tau_k."""
    n = hi - lo
    assert 0 <= kuse <= n - 1 and 1 <= nlive <= x.shape[2]
    num, terms, _, _ = pre or _acf_numerators(x[:, :, :nlive], lo, hi, kuse)
    nd = x.shape[1]
    out = {k: np.full(nd, np.nan) for k in ("tau", "bound", "margin")}
    out["window"], out["status"] = np.zeros(nd), np.zeros(nd)
    ks = np.arange(kuse + 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        acf0 = num[0] / float(n * n)
        rho = num / num[0].astype(np.float64)
        d_acf = 6 * U * terms
        d_rho = (d_acf + np.abs(rho) * d_acf[0]) / np.abs(acf0) + U * np.abs(rho)
    for d in range(nd):
        if not np.all(num[0, d] != 0):
            out["margin"][d] = np.inf                       # 0 / 0 exactly, on the device as here: nothing to decide
            continue
        f = np.array([math.fsum(rho[k, d]) for k in ks]) / nlive
        absf = np.array([math.fsum(np.abs(rho[k, d])) for k in ks]) / nlive
        d_f = (d_rho[:, d].sum(axis=1) + 23 * U * np.abs(rho[:, d]).sum(axis=1)) / nlive
        taus = np.asarray(2 * np.cumsum(f.astype(np.longdouble)) - 1, np.float64)
        d_tau = SLACK * (2 * (np.cumsum(d_f) + (ks + 256) * U * np.cumsum(absf)) + U * np.abs(taus))
        false = np.nonzero(~(ks < c * taus))[0]
        if len(false):
            w, status = int(false[0]), 0
        elif kuse >= n - 1:
            w, status = 0, 0
        else:
            w, status = kuse, 1
        upto = kuse if not len(false) else w
        out["tau"][d], out["window"][d], out["status"][d], out["bound"][d] = taus[w], w, status, d_tau[w]
        out["margin"][d] = np.min(np.abs(ks - c * taus)[:upto + 1] - c * d_tau[:upto + 1])
    return out


# ----------------------------------------------------------------------------------------------- multi-chain ESS
def ess_ref(x, lo, hi, kuse, nlive, pre=None):
    """Stan's multi-chain ESS as include/linna_hip.h states it for linna_acorr_ess, on the first nlive lanes of x.

    Returns a dict of [nd] arrays: ess, last (pair index, -1: none), status, bound (on ess), margin (of last and status).

    Reference, rational: A_k = sum_j N^2 acf_jk / (nlive N^3); the chain means xbar_j = (N (x0_j - x0_0) + T_j) / N; W, var+,
    rho_k, the pairs, the monotone sum and tau as Fractions; one rounding at the end (and the float64 floor 1 / log10(nlive N)).
    var+ = 0 (every chain constant at one point): ESS = NaN, last = -1, status 0.

    Bound, reading acorr_cov_kernel, acorr_fmean_kernel and acorr_geyer_kernel:
     * d_acf as in tau_ref; acov = acf / N (1);  d_A_k <= (sum_j (d_acf_jk / N + u |acov_jk|) + 23 u sum_j |acov_jk|) / nlive;
     * xbar = (ref - refd) + m: d_xb <= u |m| + u |xbar|; q1 = sum xbar, q2 = sum xbar^2 over 6 butterfly levels and up to 16
       partials: d_q1 <= sum d_xb + 22 u sum |xbar|, d_q2 <= sum (2 |xbar| d_xb + u xbar^2) + 22 u sum xbar^2;
       between = (q2 - q1 q1 / nl) / (nl - 1): d_between <= (d_q2 + (2 |q1| d_q1 + 2 u q1^2) / nl + u (q2 + q1^2 / nl)) / (nl - 1)
       + u between -- the cancellation of q2 against q1^2 / nl is in the absolute terms;
     * W = N / (N - 1) * A_0: d_W <= N / (N - 1) d_A0 + 2 u W;  var+ = (N - 1) / N * W + between: d_vp <= d_W + 2 u W + d_between + u var+;
     * r_k = (W - A_k) / var+: d_r <= (d_W + d_A_k + u |W - A_k|) / var+ + |r| d_vp / var+ + u |r|;
       P_t = (1 - r_2t) + (1 - r_2t+1): d_P <= d_r_2t + d_r_2t+1 + u (|1 - r_2t| + |1 - r_2t+1| + |P_t|);
     * tau = -1 + 2 sum of T + 1 monotone pairs: d_tau <= 2 (sum d_P + (T + 1) u sum |P|) + u |tau|; floored: 4 u floor (log10,
       one division); ESS = nl N / tau: d_ESS <= ESS (d_tau / tau + u).
    Margin: min over the pairs up to and with the first non-positive one of |P_t| - d_P_t."""
    n = hi - lo
    assert 0 <= kuse <= n - 1 and 1 <= nlive <= x.shape[2]
    xs = x[:, :, :nlive]
    num, terms, _, T = pre or _acf_numerators(xs, lo, hi, kuse)
    nd, nl = x.shape[1], nlive
    out = {k: np.full(nd, np.nan) for k in ("ess", "bound")}
    out["last"], out["status"], out["margin"] = np.full(nd, -1.0), np.zeros(nd), np.full(nd, np.inf)
    npairs = (kuse + 1) // 2
    for d in range(nd):
        A = [Fraction(int(num[k, d].sum()), nl * n ** 3) for k in range(kuse + 1)]
        X = [int(v) for v in n * (xs[0, d] - xs[0, d, 0]) + T[d]]
        between = Fraction(nl * sum(v * v for v in X) - sum(X) ** 2, nl * (nl - 1) * n * n) if nl > 1 else Fraction(0)
        W = Fraction(n, n - 1) * A[0]
        vp = A[0] + between
        if not vp > 0:
            continue
        # ---- the kernel's error, in float64 magnitudes
        acov = np.abs(num[:, d] / float(n) ** 3)
        d_A = ((6 * U * terms[:, d] / n + U * acov).sum(axis=1) + 23 * U * acov.sum(axis=1)) / nl
        m = T[d] / float(n)
        xb = np.array(X, np.float64) / n
        d_xb = U * np.abs(m) + U * np.abs(xb)
        q1, q2 = abs(xb.sum()), (xb * xb).sum()
        d_q1 = d_xb.sum() + 22 * U * np.abs(xb).sum()
        d_q2 = (2 * np.abs(xb) * d_xb + U * xb * xb).sum() + 22 * U * q2
        fb, fW, fvp = float(between), float(W), float(vp)
        d_b = ((d_q2 + (2 * q1 * d_q1 + 2 * U * q1 * q1) / nl + U * (q2 + q1 * q1 / nl)) / (nl - 1) + U * fb) if nl > 1 else 0.0
        d_W = n / (n - 1.0) * d_A[0] + 2 * U * fW
        d_vp = d_W + 2 * U * fW + d_b + U * fvp
        r = [(W - a) / vp for a in A]
        fr = np.array([float(v) for v in r])
        fA = np.array([float(a) for a in A])
        d_r = (d_W + d_A + U * np.abs(fW - fA)) / fvp + np.abs(fr) * d_vp / fvp + U * np.abs(fr)
        P = [(1 - r[2 * t]) + (1 - r[2 * t + 1]) for t in range(npairs)]
        fP = np.array([float(p) for p in P])
        d_P = SLACK * (d_r[0:2 * npairs:2] + d_r[1:2 * npairs:2] + U * (np.abs(1 - fr[0:2 * npairs:2]) + np.abs(1 - fr[1:2 * npairs:2]) + np.abs(fP)))
        tend = next((t for t in range(npairs) if not P[t] > 0), npairs)
        total, prev = Fraction(0), None
        for t in range(tend):
            prev = P[t] if prev is None or P[t] < prev else prev
            total += prev
        tau = -1 + 2 * total
        ftau = float(tau)
        d_tau = 2 * (d_P[:tend].sum() + tend * U * np.abs(fP[:tend]).sum()) + U * abs(ftau)
        floor_ = 1.0 / math.log10(nl * n)
        if ftau < floor_:
            ftau, d_tau = floor_, 4 * U * floor_
        ess = nl * n / ftau
        out["ess"][d], out["last"][d] = ess, tend - 1
        out["status"][d] = 1.0 if (tend == npairs and kuse < n - 1) else 0.0
        out["bound"][d] = SLACK * ess * (d_tau / ftau + U)
        if npairs:
            upto = min(tend, npairs - 1)
            out["margin"][d] = np.min(np.abs(fP[:upto + 1]) - d_P[:upto + 1])
    return out


# ----------------------------------------------------------------------------------------------- split-R-hat
def rhat_ref(xf, lo, hi, nwp):
    """Split-R-hat as include/linna_hip.h states it, over all lanes of ``xf[row][nd][nw]`` (float64 image of an integer chain
    that may hold NaN rows), for a CT of nwp lanes per parameter (the bound counts its nwp / 64 lane groups).

    Returns (out[nd][4] = R-hat, W, var+, grand mean; bound[nd][4]; margin[nd] of NaN versus finite).

    Reference, rational: per split chain c the integers s1 = sum y, s2 = sum y^2 (y = x - the walker's row 0), s2_c =
    (n s2 - s1^2) / (n (n - 1)), xbar_c = (n (x0_j - x0_0) + s1) / n relative to the parameter's reference x0_0; W, B / n,
    var+ and the grand mean as Fractions, one rounding each, R-hat = sqrt of the rounded ratio.  A non-finite value in a row of
    the two halves: all four NaN here (the header promises the NaN R-hat); W = 0: R-hat NaN, the rest exact zeros / the mean.

    Bound, reading chain_rhat_kernel (s1, s2 exact, with or without block records M):
     * mrel = s1 / n (1); var = (s2 - s1 * mrel) / (n - 1): d_var <= 4 u (s2 + s1^2 / n) / (n - 1);
       mean = (ref - refd) + mrel: d_mean <= u |mrel| + u |mean|;
     * am, am2, av: per lane 2 nwp / 64 additions, then 6 butterfly levels -- g = 2 nwp / 64 + 6 roundings:
       d_am <= sum d_mean + g u sum |mean|; d_am2 <= sum (2 |mean| d_mean + u mean^2) + g u sum mean^2; d_av <= sum d_var + g u sum var;
     * W = av / nc: d_W <= d_av / nc + u W;  Bn = (am2 - am am / nc) / (nc - 1):
       d_Bn <= (d_am2 + (2 |am| d_am + 2 u am^2) / nc + u (am2 + am^2 / nc)) / (nc - 1) + u Bn;
       var+ = (n - 1) / n * W + Bn: d_vp <= d_W + 2 u W + d_Bn + u var+;  mean = refd + am / nc: d <= d_am / nc + u |am / nc| + u |mean|;
     * R-hat = sqrt(var+ / W): d_R <= R (d_vp / var+ + d_W / W) / 2 + 2 u R.
    Margin: W - d_W where R-hat is finite (W = 0 happens only when every split chain is constant: s1 / n is then an integer v
    and s1 * v = s2 without rounding, so the device's W is an exact zero too)."""
    nt, nd, nw = xf.shape
    n = (hi - lo) // 2
    assert n >= 2
    out, bound, margin = np.full((nd, 4), np.nan), np.full((nd, 4), np.nan), np.full(nd, np.inf)
    g = 2 * (nwp // 64) + 6
    nc = 2 * nw
    for d in range(nd):
        halves = [xf[lo:lo + n, d], xf[hi - n:hi, d]]
        if not all(np.all(np.isfinite(h)) for h in halves):
            continue
        x0 = xf[0, d].astype(np.int64)
        s1 = np.concatenate([(h.astype(np.int64) - x0).sum(axis=0) for h in halves])
        s2 = np.concatenate([((h.astype(np.int64) - x0) ** 2).sum(axis=0) for h in halves])
        r = np.concatenate([x0 - x0[0], x0 - x0[0]])
        X = [int(v) for v in n * r + s1]
        V = [int(v) for v in n * s2 - s1 * s1]
        W = Fraction(sum(V), nc * n * (n - 1))
        Bn = Fraction(nc * sum(v * v for v in X) - sum(X) ** 2, nc * (nc - 1) * n * n)
        vp = Fraction(n - 1, n) * W + Bn
        gm = int(x0[0]) + Fraction(sum(X), nc * n)
        fW, fvp, fBn = float(W), float(vp), float(Bn)
        # ---- the kernel's error
        mrel = s1 / float(n)
        mean = np.array(X, np.float64) / n
        var = np.array(V, np.float64) / (n * (n - 1.0))
        d_var = 4 * U * (s2 + s1 * mrel) / (n - 1.0)
        d_mean = U * np.abs(mrel) + U * np.abs(mean)
        am, am2 = abs(mean.sum()), (mean * mean).sum()
        d_am = d_mean.sum() + g * U * np.abs(mean).sum()
        d_am2 = (2 * np.abs(mean) * d_mean + U * mean * mean).sum() + g * U * am2
        d_av = d_var.sum() + g * U * var.sum()
        d_W = d_av / nc + U * fW
        d_Bn = (d_am2 + (2 * am * d_am + 2 * U * am * am) / nc + U * (am2 + am * am / nc)) / (nc - 1) + U * fBn
        d_vp = d_W + 2 * U * fW + d_Bn + U * fvp
        d_gm = d_am / nc + U * am / nc + U * abs(float(gm))
        out[d, 1:], bound[d, 1:] = (fW, fvp, float(gm)), (SLACK * d_W, SLACK * d_vp, SLACK * d_gm)
        if W > 0:
            out[d, 0] = math.sqrt(fvp / fW)
            bound[d, 0] = SLACK * out[d, 0] * ((d_vp / fvp + d_W / fW) / 2 + 2 * U)
            margin[d] = fW - SLACK * d_W
        else:
            assert not np.any(s2), "W = 0 on a chain that moves"
    return out, bound, margin


# ----------------------------------------------------------------------------------------------- checkmeanstd's moments
def meanstd_ref(x, nws, t0, tm, t1):
    """out[d][h] = (mean, population standard deviation) of parameter d over rows [t0, tm) (h = 0) and [tm, t1) (h = 1) of the
    first nws lanes, as include/linna_hip.h states it; an empty half: NaN, NaN.  Returns (out[nd][2][2], bound[nd][2][2]).

    Reference, rational: with v = x - ref, ref = x[t0][d][0] (the kernel's reference point), a = sum v, b = sum v^2 integers,
    n = rows * nws: mean = ref + a / n, var = (n b - a^2) / n^2, one rounding each, then the square root.

    Bound, reading chain_meanstd_kernel (a and b are exact): mu = a / n (1), b / n (1), mu * mu (2 from mu, 1), the subtraction
    (1): d_var <= 4 u (b / n + mu^2) -- the cancellation of b / n against mu^2 is in the absolute terms, and the reference point
    at t0 keeps mu^2 at the drift of the window, not at OFFSET^2; std = sqrt(var): d_std <= min(d_var / std, sqrt(d_var)) +
    u std; mean = mu + ref: d_mean <= u |mu| + u |mean|."""
    nd = x.shape[1]
    out, bound = np.full((nd, 2, 2), np.nan), np.full((nd, 2, 2), np.nan)
    for d in range(nd):
        ref = int(x[t0, d, 0])
        for h, (r0, r1) in enumerate(((t0, tm), (tm, t1))):
            n = (r1 - r0) * nws
            if n == 0:
                continue
            v = x[r0:r1, d, :nws] - ref
            a, b = int(v.sum()), int((v * v).sum())
            mean, var = ref + Fraction(a, n), Fraction(n * b - a * a, n * n)
            std = math.sqrt(float(var))
            mu = a / float(n)
            d_var = 4 * U * (b / float(n) + mu * mu)
            d_std = (min(d_var / std, math.sqrt(d_var)) if std > 0 else math.sqrt(d_var)) + U * std
            out[d, h] = float(mean), std
            bound[d, h] = SLACK * (U * abs(mu) + U * abs(float(mean))), SLACK * d_std
    return out, bound


# ----------------------------------------------------------------------------------------------- the cases of the GPU test
# (here, so that tests/test_chain_exact_host.py can hold every one of them to the conditions on the inputs)
_CHAINS = {}


def cached_chain(key, nt, nl, params):
    k = (key, nt, nl, params)
    if k not in _CHAINS:
        _CHAINS[k] = chain(key, nt, nl, params)
        _CHAINS[k].setflags(write=False)
    return _CHAINS[k]


TAU_PARAMS = (("ar", 0.5), ("const",), ("ar", 0.9), ("ar", 0.99))
ALT_PARAMS = (("alt",), ("ar", 0.5))
TAU_KUSE = (0, 31, 32, 33, 255, 256, 600, 639)                  # 639 = N - 1: every lag of the window
# (name, chain params, rows, nwp, nwc, nlive, lo, hi, kuse)
TAU_CASES = tuple(("n640_k%d_l%d" % (k, nl), TAU_PARAMS, 650, 128, 64, nl, 3, 643, k) for k in TAU_KUSE for nl in (1, 63, 64)) + tuple(
    ("n640_w%d_c%d_k%d" % (nwp, nwc, k), TAU_PARAMS, 650, nwp, nwc, nwc - 1, 3, 643, k) for nwp, nwc in ((128, 128), (192, 128)) for k in (33, 600)) + tuple(
    ("alt_k%d_l%d" % (k, nl), ALT_PARAMS, 50, 128, 64, nl, 4, 44, k) for k in (1, 20, 39) for nl in (1, 63, 64)) + (
    ("n5_k4", TAU_PARAMS, 650, 128, 64, 64, 10, 15, 4),)
_TAU_REFS = {}


def tau_case_chain(case):
    return cached_chain("tau", case[2], case[4], case[1])


def tau_case_refs(case):
    """(tau_ref, ess_ref) of a case, computed once."""
    if case not in _TAU_REFS:
        _, _, _, _, _, nlive, lo, hi, kuse = case
        x = tau_case_chain(case)
        pre = _acf_numerators(x[:, :, :nlive], lo, hi, kuse)
        _TAU_REFS[case] = (tau_ref(x, lo, hi, kuse, nlive, pre=pre), ess_ref(x, lo, hi, kuse, nlive, pre=pre))
    return _TAU_REFS[case]


RHAT_PARAMS = (("ar", 0.5), ("const",), ("ar", 0.9), ("ar", 0.7))       # the last one takes the NaN row
RHAT_ROWS, RHAT_NWP = 4700, 128
RHAT_NW = (1, 64, 65)
# (name, lo, hi, nblocks or None = every complete block, NaN row of parameter 3 or None)
RHAT_WINDOWS = (
    ("n2", 13, 17, None, 14),                      # n = 2; the NaN row in the ragged rows
    ("odd_n3", 5, 12, None, 8),                 # N = 7: row 8 is the dropped middle row -> finite
    ("blocks_1_0", 100, 500, None, 101),        # halves [100, 300) and [300, 500): one whole block and none
    ("blocks_17_17", 3, 4624, None, 1000),      # N = 4621 odd, n = 2310: [3, 2313) holds blocks 1..17, [2314, 4624) blocks 19..35;
    ("blocks_17_17_mid", 3, 4624, None, 2313),  #   the NaN row inside a whole block (it arrives through M) / the dropped row
    ("nblocks_20", 3, 4624, 20, 4),             # records 20.. are NaN and must not be read: the second half keeps one block
    ("nblocks_10", 3, 4624, 10, 4),             # the first half keeps blocks 1..9, the second none
    ("nblocks_0", 100, 500, 0, 101),
)


def rhat_chain(nw):
    return cached_chain("rhat", RHAT_ROWS, RHAT_NWP, RHAT_PARAMS)[:, :, :nw]


def rhat_image(nw, nanrow):
    """float64 image [rows][nd][nw] with the NaN row in parameter 3."""
    xf = rhat_chain(nw).astype(np.float64)
    if nanrow is not None:
        xf[nanrow, 3, :] = np.nan
    return xf


MEANSTD_PARAMS = (("ar", 0.5), ("ar", 0.9), ("ar", 0.99))
MEANSTD_ROWS, MEANSTD_NWP = 60, 128
# (t0, tm, t1): equal halves from row 0, halves of one row, unequal halves with t0 > 0, an empty first / second half
MEANSTD_WINDOWS = ((0, 20, 40), (7, 8, 9), (7, 10, 31), (7, 7, 20), (7, 20, 20))
# one value per half (a half of one row, one lane) has std = 0 exactly and nothing to bound: not a case
MEANSTD_CASES = tuple((w, nws) for w in MEANSTD_WINDOWS for nws in (1, 127, 128) if not (w == (7, 8, 9) and nws == 1))


def meanstd_chain():
    return cached_chain("meanstd", MEANSTD_ROWS, MEANSTD_NWP, MEANSTD_PARAMS)
