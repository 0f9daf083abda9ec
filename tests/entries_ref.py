"""Input tables and float64 references for the stand-alone ABI entries (tests/test_entries_host.py pins them on the CPU,
tests/test_gpu_entries.py runs the entries of include/linna_hip.h against them).  Not a test module.

Two kinds of table:
 * EXACT tables: small integers (|x| <= 4), weights from {0.5, 1, 2}, scales that are powers of two, T = 2.  Every fp32
   product and every partial sum of such a table is an integer multiple of a small power of two below 2^24, so the fp32
   result does not depend on the order of summation and equals the float64 reference bit for bit.
 * RANDOM tables for what cannot be exact (the fixed 0.1 of a residual block, exp / erf / log columns).
Every table is a pure function of its key (a CRC of the key seeds the generator): nothing is drawn at run time.
Every reference takes the float32 arrays the device gets and computes in float64 (numpy + the pieces of ``oracle/``).
"""
import zlib

import numpy as np

from oracle import likelihood, training

F = np.float32
SENTINEL = 7.0           # pre-fill of every output buffer and of its guard
T_EXACT = 2.0


def ld4(n):
    return (int(n) + 3) & ~3


def rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def ints(key, shape, amax=4):
    """Small integers in [-amax, amax] as float32."""
    return rng("ints", key).randint(-amax, amax + 1, size=shape).astype(F)


def pow2w(key, shape):
    """Weights from {0.5, 1, 2}."""
    return rng("pow2w", key).choice([0.5, 1.0, 2.0], size=shape).astype(F)


def f64(a):
    return np.asarray(a, F).astype(np.float64)


def exact_ok(*term_arrays):
    """The exact-table condition: the sum of |terms| along the last axis (every partial sum in any order is bounded by
    it) stays below 2^24."""
    return all(float(np.abs(f64(t)).sum(axis=-1).max()) < 2.0 ** 24 for t in term_arrays)


def round_once(a):
    """float64 -> float32, one rounding."""
    with np.errstate(over="ignore"):
        return np.asarray(a, np.float64).astype(F)


# ----------------------------------------------------------------------------------------------- linna_val_metrics
VAL_NS = (1, 2, 3, 255, 256, 257, 512, 513, 1000, 65536)
VAL_TABLES = ("distinct", "ties", "equal", "inf", "nan_loss", "nan_frac", "nan_first", "nan_last", "nan_last_loss")
VAL_TABLES_BIG = ("distinct", "ties")          # n = 65536


def val_table_names(n):
    return VAL_TABLES_BIG if n == 65536 else VAL_TABLES


def val_table(n, name):
    """(loss[n], frac[n]) float32.  distinct: a random order of n different values; ties: draws from {-0.0, 0.0, 1, 2};
    equal: one value; inf: +inf at the first, middle and last index; nan_loss / nan_frac: one NaN inside that vector only;
    nan_first: loss[0]; nan_last: frac[n-1] (for n = 257, 513 the only element of the last tile of 256); nan_last_loss:
    loss[n-1]."""
    r = rng("val", n, name)
    distinct = lambda: ((r.permutation(n) - n // 3) * 0.125 + 0.0625).astype(F)
    if name == "ties":
        vals = np.array([-0.0, 0.0, 1.0, 2.0], F)
        return vals[r.randint(0, 4, n)], vals[r.randint(0, 4, n)]
    if name == "equal":
        return np.full(n, 1.5, F), np.full(n, 0.25, F)
    loss, frac = distinct(), distinct()
    if name == "inf":
        for i in {0, n // 2, n - 1}:
            loss[i] = np.inf
        frac[n // 2] = np.inf
    elif name == "nan_loss":
        loss[n // 3] = np.nan
    elif name == "nan_frac":
        frac[n // 3] = np.nan
    elif name == "nan_first":
        loss[0] = np.nan
    elif name == "nan_last":
        frac[n - 1] = np.nan
    elif name == "nan_last_loss":
        loss[n - 1] = np.nan
    elif name != "distinct":
        raise KeyError(name)
    return loss, frac


def val_metrics_ref(loss, frac, last=None):
    """out[4] of linna_val_metrics: {last (NaN if None), lower median of loss, max of frac, lower median of frac}; a NaN
    anywhere in a vector makes its statistics NaN (torch.median / torch.max)."""
    loss, frac = np.asarray(loss, F), np.asarray(frac, F)
    med = lambda a: F(np.nan) if np.isnan(a).any() else F(training.lower_median(a.astype(np.float64)))
    mx = F(np.nan) if np.isnan(frac).any() else F(frac.astype(np.float64).max())
    return np.array([np.nan if last is None else last, med(loss), mx, med(frac)], F)


# ----------------------------------------------------------------------------------------------- layers
def linear_fwd_ref(X, W, b, alpha, R, relu):
    v = f64(X) @ f64(W).T
    if b is not None:
        v = v + f64(b)[None, :]
    v = float(F(alpha)) * v
    if R is not None:
        v = v + f64(R)
    return np.maximum(v, 0.0) if relu else v


def linear_fwd_terms(X, W, b, R):
    """|terms| of one output element of the exact table, summed: bounds every partial sum."""
    t = np.abs(f64(X)) @ np.abs(f64(W)).T
    if b is not None:
        t = t + np.abs(f64(b))[None, :]
    if R is not None:
        t = t + np.abs(f64(R))
    return t


def resblock_fwd_ref(X, W1, b1, W2, b2, Ws):
    """T = relu(X W1^T + b1); Y = relu(0.1 (T W2^T + b2) + X Ws^T)  (Ws None: + X); 0.1 is the float32 constant."""
    T = np.maximum(f64(X) @ f64(W1).T + f64(b1)[None, :], 0.0)
    skip = f64(X) if Ws is None else f64(X) @ f64(Ws).T
    Y = np.maximum(float(F(0.1)) * (T @ f64(W2).T + f64(b2)[None, :]) + skip, 0.0)
    return T, Y


def linear_bwd_ref(dY, X, W, Xmask, scale):
    """dX = scale (dY W) [* (Xmask > 0)], dW = scale dY^T X, db = scale colsum dY."""
    s = float(F(scale))
    dX = s * (f64(dY) @ f64(W))
    if Xmask is not None:
        dX = np.where(f64(Xmask) > 0, dX, 0.0)
    return dX, s * (f64(dY).T @ f64(X)), s * f64(dY).sum(axis=0)


LAYER_SHAPES = ((1, 1, 1), (1, 130, 3), (17, 3, 33), (17, 33, 130), (17, 130, 1), (130, 33, 3), (130, 3, 130), (130, 130, 33))   # (B, K, N)
RESBLOCK_SHAPES = ((1, 1, 1, 1, False), (17, 33, 130, 33, False), (130, 3, 33, 3, False), (17, 3, 33, 130, True), (130, 130, 3, 1, True),
                   (130, 33, 33, 33, True), (1, 130, 130, 3, True))                                                                 # (B, K, C, N, Ws)
COLSUM_B = (1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 113, 1000)
COLSUM_N = (1, 63, 64, 65, 130)
GEMM_EXTRA_SHAPES = tuple((M, N, K) for M in (1, 65) for N in (3, 65) for K in (5, 130))


def linear_exact_table(B, K, N):
    """X, R integers; W from {0.5, 1, 2}; b integer."""
    return dict(X=ints(("linX", B, K, N), (B, K)), W=pow2w(("linW", K, N), (N, K)), b=ints(("linb", K, N), N), R=ints(("linR", B, N), (B, N)))


def linear_random_table(B, K, N):
    r = rng("linrand", B, K, N)
    return dict(X=r.standard_normal((B, K)).astype(F), W=r.standard_normal((N, K)).astype(F), b=r.standard_normal(N).astype(F),
                R=r.standard_normal((B, N)).astype(F))


def resblock_table(B, K, C, N, ws):
    r = rng("resblock", B, K, C, N, ws)
    g = lambda *shape: r.standard_normal(shape).astype(F)
    return dict(X=g(B, K), W1=g(C, K), b1=g(C), W2=g(N, C), b2=g(N), Ws=g(N, K) if ws else None)


def linear_bwd_table(B, K, N):
    """dY, X integers; W from {0.5, 1, 2}; Xmask integers in [-1, 1]: zeros, negatives and positives."""
    return dict(dY=ints(("bwddY", B, K, N), (B, N)), X=ints(("bwdX", B, K, N), (B, K)), W=pow2w(("bwdW", K, N), (N, K)),
                Xmask=ints(("bwdM", B, K, N), (B, K), 1))


def colsum_table(B, N):
    return ints(("colsum", B, N), (B, N))


def gemm_dot_table(M, N, K):
    """A in {-1, 0, 1}, B from {0.5, 1, 2}, bias and dotwith integers: C = A B^T + bias stays small enough for sum_n C^2."""
    return dict(A=ints(("dotA", M, N, K), (M, K), 1), B=pow2w(("dotB", N, K), (N, K)), bias=ints(("dotb", N, K), N, 2),
                dw=ints(("dotw", M, N), (M, N)))


def gemm_exp_table(M, N, K):
    """|A B^T| <= 1, cscale in [0.5, 2], cshift in [-2, 2]: the argument of exp stays inside [-4, 4]."""
    r = rng("gemmexp", M, N, K)
    return dict(A=r.uniform(-1, 1, (M, K)).astype(F), B=(r.uniform(-1, 1, (N, K)) / K).astype(F), cscale=r.uniform(0.5, 2, N).astype(F),
                cshift=r.uniform(-2, 2, N).astype(F), cpost=r.uniform(0.5, 2, N).astype(F), cshift2=r.standard_normal(N).astype(F))


def gemm_bound(ref, k_total):
    """The bound tools/fuzz_gemm.py asserts: max|got - ref| / (max|ref| + 1e-6) < 2e-6 max(8, sqrt(K_total)) + 1e-6."""
    return 2e-6 * max(8.0, float(k_total) ** 0.5) + 1e-6, float(np.abs(ref).max()) + 1e-6


def gemm_epilogue_ref(A, B, bias, cscale, cshift, cexp, cpost, cshift2):
    """epi(A B^T + bias): v = v cscale + cshift; [exp: v = exp(v) cpost + cshift2]; also returns the argument of exp."""
    v = f64(A) @ f64(B).T
    if bias is not None:
        v = v + f64(bias)[None, :]
    if cscale is not None or cshift is not None:
        v = v * (1.0 if cscale is None else f64(cscale)[None, :]) + (0.0 if cshift is None else f64(cshift)[None, :])
    arg = v
    if cexp:
        v = np.exp(v) * (1.0 if cpost is None else f64(cpost)[None, :]) + (0.0 if cshift2 is None else f64(cshift2)[None, :])
    return v, arg


# ----------------------------------------------------------------------------------------------- log-likelihood
DIAG_NOUT = (1, 3, 16, 17, 32, 33, 64, 65, 128, 129, 300)
DIAG_SHAPES = tuple((n, 5) for n in DIAG_NOUT) + ((3, 17), (3, 65), (5, 129))
DIAG_B = (1, 3, 15, 16, 17, 63, 64, 65, 257)
DIAG_RANDOM = ((9, 5), (27, 5), (50, 5), (100, 5), (300, 5))       # one per lanes-per-row value: 4, 8, 16, 32, 64
DENSE_NOUT = (1, 5, 64, 65, 130)
DENSE_B = (1, 65, 300)


def diag_lanes_per_row(nout, nin):
    q = (max(nout, nin) + 3) // 4
    return 64 if q > 32 else 32 if q > 16 else 16 if q > 8 else 8 if q > 4 else 4


def loglike_diag_ref(D, w, Z, T):
    """(-0.5 sum_j d_j^2 w_j) / T - 0.5 |z|^2, NaN -> -inf, per row."""
    D, w, Z = f64(D), f64(w), f64(Z)
    with np.errstate(invalid="ignore"):
        v = (-0.5 * ((D * w[None, :]) * D).sum(-1)) / float(F(T)) - 0.5 * (Z * Z).sum(-1)
    return np.where(np.isnan(v), -np.inf, v)


def loglike_diag_bound(D, w, Z, T):
    """Row-wise error bound of the fp32 kernel against float64.  Each of the nout (nin) terms carries two roundings of its
    products and at most one per addition on its way through the lane's chain and the shuffle tree; a recursive sum of n
    terms errs by at most (n - 1) eps sum|t| (Higham, Accuracy and Stability, eq. 4.4), the products add 2 eps sum|t|,
    the scaling by -0.5 / T and the final addition one eps each of the result's parts:
        |err| <= (nout + nin + 4) 2^-24 ( sum_j |d_j^2 w_j| / (2 T) + sum z^2 / 2 )."""
    D, w, Z = f64(D), f64(w), f64(Z)
    mag = np.abs((D * w[None, :]) * D).sum(-1) / (2.0 * float(F(T))) + (Z * Z).sum(-1) / 2.0
    return (D.shape[1] + Z.shape[1] + 4) * 2.0 ** -24 * mag


def loglike_dense_ref(D, S, Z, T):
    """(-0.5 d S d^T) / T - 0.5 |z|^2 per row, through oracle.likelihood.gaussian_loglike_rows (data = 0)."""
    D, Z = f64(D), f64(Z)
    with np.errstate(invalid="ignore"):
        ll = likelihood.gaussian_loglike_rows(D, np.zeros(D.shape[1]), f64(S))
        v = ll / float(F(T)) + likelihood.lnprior_rows(Z)
    return np.where(np.isnan(v), -np.inf, v)


def diag_exact_table(nout, nin, B):
    return ints(("diagD", nout, nin, B), (B, nout)), pow2w(("diagw", nout), nout), ints(("diagZ", nout, nin, B), (B, nin))


def dense_exact_table(nout, nin, B):
    return ints(("denseD", nout, B), (B, nout)), pow2w(("denseS", nout), (nout, nout)), ints(("denseZ", nin, B), (B, nin))


# ----------------------------------------------------------------------------------------------- prior map
PRIOR_NIN = (1, 5, 64, 65)
PRIOR_B = (1, 3, 300)
Z_GRID = np.array([0.0, 2.0 ** -10, -2.0 ** -10, 1.0, -1.0, 3.0, -3.0, 6.0, -6.0, 9.0, -9.0], F)


def prior_table(nin, B):
    """Columns cycle through six kinds: Gaussian, flat, Gaussian + log10 (theta = 1 + z: zero at z = -1, negative below),
    flat + log10 (lo > 0), Gaussian with other dyadic constants, flat.  Every constant of a Gaussian non-log column is
    dyadic, so its algebra is exact in fp32.  z walks the fixed grid (erf saturates at |z| = 6; +-9)."""
    j = np.arange(nin)
    kind = j % 6
    is_flat = np.isin(kind, (1, 3, 5)).astype(np.int32)
    lg = np.isin(kind, (2, 3)).astype(np.int32)
    a1 = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                   [0.5 * (j % 7) - 1.0, 0.1 + 0.01 * j, 1.0, 0.3 + 0.1 * (j % 5), -2.0 + (j % 3), -1.7 - 0.01 * j]).astype(F)
    a2 = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                   [2.0 ** ((j % 5) - 2), 0.9 + 0.1 * (j % 4), 1.0, 2.5 + 0.01 * j, 0.25, 3.3 + 0.1 * (j % 3)]).astype(F)   # flat: hi - lo
    xmean = np.where((is_flat == 0) & (lg == 0), 0.25 * (j % 9) - 1.0, 0.3 + 0.07 * (j % 11)).astype(F)
    xstd = np.where((is_flat == 0) & (lg == 0), 2.0 ** ((j % 4) - 1), 0.6 + 0.05 * (j % 13)).astype(F)
    b = np.arange(B)
    Z = Z_GRID[(b[:, None] * 7 + j[None, :] * 3) % len(Z_GRID)]
    dX = ints(("priordX", nin, B), (B, nin))
    return dict(Z=Z, is_flat=is_flat, lg=lg, a1=a1, a2=a2, xmean=xmean, xstd=xstd, dX=dX, algebra=(is_flat == 0) & (lg == 0))


def _priors(t):
    a1, a2 = f64(t["a1"]), f64(t["a2"])
    return [{"dist": "flat", "arg1": a1[j], "arg2": a1[j] + a2[j]} if t["is_flat"][j] else {"dist": "gauss", "arg1": a1[j], "arg2": a2[j]}
            for j in range(len(a1))]


def prior_fwd_ref(t):
    """(X, THETA) in float64; a non-finite x (log10 of theta <= 0) is NaN."""
    theta = likelihood.prior_map(f64(t["Z"]), _priors(t))
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(t["lg"][None, :] != 0, np.log10(theta), theta)
        x = (v - f64(t["xmean"])[None, :]) / f64(t["xstd"])[None, :]
    return np.where(np.isfinite(x), x, np.nan), theta


def prior_bwd_ref(t):
    """dz = dx / xstd * [1 / (theta ln 10)] * dtheta/dz - z, chained by hand around oracle.likelihood.prior_map_grad."""
    z = f64(t["Z"])
    pri = _priors(t)
    theta = likelihood.prior_map(z, pri)
    g = f64(t["dX"]) / f64(t["xstd"])[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where(t["lg"][None, :] != 0, g / (theta * np.log(10.0)), g)
        return g * likelihood.prior_map_grad(z, pri) - z


def prior_fwd_f32(t):
    """float32 numpy restatement of the Gaussian, non-log columns (algebra only): x = (z a2 + a1 - xmean) / xstd."""
    th = t["Z"] * t["a2"][None, :] + t["a1"][None, :]
    return (th - t["xmean"][None, :]) / t["xstd"][None, :], th


def prior_bwd_f32(t):
    return (t["dX"] / t["xstd"][None, :]) * t["a2"][None, :] - t["Z"]


# ----------------------------------------------------------------------------------------------- gather + transforms
XFORM_B = (1, 5, 257)
XFORM_W = (1, 3, 33, 65)


def rows_tables(B, ntot):
    """ROWS: None (identity), a permutation's first B entries, a list with repeats that ends in the last row of the set."""
    r = rng("rows", B, ntot)
    rep = r.randint(0, ntot, B).astype(np.int32)
    rep[-1] = ntot - 1
    if B > 1:
        rep[0] = rep[B // 2]
    return {"none": None, "perm": r.permutation(ntot)[:B].astype(np.int32), "repeat": rep}


def gather_table(B, nin):
    """A resident set of B + 3 rows.  Plain columns: integers in [-4, 4], integer mean, power-of-two std (exact in fp32);
    every third column is logged: 1.25 x an integer in [1, 5], generic mean and std."""
    ntot = B + 3
    j = np.arange(nin)
    lg = (j % 3 == 1).astype(np.int32)
    X = ints(("gatherX", B, nin), (ntot, nin))
    X[:, lg != 0] = (np.abs(X[:, lg != 0]) + 1) * F(1.25)
    xmean = np.where(lg != 0, 0.3 + 0.01 * j, (j % 5) - 2).astype(F)
    xstd = np.where(lg != 0, 0.7 + 0.02 * (j % 9), 2.0 ** ((j % 3) - 1)).astype(F)
    return dict(X=X, lg=lg, xmean=xmean, xstd=xstd, ntot=ntot)


def gather_xform_ref(t, rows):
    """XB[i] = (X[rows[i]] (log10 on flagged columns) - mean) / std in float64; rows None = the first B rows."""
    X = f64(t["X"])
    X = X[: t["ntot"] - 3] if rows is None else X[rows]
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(t["lg"][None, :] != 0, np.log10(np.where(t["lg"][None, :] != 0, X, 1.0)), X)
    return (v - f64(t["xmean"])[None, :]) / f64(t["xstd"])[None, :]


def gather_xform_f32(t, rows):
    """float32 restatement of the plain columns."""
    X = t["X"][: t["ntot"] - 3] if rows is None else t["X"][rows]
    return (X - t["xmean"][None, :]) / t["xstd"][None, :]


def loss_consts(nout, kind="exact", cinv="full"):
    """sigma, ymean, ystd, data_norm, Cinv[nout][nout] (float32).  exact: powers of two / small integers, Cinv symmetric from
    {0.5, 1, 2} (``full``) or 0.5 I (``diag``: chi2 = |delta|^2 / 2, so rows at, below and above the floor nout / 2 can be
    built; no masked column); random: generic constants and a positive definite Cinv.  data_norm of column 1 (if any) is the mask sentinel."""
    j = np.arange(nout)
    r = rng("lossc", nout, kind)
    if kind == "exact":
        sigma, ymean, ystd = (2.0 ** (j % 2)).astype(F), ((j % 3) - 1).astype(F), (2.0 ** ((j + 1) % 2)).astype(F)
        dn = ((j % 3) - 1).astype(F)[::-1].copy()
        if cinv == "diag":
            C = 0.5 * np.eye(nout)
        else:
            U = np.triu(r.choice([0.5, 1.0, 2.0], size=(nout, nout)))
            C = U + np.triu(U, 1).T
    else:
        sigma, ymean, ystd = r.uniform(0.5, 2, nout).astype(F), r.standard_normal(nout).astype(F), r.uniform(0.5, 2, nout).astype(F)
        dn = r.standard_normal(nout).astype(F)
        A = r.standard_normal((nout, nout))
        C = A @ A.T / nout + np.eye(nout)
    if nout > 1 and cinv != "diag":
        dn[1] = F(1e-30)
    return dict(sigma=sigma, ymean=ymean, ystd=ystd, dn=dn, Cinv=np.asarray(C, F), nout=nout)


def loss_Y(key, n, nout, kind="exact"):
    """Targets with both sentinels (1e10 in row 1 / column 0, 1e-30 in row 2 / last column, when those rows exist)."""
    Y = ints(("lossY", key), (n, nout), 2) if kind == "exact" else rng("lossY", key).standard_normal((n, nout)).astype(F)
    if n > 1:
        Y[1, 0] = F(1e10)
    if n > 2:
        Y[2, nout - 1] = F(1e-30)
    return Y


def floor_Y(c):
    """Targets for the ``diag`` constants whose normalised residual against data_norm is 0, 1, 2 in every column (rows 0, 1, 2:
    chi2 = 0, nout / 2, 2 nout -- below, at and above the floor) and 1 in all but the first column (row 3: just below)."""
    lvl = np.array([0.0, 1.0, 2.0, 1.0])[:, None] * np.ones((1, c["nout"]))
    lvl[3, 0] = 0.0
    return ((f64(c["dn"])[None, :] + lvl) * f64(c["ystd"])[None, :] + f64(c["ymean"])[None, :]) * f64(c["sigma"])[None, :]


def _unsentinel(a):
    """float64 copy in which the fp32 mask sentinel 1e-30 is the float64 1e-30 oracle.training.aux compares with."""
    a32 = np.asarray(a, F)
    return np.where(a32 == F(1e-30), 1e-30, a32.astype(np.float64))


def loss_targets_ref(c, Y, ylog=0):
    """YN = ((log) (y / sigma) - ymean) / ystd in float64, NaN where masked."""
    Y32 = np.asarray(Y, F)
    masked = (Y32 == F(1e-30)) | (Y32 == F(1e10)) | (c["dn"][None, :] == F(1e-30))
    with np.errstate(invalid="ignore", divide="ignore"):
        v = f64(Y) / f64(c["sigma"])[None, :]
        v = np.log(v) if ylog else v
        yn = (v - f64(c["ymean"])[None, :]) / f64(c["ystd"])[None, :]
    return np.where(masked, np.nan, yn)


def loss_aux(c, pred, Yb):
    """oracle.training.aux in float64 on the float32 inputs: loss rows, chisqMd (floored), chisqnnd, delta, notmask."""
    return training.aux(f64(pred), _unsentinel(Yb), _unsentinel(c["dn"]), f64(c["Cinv"]), c["sigma"], c["ymean"], c["ystd"])


def chi2_md_ref(c, Y):
    """den[n] = max(chisqMd, nout / 2)."""
    return loss_aux(c, np.zeros(np.shape(Y)), Y)[1]


def loss_grad_ref(c, pred, Yb):
    return training.loss_grad(f64(pred), _unsentinel(Yb), _unsentinel(c["dn"]), f64(c["Cinv"]), c["sigma"], c["ymean"], c["ystd"])


def val_rows_ref(c, pred, Y):
    """(loss rows, |chisqnnd / chisqMd - 1| rows): the rows behind oracle.training.val_metric."""
    l, cMd, cnnd, _, _ = loss_aux(c, pred, Y)
    return l, np.abs(cnnd / cMd - 1)


def chi2_terms(c, delta):
    """|delta_i C_ij delta_j| summed over i, j per row: bounds every partial sum of the chi2 GEMM + row-dot."""
    d = np.abs(f64(delta))
    return ((d @ np.abs(f64(c["Cinv"]))) * d).sum(-1)


# ----------------------------------------------------------------------------------------------- AdamW
ADAMW_N = (1, 3, 255, 256, 257, 1027)
BETA1, BETA2, EPS, LR = F(0.9), F(0.999), F(1e-8), F(1e-3)


def adamw_table(n):
    """p, g (three steps' gradients).  Element 0 has g = 0 in every step (m = v = 0 from the zero state).  An element's
    gradient keeps its sign over the steps: m' = 0.9 m + 0.1 g then never cancels (|g - m| / 10 <= |m'| / 0.9), so the
    half-ulp rounding errors of its fp32 operations stay within a few ulps OF THE RESULT -- the unit the 4 ulp bound on m
    and v is asserted in.  (v' = b2 v + (1 - b2) g^2 is a sum of non-negative terms.)"""
    r = rng("adamw", n)
    p = r.standard_normal(n).astype(F)
    sign = np.where(r.randint(0, 2, n) > 0, 1.0, -1.0)
    g = (sign[None, :] * np.exp(r.uniform(-6, 2, (3, n)))).astype(F)
    g[:, 0] = 0
    return p, g


def adamw_ref(p, g, m, v, step, lr, wd):
    """oracle.training.adamw_step in float64 on copies, with the float32 values of beta1 / beta2 / eps / lr the device gets."""
    p, m, v = f64(p).copy(), f64(m).copy(), f64(v).copy()
    return training.adamw_step(p, f64(g), m, v, step, float(F(lr)), float(BETA1), float(BETA2), float(EPS), float(F(wd)))


def adamw_bc(step):
    """hyper[2], hyper[3]: float32(1 - b1^t), float32(sqrt(1 - b2^t)) computed in float64."""
    return F(1.0 - float(BETA1) ** step), F(np.sqrt(1.0 - float(BETA2) ** step))


def ulps(got, ref64):
    """|got - ref| in units of the float32 spacing at ref."""
    r32 = round_once(ref64)
    return np.abs(np.asarray(got, np.float64) - np.asarray(ref64, np.float64)) / np.spacing(np.maximum(np.abs(r32), np.finfo(F).tiny)).astype(np.float64)
