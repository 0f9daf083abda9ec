"""Convergence statistics of a chain: the host restatements and ``DeviceChain`` (linna_amd.sampler re-exports both)."""
import numpy as np
import torch

from . import _lib


def _next_pow_two(n):
    i = 1
    while i < n:
        i <<= 1
    return i


def _autocorr_1d(x):
    x = np.asarray(x, np.float64)
    n = _next_pow_two(len(x))
    f = np.fft.fft(x - np.mean(x), n=2 * n)
    acf = np.fft.ifft(f * np.conjugate(f))[:len(x)].real
    if acf[0] == 0:
        return np.full(len(x), np.nan)
    return acf / acf[0]


def integrated_time(x, c=5.0):
    """Integrated autocorrelation time per parameter of a chain ``x[nstep, nwalker, ndim]``
    (emcee's estimator as called at sampler.py:538 with tol=0: FFT autocorrelation averaged over
    walkers, Sokal window with c = 5)."""
    x = np.atleast_1d(x)
    if x.ndim == 1:
        x = x[:, None, None]
    if x.ndim == 2:
        x = x[:, :, None]
    nt, nw, nd = x.shape
    tau = np.empty(nd)
    for d in range(nd):
        f = np.zeros(nt)
        for k in range(nw):
            f += _autocorr_1d(x[:, k, d])
        f /= nw
        taus = 2.0 * np.cumsum(f) - 1.0
        m = np.arange(len(taus)) < c * taus
        win = int(np.argmin(m)) if np.any(m) else len(taus) - 1      # emcee's auto_window, edge cases included
        tau[d] = taus[win]
    return tau


def _chain3(x):
    x = np.asarray(x, np.float64)
    if x.ndim == 1:
        x = x[:, None, None]
    if x.ndim == 2:
        x = x[:, :, None]
    if x.ndim != 3:
        raise ValueError("a chain is [nstep, nwalker, ndim]")
    return x


def split_rhat(x):
    """Split-R-hat per parameter of the chains ``x[nstep, nwalker, ndim]`` (float64; the definition of include/linna_hip.h:
    Gelman et al. BDA3 / Vehtari et al. 2021 without rank normalisation and folding).  Every walker is cut into its first and
    last ``nstep // 2`` rows; R-hat = sqrt(((n - 1) / n W + B / n) / W) with W the mean within-variance and B / n the variance
    of the means of the 2 nwalker split chains.  NaN where W = 0 or a row of the halves is not finite."""
    x = _chain3(x)
    N = len(x)
    n = N // 2
    if n < 2:
        raise ValueError("split_rhat: %d rows; two halves of at least 2 rows are needed" % N)
    h = np.concatenate([x[:n], x[N - n:]], axis=1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        W = h.var(0, ddof=1).mean(0)
        vp = (n - 1.0) / n * W + h.mean(0).var(0, ddof=1)
        r = np.sqrt(vp / W)
    r[~(W > 0) | ~np.isfinite(h).all((0, 1)) | ~np.isfinite(vp)] = np.nan
    return r


def _ndtri(p):
    """Phi^-1 in float64 for 0 < p < 1: Wichura's algorithm AS 241 (routine PPND16, relative error about 1e-16), as the device
    evaluates it (csrc/chain_rank.hip)."""
    p = np.asarray(p, np.float64)
    q = p - 0.5

    def poly(r, c):
        v = np.full_like(r, c[-1])
        for k in c[-2::-1]:
            v = v * r + k
        return v

    with np.errstate(invalid="ignore", divide="ignore"):
        r = 0.180625 - q * q
        mid = q * poly(r, (3.3871328727963666080e0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
                           4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3)) / \
            poly(r, (1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3, 2.1213794301586595867e+4,
                     3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3))
        t = np.sqrt(-np.log(np.where(q < 0, p, 1.0 - p)))
        r = t - 1.6
        near = poly(r, (1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
                        1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)) / \
            poly(r, (1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
                     1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9))
        r = t - 5.0
        far = poly(r, (6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
                       2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7)) / \
            poly(r, (1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
                     1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15))
        tail = np.where(t <= 5.0, near, far)
        return np.where(np.abs(q) <= 0.425, mid, np.where(q < 0, -tail, tail))


def _rank2(v):
    """Twice the average rank (1-based, ties averaged) of every element of the 1-d array ``v``: an exact integer."""
    order = np.argsort(v, kind="stable")
    sv = v[order]
    lb = np.searchsorted(sv, sv, side="left")
    ub = np.searchsorted(sv, sv, side="right")
    r2 = np.empty(len(v), np.int64)
    r2[order] = lb + ub + 1
    return r2


def _rhat_of_scores(z, n):
    """Split-R-hat of normal scores ``z[2 n rows, nw]`` (the first n rows: first halves, the last n: second halves); every
    split chain's moments are taken relative to its first value, so that constant chains have exactly no variance."""
    h = np.concatenate([z[:n], z[n:]], axis=1)
    rel = h - h[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        W = rel.var(0, ddof=1).mean()
        vp = (n - 1.0) / n * W + (h[0] + rel.mean(0)).var(ddof=1)
        return float(np.sqrt(vp / W)) if W > 0 and np.isfinite(W) and np.isfinite(vp) else np.nan


def rank_rhat(x):
    """Rank-normalised, folded split-R-hat (Vehtari et al. 2021; the definition of include/linna_hip.h) per parameter of the
    chains ``x[nstep, nwalker, ndim]``: ``(rhat, bulk, tail)`` with rhat = max(bulk, tail), float64.  The values are compared
    as float32 (the device's chain).  The pooled values of the 2 nwalker split chains are replaced by the normal scores
    z = Phi^-1((r - 3/8) / (S + 1/4)) of their average ranks r: split-R-hat of z is the bulk R-hat; the same on
    float32(|x - median|) is the folded (tail) R-hat, which sees chains that agree in location but not in scale.  NaN where a
    value of the halves is not finite or the scores have no within-chain variance."""
    x = np.asarray(_chain3(x), np.float32)
    N, nw, nd = x.shape
    n = N // 2
    if n < 2:
        raise ValueError("rank_rhat: %d rows; two halves of at least 2 rows are needed" % N)
    S = 2 * n * nw
    out = np.full((3, nd), np.nan)
    for d in range(nd):
        v = np.concatenate([x[:n, :, d], x[N - n:, :, d]]).reshape(-1) + np.float32(0.0)         # (-0 + 0 = +0)
        if not np.isfinite(v).all():
            continue
        sv = np.sort(v).astype(np.float64)
        med = 0.5 * (sv[S // 2 - 1] + sv[S // 2])
        with np.errstate(over="ignore"):
            zeta = np.abs(v.astype(np.float64) - med).astype(np.float32)
        for k, u in ((1, v), (2, zeta)):
            z = _ndtri((0.5 * _rank2(u) - 0.375) / (S + 0.25)).reshape(2 * n, nw)
            out[k, d] = _rhat_of_scores(z, n)
        out[0, d] = np.nan if np.isnan(out[1, d]) or np.isnan(out[2, d]) else max(out[1, d], out[2, d])
    return out[0], out[1], out[2]


def multichain_ess(x, return_pairs=False):
    """Multi-chain effective sample size per parameter of the chains ``x[nstep, nwalker, ndim]`` (float64; Stan's estimator as
    include/linna_hip.h states it): autocovariances averaged over the chains, rho_k = 1 - (W - A_k) / var+, Geyer's initial
    positive sequence of the pairs rho_2t + rho_2t+1 made monotone, tau at least 1 / log10(nwalker nstep), ESS = nwalker
    nstep / tau.  NaN where a value is not finite or var+ is not positive.  ``return_pairs``: also the last pair index used."""
    x = _chain3(x)
    N, nw, nd = x.shape
    ess, last = np.full(nd, np.nan), np.full(nd, -1.0)
    for d in range(nd):
        y = x[:, :, d]
        if N < 2 or not np.isfinite(y).all():
            continue
        xb = y.mean(0)
        f = np.fft.rfft(y - xb, n=2 * _next_pow_two(N), axis=0)
        A = (np.fft.irfft(f * np.conjugate(f), axis=0)[:N] / N).mean(1)
        W = N / (N - 1.0) * A[0]
        vp = (N - 1.0) / N * W + (xb.var(ddof=1) if nw > 1 else 0.0)
        if not (np.isfinite(W) and np.isfinite(vp) and vp > 0):
            continue
        rho = 1.0 - (W - A) / vp
        npairs = N // 2
        P = rho[0:2 * npairs:2] + rho[1:2 * npairs:2]
        ended = ~(P > 0)
        tend = int(np.argmax(ended)) if ended.any() else npairs
        tau = max(-1.0 + 2.0 * np.sum(np.minimum.accumulate(P[:tend])), 1.0 / np.log10(nw * N))
        ess[d], last[d] = nw * N / tau, tend - 1
    return (ess, last) if return_pairs else ess


def rank_ess(x, return_all=False):
    """Rank-normalised bulk-ESS and tail-ESS (Vehtari et al. 2021; the definition of include/linna_hip.h) per parameter of the
    chains ``x[nstep, nwalker, ndim]``: ``(bulk, tail)``, float64.  The values are compared as float32 (the device's chain).
    The pooled values of the 2 nwalker split chains give three series: the normal scores of their average ranks, rounded to
    float32, and the indicators ``x <= q`` of the 5 % and the 95 % quantile (type 7, integer position arithmetic).  Each
    series' ESS is ``multichain_ess`` of the split chains; tail = min of the two indicators'.  NaN where a value of the halves
    is not finite, or for a series with var+ <= 0.  ``return_all``: also the two quantiles' ESS and the last pair used per
    series ``[ndim, 3]`` (-1 beside a NaN)."""
    x = np.asarray(_chain3(x), np.float32)
    N, nw, nd = x.shape
    n = N // 2
    if n < 2:
        raise ValueError("rank_ess: %d rows; two halves of at least 2 rows are needed" % N)
    S = 2 * n * nw
    ess, last = np.full((nd, 3), np.nan), np.full((nd, 3), -1.0)
    for d in range(nd):
        v = np.concatenate([x[:n, :, d], x[N - n:, :, d]]).reshape(-1) + np.float32(0.0)         # (-0 + 0 = +0)
        if not np.isfinite(v).all():
            continue
        sv = np.sort(v).astype(np.float64)
        series = [_ndtri((0.5 * _rank2(v) - 0.375) / (S + 0.25)).astype(np.float32).astype(np.float64)]
        for num in (1, 19):
            j, r = divmod(num * (S - 1), 20)
            q = sv[j] + (r / 20.0) * (sv[min(j + 1, S - 1)] - sv[j])
            series.append((v.astype(np.float64) <= q).astype(np.float64))
        y = np.stack(series, axis=1).reshape(2 * n, nw, 3)
        ess[d], last[d] = multichain_ess(np.concatenate([y[:n], y[n:]], axis=1), return_pairs=True)
    with np.errstate(invalid="ignore"):
        tail = np.where(np.isnan(ess[:, 1]) | np.isnan(ess[:, 2]), np.nan, np.minimum(ess[:, 1], ess[:, 2]))
    return (ess[:, 0], tail, ess[:, 1], ess[:, 2], last) if return_all else (ess[:, 0], tail)


class DeviceChain(object):
    """The chain of a run kept on the GPU for the convergence statistics, which are computed there INCREMENTALLY.

    The reference recomputes emcee's integrated autocorrelation time of the WHOLE chain every 100 iterations on the
    host (sampler.py:538, 684) -- quadratic in the chain length over a run.  Only the lags up to Sokal's window enter
    that estimate, so this class keeps per (walker, parameter) series the running lagged products ``S_k`` for ``k < K``
    and the running sum in float64 (``linna_acorr_update``: each check adds the products of the ~100 new rows, and takes
    out those of the rows zeus' moving discard drops), and ``linna_acorr_tau`` turns them into emcee's estimate: mean
    removal through prefix sums, normalisation, walker average, cumulative sum, window -- kernels of this library
    (csrc/autocorr.hip), no FFT.  ``K`` starts at 512 lags and grows (new lags computed from the stored chain) whenever
    the window is not found below it or comes within a third of it.  The statistics' copy of the chain is
    ``ct[row][parameter][walker]`` (walkers padded to a multiple of 64).  All work is enqueued on the current stream;
    ``tau_begin`` / ``tau_end`` let a driver collect the result one block later without stalling the sampler.

    Those statistics are within-chain.  For independent chains (``method="hmc"``) ``rhat_begin`` / ``rhat_end`` give
    split-R-hat over all walkers -- from float64 block moments (sum and sum of squares per lane and block of 128 rows,
    ``linna_chain_block_moments``, allocated and filled only once an R-hat is asked for) plus the ragged rows at the ends of
    the two halves -- and ``ess_begin`` / ``ess_end`` Stan's multi-chain effective sample size from the same running sums
    as tau (``linna_acorr_ess``).  ``rank_rhat_begin`` / ``rank_rhat_end`` give the rank-normalised, folded split-R-hat of
    Vehtari et al. 2021 (``linna_chain_rank_rhat``: a radix sort of the pooled values per parameter), which also sees chains
    that agree in location but not in scale, and ``rank_ess_begin`` / ``rank_ess_end`` that paper's bulk-ESS and tail-ESS
    (``linna_chain_rank_ess``: one sort, then the lagged products of the normal scores and of two quantile indicators)."""

    MAX_WALKERS = 1024      # the running sums (8 bytes x lags per series, read and written at every check) cover an evenly spaced
                            # subset of at most so many walkers; the drivers confirm a positive check with ALL walkers (sums
                            # of their own, from the stored chain) before they stop.  None: every walker, always.
    LAGS0 = 512             # initial lag capacity (a multiple of 32)
    RANK_SCRATCH = 1 << 30  # bytes the sort of rank_rhat / rank_ess may take for the parameters of one round (one parameter always fits)

    def __init__(self, max_walkers=-1):
        self.ct = None           # [capacity, nd, nwp] fp32 on the device, grown by doubling
        self.n = 0
        self.nw = self.nd = self.nws = self.nwp = self.nwc = self.wstride = None
        self.max_walkers = self.MAX_WALKERS if max_walkers == -1 else max_walkers
        self._S = self._T = None     # running sums of the window [_lo, _hi) over the subset's lanes
        self._lo = self._hi = 0
        self._scratch = None
        self.lag_growths = 0
        self._M, self._mb = None, 0  # block-moment records [blocks, 2, nd, nwp] float64 and how many are filled (rhat only)
        self._rank_scratch = None    # the sort's buffers (rank_rhat and rank_ess only), bytes

    # -- storage
    def _setup(self, z):
        self.nw, self.nd = int(z.shape[1]), int(z.shape[2])
        self.wstride = 1 if not self.max_walkers else max(1, -(-self.nw // int(self.max_walkers)))
        self.nws = len(range(0, self.nw, self.wstride))
        self.nwp = (self.nw + 63) & ~63              # lanes per parameter in ct: the subset's walkers first, then the others
        self.nwc = (self.nws + 63) & ~63             # lanes the running sums cover
        self.dev = z.device
        self.ctx = _lib.ctx(self.dev.index)

    @property
    def subset(self):
        """True when the routine estimate averages over fewer walkers than the ensemble has."""
        return self.nws < self.nw

    def append(self, z_block):
        z = torch.as_tensor(z_block)
        z = (z if z.is_cuda else z.cuda()).to(torch.float32).contiguous()
        if z.ndim != 3 or len(z) == 0:
            raise ValueError("chain blocks are [nsteps, nwalkers, ndim]")
        if self.ct is None:
            self._setup(z)
        elif (int(z.shape[1]), int(z.shape[2])) != (self.nw, self.nd):
            raise ValueError("chain block of another ensemble")
        need = self.n + len(z)
        if self.ct is None or need > len(self.ct):
            self.ct = self._grown(self.ct, need, 1024, (self.nd, self.nwp), torch.float32, self.n)
        for i0 in range(0, len(z), 32768):                   # (grid.y of the transposing kernel is the step count)
            blk = z[i0:i0 + 32768]
            _lib.call("linna_chain_append_t", self.ctx, _lib.ptr(blk), self.nd, len(blk), self.nw, self.nd, self.wstride,
                      _lib.ptr(self.ct), self.nwp, self.n + i0, _lib.stream())
        self.n = need

    def _grown(self, old, need, floor, tail, dtype, filled=0):
        """A new device buffer [max(need, twice old's rows, floor), *tail] with the first ``filled`` rows of ``old``.  The old one
        may belong to ANOTHER stream's pool (a resumed run fills the chain on the default stream, the in-loop appends run on the
        statistics stream; a check there may still sort in the scratch): the caching allocator must not hand it out meanwhile."""
        buf = torch.empty((max(need, 2 * (0 if old is None else len(old)), floor),) + tail, dtype=dtype, device=self.dev)
        if filled:
            buf[:filled] = old[:filled]
        if old is not None:
            old.record_stream(torch.cuda.current_stream(self.dev))
        return buf

    def __len__(self):
        return self.n

    def last(self, n):
        """The last ``n`` steps as one device tensor [n, nw, nd] (walkers in the ensemble's order)."""
        w = np.arange(self.nw)
        lane = np.where(w % self.wstride == 0, w // self.wstride, self.nws + w - w // self.wstride - 1)
        idx = torch.as_tensor(lane, device=self.dev)
        return self.ct[max(0, self.n - int(n)):self.n].index_select(2, idx).permute(0, 2, 1).contiguous()

    # -- running sums
    def _dptr(self, t):
        return _lib.ptr(t, torch.float64)

    def _update(self, S, T, a0, a1, lo, hi, k0, k1, remove):
        _lib.call("linna_acorr_update", self.ctx, _lib.ptr(self.ct), self.nd, self.nwp, int(S.shape[2]), int(a0), int(a1), int(lo),
                  int(hi), int(k0), int(k1), self._dptr(S), self._dptr(T) if T is not None else None, 1 if remove else 0, _lib.stream())

    def _fresh(self, lags, full=False):
        z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device=self.dev)
        nwc = self.nwp if full else self.nwc
        return z(lags, self.nd, nwc), z(self.nd, nwc)

    def _advance(self, lo, hi):
        """Bring the running sums to the window [lo, hi)."""
        if self._S is None or lo < self._lo or hi < self._hi or lo > self._hi:
            lags = self.LAGS0 if self._S is None else len(self._S)
            self._S, self._T = self._fresh(lags)
            self._lo = self._hi = lo
        if hi > self._hi:
            self._update(self._S, self._T, self._hi, hi, self._lo, hi, 0, len(self._S), False)
            self._hi = hi
        if lo > self._lo:
            self._update(self._S, self._T, self._lo, lo, self._lo, self._hi, 0, len(self._S), True)
            self._lo = lo

    def _grow(self, S, lo, hi, lags):
        """More lags: the old rows are kept, the new ones computed from the stored chain."""
        lags = min((int(lags) + 31) & ~31, (hi - lo + 31) & ~31)
        if lags <= len(S):
            return S
        big = torch.zeros((lags,) + tuple(S.shape[1:]), dtype=torch.float64, device=self.dev)
        big[:len(S)] = S
        self._update(big, None, lo, hi, lo, hi, len(S), lags, False)
        self.lag_growths += 1
        return big

    def _estimate(self, S, T, lo, hi, c, nlive):
        """Enqueue an estimate from the sums -- emcee's tau with Sokal's constant ``c``, the multi-chain ESS with ``c`` None --
        and return the device result [3 nd] (tau | window | more lags needed; ESS | last pair | more lags needed)."""
        kuse = min(len(S), hi - lo) - 1
        nwc = int(S.shape[2])
        entry, sizer, cs = ("linna_acorr_ess", "linna_acorr_ess_scratch_bytes", ()) if c is None else \
            ("linna_acorr_tau", "linna_acorr_scratch_bytes", (float(c),))
        nb = int(getattr(_lib.load(), sizer)(self.nd, nwc, kuse))
        if self._scratch is None or self._scratch.numel() * 8 < nb:
            self._scratch = torch.empty((nb + 7) // 8, dtype=torch.float64, device=self.dev)
        out = torch.empty(3 * self.nd, dtype=torch.float64, device=self.dev)
        _lib.call(entry, self.ctx, _lib.ptr(self.ct), self.nd, self.nwp, nwc, int(nlive),
                  int(lo), int(hi), int(kuse), self._dptr(S), self._dptr(T), *cs, self._dptr(self._scratch), self._dptr(out), _lib.stream())
        return out

    def _estimate_ess(self, S, T, lo, hi, nlive):
        return self._estimate(S, T, lo, hi, None, nlive)

    def _window(self, discard, upto):
        """The rows [lo, hi) of a statistic; ``ValueError`` unless they are stored rows, one at least."""
        hi, lo = self.n if upto is None else int(upto), int(discard)
        if not 0 <= lo < hi <= self.n:
            raise ValueError("empty chain window")
        return lo, hi

    def _hand_off(self, tok, out):
        """``out`` (device) into the token's pinned buffer -- kept when a token is enqueued again for more lags -- and an event behind it."""
        if "pin" not in tok:
            tok["pin"] = torch.empty(out.shape, dtype=torch.float64).pin_memory()
        tok["pin"].copy_(out, non_blocking=True)
        tok["ev"] = torch.cuda.Event()
        tok["ev"].record(torch.cuda.current_stream(self.dev))
        return tok

    def _collect(self, tok):
        """Wait for the token's event; the result as a numpy array of its own, in the shape of the device result."""
        tok["ev"].synchronize()
        return tok["pin"].numpy().copy()

    def tau_begin(self, discard=0, c=5.0, upto=None, all_walkers=False):
        """Enqueue everything a check needs on the current stream -- the sums' update, the estimate, its copy into pinned
        memory -- and return a token for ``tau_end``; nothing waits.  ``all_walkers``: the estimate over every walker of
        the ensemble (sums of their own, computed from the stored chain) instead of the routine subset."""
        lo, hi = self._window(discard, upto)                # (``c`` None: ``ess_begin`` -- both estimates read the same running sums)
        full = bool(all_walkers) and self.subset
        live = (upto is None or hi == self.n) and not full
        if live:
            self._advance(lo, hi)
            S, T = self._S, self._T
        else:                                              # another window, or every walker: sums of their own, from scratch
            S, T = self._fresh(min(len(self._S) if self._S is not None else self.LAGS0, (hi - lo + 31) & ~31), full)
            self._update(S, T, lo, hi, lo, hi, 0, len(S), False)
        nlive = self.nw if full else self.nws
        return self._sums_enqueue(dict(lo=lo, hi=hi, c=c, live=live, S=S, T=T, nlive=nlive))

    def _sums_enqueue(self, tok):
        return self._hand_off(tok, self._estimate(tok["S"], tok["T"], tok["lo"], tok["hi"], tok["c"], tok["nlive"]))

    def _sums_end(self, tok, want_of):
        """The three rows of an estimate [3, nd] (value | window or last pair | more lags needed).  When the estimate asks for
        more lags than are kept they are doubled (new lags from the stored chain) and the estimate repeated -- early in a
        run, while it still grows with the chain; afterwards the capacity stays ahead of what it used (1.5 x)."""
        while True:
            r = self._collect(tok).reshape(3, self.nd)
            lo, hi, S = tok["lo"], tok["hi"], tok["S"]
            if not np.any(r[2] > 0):
                break
            S = self._grow(S, lo, hi, 2 * len(S))
            if tok["live"]:
                self._S = S
            tok["S"] = S
            self._sums_enqueue(tok)
        if tok["live"] and np.all(np.isfinite(r[1])):
            want = want_of(r[1])
            if want > len(self._S) and len(self._S) < ((hi - lo + 31) & ~31):
                self._S = self._grow(self._S, lo, hi, max(want, 2 * len(self._S)))
        return r

    def tau_end(self, tok):
        """The estimate of ``tau_begin`` as numpy [nd].  When Sokal's window lies beyond the lags kept so far they are doubled
        (new lags from the stored chain) and the estimate repeated -- early in a run, while the estimate still grows with
        the chain; afterwards the capacity stays ahead of the window (1.5 x)."""
        r = self._sums_end(tok, lambda win: int(1.5 * float(np.max(win))) + 64)
        self.last_window = r[1]
        return r[0]

    def ess_begin(self, discard=0, upto=None, all_walkers=False):
        """``tau_begin`` for the multi-chain effective sample size (Stan's estimator, include/linna_hip.h) of the window
        [discard, upto): the chains are the lanes the running sums cover -- the walker subset, or with ``all_walkers`` every
        walker (sums of their own).  The sums, ``_advance`` and ``_grow`` are the ones of the tau estimate."""
        return self.tau_begin(discard, None, upto, all_walkers)

    def ess_end(self, tok):
        """The estimate of ``ess_begin`` as numpy [nd] (NaN: a value of the window is not finite).  More lags are added while
        Geyer's positive sequence has not ended within the lags kept."""
        r = self._sums_end(tok, lambda last: int(1.5 * (2.0 * float(np.max(last)) + 2.0)) + 64)
        self.last_pair = r[1]
        return r[0]

    def ess(self, discard=0, upto=None, all_walkers=False):
        return self.ess_end(self.ess_begin(discard, upto, all_walkers))

    # -- split-R-hat from block moments
    def _records(self):
        """The block-moment records of every complete block of ``_lib.RHAT_BLOCK`` stored rows, filled up to the chain's length
        on the current stream.  Nothing exists before the first R-hat is asked for."""
        nb = self.n // _lib.RHAT_BLOCK
        if self._M is None or nb > len(self._M):
            self._M = self._grown(self._M, nb, 64, (2, self.nd, self.nwp), torch.float64, self._mb)
        if nb > self._mb:
            _lib.call("linna_chain_block_moments", self.ctx, _lib.ptr(self.ct), self.nd, self.nwp, self._mb, nb,
                      self._dptr(self._M), _lib.stream())
            self._mb = nb
        return self._M, self._mb

    def rhat_begin(self, discard=0, upto=None, records=True):
        """Enqueue split-R-hat (include/linna_hip.h) of the rows [discard, upto) over ALL walkers on the current stream, its copy
        into pinned memory and an event; returns a token for ``rhat_end``; nothing waits.  ``records=False``: every row is
        read from the stored chain instead of the block moments (the from-scratch route)."""
        lo, hi = self._window(discard, upto)
        M, mb = self._records() if records else (None, 0)
        out = torch.empty((self.nd, 4), dtype=torch.float64, device=self.dev)
        _lib.call("linna_chain_rhat", self.ctx, _lib.ptr(self.ct), self.nd, self.nwp, self.nw, lo, hi,
                  self._dptr(M) if M is not None else None, int(mb), self._dptr(out), _lib.stream())
        return self._hand_off(dict(lo=lo, hi=hi), out)

    def rhat_end(self, tok):
        """R-hat per parameter as numpy [nd] (NaN: no within-chain variance, or a value that is not finite);
        ``last_rhat`` keeps all four columns (R-hat, W, var+, grand mean)."""
        self.last_rhat = self._collect(tok)
        return self.last_rhat[:, 0].copy()

    def rhat(self, discard=0, upto=None, records=True):
        return self.rhat_end(self.rhat_begin(discard, upto, records))

    # -- rank-normalised, folded split-R-hat (a sort of the pooled values per parameter: csrc/chain_rank.hip)
    def rank_rhat_begin(self, discard=0, upto=None):
        """Enqueue the rank-normalised, folded split-R-hat (include/linna_hip.h) of the rows [discard, upto) over ALL walkers on
        the current stream, its copy into pinned memory and an event; returns a token for ``rank_rhat_end``; nothing waits.
        The sort's scratch exists only once this is asked for and grows by doubling; as many parameters as ``RANK_SCRATCH``
        bytes hold share the launches of a round (at least one)."""
        lo, hi = self._window(discard, upto)
        rows = (hi - lo) // 2 * 2
        lib = _lib.load()
        one = int(lib.linna_chain_rank_rhat_scratch_bytes(self.nd, self.nw, rows, 1)) if rows >= 4 else 0
        npar = max(1, min(self.nd, int(self.RANK_SCRATCH) // max(one, 1)))
        need = int(lib.linna_chain_rank_rhat_scratch_bytes(self.nd, self.nw, rows, npar)) if one else 8
        if self._rank_scratch is None or self._rank_scratch.numel() < need:
            self._rank_scratch = self._grown(self._rank_scratch, need, 0, (), torch.uint8)
        out = torch.empty((self.nd, 4), dtype=torch.float64, device=self.dev)
        _lib.call("linna_chain_rank_rhat", self.ctx, _lib.ptr(self.ct), self.nd, self.nwp, self.nw, lo, hi,
                  _lib.ptr(self._rank_scratch, torch.uint8), int(self._rank_scratch.numel()), None, self._dptr(out), _lib.stream())
        return self._hand_off(dict(lo=lo, hi=hi), out)

    def rank_rhat_end(self, tok):
        """max(bulk, tail) R-hat per parameter as numpy [nd] (NaN: no within-chain variance of the scores, or a value that is
        not finite); ``last_rank_rhat`` keeps all four columns (maximum, bulk R-hat, tail R-hat, median)."""
        self.last_rank_rhat = self._collect(tok)
        return self.last_rank_rhat[:, 0].copy()

    def rank_rhat(self, discard=0, upto=None):
        return self.rank_rhat_end(self.rank_rhat_begin(discard, upto))

    # -- rank-normalised bulk-ESS and tail-ESS (one sort per parameter, then the lagged products of the scores image)
    def rank_ess_begin(self, discard=0, upto=None):
        """Enqueue the rank-normalised bulk-ESS and tail-ESS (include/linna_hip.h) of the rows [discard, upto) over ALL walkers on
        the current stream, its copy into pinned memory and an event; returns a token for ``rank_ess_end``; nothing waits.
        The scratch is the one of ``rank_rhat_begin``, grown to the larger need.  The first call asks for the lags below
        ``LAGS0`` (all of them, for halves shorter than that)."""
        lo, hi = self._window(discard, upto)
        return self._rank_ess_enqueue(dict(lo=lo, hi=hi, kuse=min((hi - lo) // 2 - 1, self.LAGS0 - 1)))

    def _rank_ess_enqueue(self, tok):
        lo, hi, kuse = tok["lo"], tok["hi"], tok["kuse"]
        rows = (hi - lo) // 2 * 2
        lib = _lib.load()
        one = int(lib.linna_chain_rank_ess_scratch_bytes(self.nd, self.nw, rows, kuse, 1))       # (0: a window the entry refuses)
        npar = max(1, min(self.nd, int(self.RANK_SCRATCH) // max(one, 1)))
        need = int(lib.linna_chain_rank_ess_scratch_bytes(self.nd, self.nw, rows, kuse, npar)) if one else 8
        if self._rank_scratch is None or self._rank_scratch.numel() < need:
            self._rank_scratch = self._grown(self._rank_scratch, need, 0, (), torch.uint8)
        out = torch.empty((self.nd, 8), dtype=torch.float64, device=self.dev)
        _lib.call("linna_chain_rank_ess", self.ctx, _lib.ptr(self.ct), self.nd, self.nwp, self.nw, lo, hi, int(kuse),
                  _lib.ptr(self._rank_scratch, torch.uint8), int(self._rank_scratch.numel()), self._dptr(out), _lib.stream())
        return self._hand_off(tok, out)

    def rank_ess_end(self, tok):
        """``(bulk, tail)`` ESS per parameter as numpy [nd] each (NaN: a value that is not finite, or a series without
        variance); ``last_rank_ess`` keeps all eight columns (bulk, tail, the 5 % and the 95 % quantile's ESS, the three
        series' last pairs, status).  While a series' positive sequence has not ended within the lags asked for, four times
        as many are asked for, up to every lag of a half (sticky chains keep their pairs positive that far)."""
        while True:
            r = self._collect(tok)
            if not np.any(r[:, 7] > 0):
                break
            tok["kuse"] = min((tok["hi"] - tok["lo"]) // 2 - 1, 4 * (tok["kuse"] + 1) - 1)
            self._rank_ess_enqueue(tok)
        self.last_rank_ess = r
        return r[:, 0].copy(), r[:, 1].copy()

    def rank_ess(self, discard=0, upto=None):
        return self.rank_ess_end(self.rank_ess_begin(discard, upto))

    def integrated_time(self, discard=0, c=5.0, upto=None, all_walkers=False):
        """emcee's estimator (autocovariance of the mean-removed series normalised at lag 0, averaged over walkers, Sokal
        window, tol=0) per parameter -> numpy [nd]; ``discard`` leading steps are dropped (zeus: 20 %); ``upto``: only the
        first ``upto`` steps (the chain as it was at an earlier check); ``all_walkers``: see ``tau_begin``."""
        return self.tau_end(self.tau_begin(discard, c, upto, all_walkers))

    def checkmeanstd(self, nlast, meanshift, stdshift):
        """sampler.py:370-387 on the last ``nlast`` steps: first-half / second-half drift (moments: linna_chain_meanstd)."""
        t0 = max(0, self.n - int(nlast))
        half = int((self.n - t0) / 2)
        out = torch.empty((self.nd, 2, 2), dtype=torch.float64, device=self.dev)
        _lib.call("linna_chain_meanstd", self.ctx, _lib.ptr(self.ct), self.nd, self.nwp, self.nw, t0, t0 + half, self.n,
                  self._dptr(out), _lib.stream())
        m = out.cpu().numpy()
        with np.errstate(invalid="ignore", divide="ignore"):
            meanshifte = np.median(np.abs(m[:, 0, 0] - m[:, 1, 0]) / m[:, 1, 1])
            stdshifte = np.median((m[:, 0, 1] - m[:, 1, 1]) / m[:, 1, 1])
        print(meanshifte, stdshifte, flush=True)
        return bool((meanshifte < meanshift) and (stdshifte < stdshift))


def checkmeanstd(samples, meanshift, stdshift):
    """sampler.py:370-387: first-half / second-half drift of mean and standard deviation."""
    half = int(len(samples) / 2)
    a = samples[:half].reshape(-1, samples.shape[-1])
    b = samples[half:].reshape(-1, samples.shape[-1])
    meanshifte = np.median(np.abs(np.mean(a, axis=0) - np.mean(b, axis=0)) / np.std(b, axis=0))
    stdshifte = np.median((np.std(a, axis=0) - np.std(b, axis=0)) / np.std(b, axis=0))
    print(meanshifte, stdshifte, flush=True)
    return (meanshifte < meanshift) & (stdshifte < stdshift)
