"""numpy restatement of the dense mass of ``method="hmc"`` (hmc_comoments_kernel, hmc_chol_from_comoments_kernel and
hmc_kick_drift_dense_kernel of csrc/hmc.hip, ``BatchedHMC.adapt(adapt_mass="dense")``), on top of
tests/hmc_adapt_emul.py and tests/hmc_mass_emul.py; shared by tests/test_hmc_dense_host.py and tests/test_gpu_hmc_dense.py
(not a test module).

With cov = C C^T and the mass M = cov^-1 the kernels carry the whitened momentum w = C^T p: w ~ N(0, I), K = |w|^2 / 2,
kick w += eps C^T g, drift q += eps C w.

* ``empty_comoments`` / ``merge``: {n, c, S1[slots][nd], S2[slots][nd][nd]} and one batch of rows into them (slot s takes
  rows [s per, (s + 1) per), per = ceil(B / SLOTS); t = (double)x - c).
* ``chol_from_comoments``: slots summed in order, covariance, Stan's shrinkage, Cholesky; (C float32 or None, info).
* ``tri_matvec`` / ``kick_drift``: the kernel's two triangle products, j ascending, a product and then an add in ``dtype``.
* ``transition``: one transition in the whitened form, the kernels' order of operations in ``dtype``;
  ``textbook_transition``: the same the textbook way (p ~ N(0, M), q += eps M^-1 p, K = p^T M^-1 p / 2) in float64.
* ``adapt_run``: ``BatchedHMC.adapt(Madapt, delta, "dense")`` and ``nafter`` transitions on the kernels' Philox draws.
* ``rotated_target``: 8 parameters, N(0, 1) priors, likelihood covariance Q diag(geomspace(0.003, 0.3, 8)^2) Q^T.
"""
import numpy as np

import hmc_adapt_emul as emul
import hmc_mass_emul as memul

SLOTS = 8          # LINNA_HMC_COMOMENT_SLOTS
MAX_NDIM = 128     # LINNA_HMC_DENSE_MAX_NDIM


def comoments_doubles(nd):
    return 1 + nd + SLOTS * (nd + nd * nd)


def empty_comoments(nd, c=None):
    return dict(n=0.0, c=np.zeros(nd) if c is None else np.asarray(c, np.float64).copy(), S1=np.zeros((SLOTS, nd)),
                S2=np.zeros((SLOTS, nd, nd)))


def merge(mom, rows):
    """In place: the ``B`` rows [B, nd] into the slots (the lower triangle of S2 is what the kernel keeps)."""
    x = np.asarray(rows, np.float64)
    B = len(x)
    per = (B + SLOTS - 1) // SLOTS
    for s in range(SLOTS):
        t = x[s * per:(s + 1) * per] - mom["c"]
        mom["S1"][s] += t.sum(0)
        mom["S2"][s] += np.tril(t.T @ t)
    mom["n"] += float(B)
    return mom


def pack(mom, guard=0, fill=0.0):
    """The device layout: n, c, then per slot S1 and S2 (row-major, zeros above the diagonal), ``guard`` doubles behind."""
    parts = [[mom["n"]], mom["c"]]
    for s in range(SLOTS):
        parts += [mom["S1"][s], np.tril(mom["S2"][s]).ravel()]
    return np.concatenate(parts + [np.full(guard, fill)]).astype(np.float64)


def unpack(flat, nd):
    flat = np.asarray(flat, np.float64)
    w = nd + nd * nd
    body = flat[1 + nd:1 + nd + SLOTS * w].reshape(SLOTS, w)
    return dict(n=float(flat[0]), c=flat[1:1 + nd].copy(), S1=body[:, :nd].copy(), S2=body[:, nd:].reshape(SLOTS, nd, nd).copy())


def covariance(mom):
    """(mean, covariance) of the rows merged: slots summed in slot order."""
    n = mom["n"]
    S1, S2 = np.zeros_like(mom["S1"][0]), np.zeros_like(mom["S2"][0])
    for s in range(SLOTS):
        S1 = S1 + mom["S1"][s]
        S2 = S2 + mom["S2"][s]
    S2 = np.tril(S2) + np.tril(S2, -1).T
    with np.errstate(invalid="ignore", divide="ignore"):
        return mom["c"] + S1 / n, (S2 - np.outer(S1, S1) / n) / (n - 1.0)


def shrink(cov, n):
    return cov * n / (n + 5.0) + 1e-3 * 5.0 / (n + 5.0) * np.eye(len(cov))


def chol_from_comoments(mom):
    """(C as float32 or None, info): info 0, k + 1 for a pivot that is not finite and positive, -1 for n < 2 or NaN."""
    n = mom["n"]
    if not n >= 2.0:
        return None, -1
    A = shrink(covariance(mom)[1], n)
    nd = len(A)
    L = np.tril(A)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(nd):
            piv = L[k, k]
            if not (piv > 0.0 and np.isfinite(piv)):
                return None, k + 1
            col = L[k + 1:, k]
            L[k + 1:, k + 1:] -= np.tril(np.outer(col / piv, col))
        d = np.sqrt(np.diag(L))
    return (L / d[None, :]).astype(np.float32), 0


def tri_matvec(T, v, lower, dtype=np.float32):
    """out[b][d] = sum_j T[d][j] v[b][j] over j <= d (``lower``) or j >= d, j ascending, product then add in ``dtype``."""
    f = dtype
    T, v = np.asarray(T, f), np.asarray(v, f)
    nd = T.shape[0]
    d = np.arange(nd)
    acc = np.zeros(v.shape, f)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(nd):
            on = (d >= j) if lower else (d <= j)
            acc = np.where(on[None, :], acc + (T[:, j][None, :] * v[:, j:j + 1]).astype(f), acc).astype(f)
    return acc


def kick_drift(Cl, eps, mul_kick, mul_drift, G, W, X, Q, dtype=np.float32):
    """(W, Q) after hmc_kick_drift_dense_kernel; ``eps`` None: e = 1; ``X`` None: the drift starts from ``Q``."""
    f = dtype
    Cl = np.asarray(Cl, f)
    e = np.ones(len(W), f) if eps is None else np.asarray(eps, f)
    ek, ed = (f(mul_kick) * e).astype(f)[:, None], (f(mul_drift) * e).astype(f)[:, None]
    W = np.asarray(W, f)
    with np.errstate(invalid="ignore", over="ignore"):
        if mul_kick != 0:
            W = (W + (ek * tri_matvec(Cl.T, G, False, f)).astype(f)).astype(f)
        base = np.asarray(Q if X is None else X, f)
        Qn = (base + (ed * tri_matvec(Cl, W, True, f)).astype(f)).astype(f) if mul_drift != 0 else base.copy()
    return W, Qn


def transition(fg, x, lnp, grad, Cl, num_steps, eps, p0, u, dtype=np.float32, kinetic=None):
    """One transition per row under the factor ``Cl`` with the step sizes ``eps[B]``, in the whitened momentum.
    Returns (x, lnp, grad, accepted, alpha, logaccept), as ``hmc_adapt_emul.transition``."""
    f = dtype
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = np.asarray(p0, f)
        H0 = f(0.5) * np.sum(w * w, -1, dtype=f) - lnp
        w, q = kick_drift(Cl, eps, 0.5, 1.0, grad, w, x, None, f)
        for i in range(num_steps):
            l, g = fg(q)
            l, g = np.asarray(l, f), np.asarray(g, f)
            last = i == num_steps - 1
            w, q = kick_drift(Cl, eps, 0.5 if last else 1.0, 0.0 if last else 1.0, g, w, None, q, f)
        H1 = f(0.5) * np.sum(w * w, -1, dtype=f) - l
        dH = H0 - H1
        ratio = np.exp(np.minimum(dH, f(0)))
        acc = (u < ratio) & np.isfinite(l)
        alpha = np.where(np.isfinite(l) & np.isfinite(dH), ratio, f(0)).astype(f)
    if kinetic is not None:
        kinetic.update(p=w, q=q, lnp_new=l, g_new=g, H0=H0)
    xn = np.where(acc[:, None], q, x).astype(f)
    ln = np.where(acc, l, lnp).astype(f)
    gn = np.where(acc[:, None], g, grad).astype(f)
    return xn, ln, gn, acc, alpha, dH


def textbook_transition(fg, x, lnp, grad, M, num_steps, eps, n01, u, kinetic=None):
    """The same transition in float64 the textbook way: p ~ N(0, M) (p = C^-T n01 with C C^T = M^-1, so that the draw is the
    whitened form's), q += eps M^-1 p, p += eps g, K = p^T M^-1 p / 2."""
    M = np.asarray(M, np.float64)
    Minv = np.linalg.inv(M)
    Cl = np.linalg.cholesky(Minv)
    e = np.asarray(eps, np.float64)[:, None]
    x = np.asarray(x, np.float64)
    p = np.linalg.solve(Cl.T, np.asarray(n01, np.float64).T).T
    K = lambda p: 0.5 * np.einsum("bi,ij,bj->b", p, Minv, p)
    H0 = K(p) - lnp
    p = p + 0.5 * e * grad
    q = x
    for i in range(num_steps):
        q = q + e * (p @ Minv.T)
        l, g = fg(q)
        if i < num_steps - 1:
            p = p + e * g
    p = p + 0.5 * e * g
    H1 = K(p) - l
    dH = H0 - H1
    ratio = np.exp(np.minimum(dH, 0.0))
    acc = (u < ratio) & np.isfinite(l)
    if kinetic is not None:
        kinetic.update(p=p, w=p @ Cl, q=q, lnp_new=l, g_new=g, H0=H0)
    return np.where(acc[:, None], q, x), np.where(acc, l, lnp), np.where(acc[:, None], g, grad), acc, ratio, dH


def find_eps(fg, x, lnp, grad, Cl, r0, max_rounds=40, dtype=np.float32):
    """The step-size search under the factor: ``hmc_adapt_emul.find_eps`` at unit mass in the whitened coordinates
    y = C^-1 q, where the dense leapfrog is the plain one (lnP(C y), gradient C^T g)."""
    f = dtype
    C64 = np.asarray(Cl, np.float64)

    def fg_y(y):
        l, g = fg((np.asarray(y, np.float64) @ C64.T).astype(f))
        return np.asarray(l, f), (np.asarray(g, np.float64) @ C64).astype(f)
    y = np.linalg.solve(C64, np.asarray(x, np.float64).T).T.astype(f)
    gy = (np.asarray(grad, np.float64) @ C64).astype(f)
    return emul.find_eps(fg_y, y, lnp, gy, np.ones(C64.shape[0], f), r0, max_rounds, dtype)


def adapt_run(fg, x0, mass, seed, num_steps, Madapt, delta, nafter, max_rounds=40, dtype=np.float32, store=False):
    """``BatchedHMC(mass=mass, seed=seed).adapt(Madapt, delta, "dense")`` and ``run(nafter)`` behind it.  Returns a dict:
    chol (float32), eps (frozen), windows, infos, acc_after[B], x, chain (with ``store``), state."""
    f = dtype
    B, nd = x0.shape
    cur = dict(x=np.asarray(x0, f), step=0, C=np.diag(1.0 / np.sqrt(np.asarray(mass, np.float64))).astype(np.float32))
    cur["lnp"], cur["g"] = (np.asarray(a, f) for a in fg(cur["x"]))

    def search():
        r0 = emul.find_eps_momenta(seed, cur["step"], B, nd)
        return emul.adapt_state(find_eps(fg, cur["x"], cur["lnp"], cur["g"], cur["C"], r0, max_rounds, dtype)[0], dtype)

    def run(st, n, Ma, mom=None, acc_count=None, chain=None):
        for _ in range(n):
            i = cur["step"]
            cur["x"], cur["lnp"], cur["g"], acc, alpha, _ = transition(
                fg, cur["x"], cur["lnp"], cur["g"], cur["C"], num_steps, st["eps"], emul.momenta(seed, i, B, nd),
                emul.uniforms(seed, i, B), dtype)
            emul.dual_average(st, alpha, Ma, delta, dtype)
            cur["step"] = i + 1
            if mom is not None:
                merge(mom, cur["x"])
            if acc_count is not None:
                acc_count += acc
            if chain is not None:
                chain.append(cur["x"].copy())

    st = search()
    windows = memul.mass_windows(Madapt)
    infos = []
    if not windows:
        if Madapt > 0:
            run(st, Madapt + 1, Madapt)
        Mlast = Madapt
    else:
        run(st, windows[0][0], memul.NEVER)
        mom = empty_comoments(nd, cur["x"][0])
        for a, b in windows:
            run(st, b - a, memul.NEVER, mom=mom)
            Cn, info = chol_from_comoments(mom)
            infos.append(info)
            if Cn is not None:
                cur["C"] = Cn
            mom = empty_comoments(nd, mom["c"] + sum(mom["S1"]) / mom["n"])
            st = search()
        Mlast = Madapt - windows[-1][1]
        run(st, Mlast + 1, Mlast)
    acc_after, chain = np.zeros(B, np.int64), ([] if store else None)
    run(st, nafter, Mlast, acc_count=acc_after, chain=chain)
    return dict(chol=cur["C"], eps=st["eps"], windows=windows, infos=infos, acc_after=acc_after, x=cur["x"], state=st,
                chain=np.array(chain) if store else None)


def gaussian_dense_fg(mean, prec, dtype=np.float64):
    """lnP = -(x - mean)^T prec (x - mean) / 2 and its exact gradient."""
    mean, prec = np.asarray(mean, dtype), np.asarray(prec, dtype)

    def fg(q):
        d = np.asarray(q, dtype) - mean
        with np.errstate(over="ignore", invalid="ignore"):
            Pd = d @ prec
            return -0.5 * np.sum(d * Pd, -1), -Pd
    return fg


def prior_likelihood_fg(means, like_prec, dtype=np.float32):
    """The same density the way the device evaluates it: the N(0, 1) priors plus the likelihood about ITS mean,
    lnP = -|z|^2 / 2 - (z - means)^T like_prec (z - means) / 2 (constants dropped).  z - means is of the prior's size in every
    direction, so in float32 the likelihood term cancels far more than ``gaussian_dense_fg`` about the posterior mean does."""
    means, prec = np.asarray(means, dtype), np.asarray(like_prec, dtype)
    half = dtype(0.5)

    def fg(q):
        q = np.asarray(q, dtype)
        d = q - means
        with np.errstate(over="ignore", invalid="ignore"):
            Pd = d @ prec
            return -half * np.sum(q * q, -1) - half * np.sum(d * Pd, -1), -q - Pd
    return fg


_T = {}


def rotated_target():
    """8 parameters with priors N(0, 1) (theta = z), likelihood N(means, Q diag(s^2) Q^T), s = geomspace(0.003, 0.3, 8), Q the
    orthogonal factor of RandomState(1).standard_normal((8, 8)): the posterior in z is Gaussian with precision I + cov^-1."""
    if not _T:
        nd = 8
        sig = np.geomspace(0.003, 0.3, nd)
        Q = np.linalg.qr(np.random.RandomState(1).standard_normal((nd, nd)))[0]
        like = (Q * sig ** 2) @ Q.T
        like = 0.5 * (like + like.T)
        means = np.linspace(-0.2, 0.2, nd)
        prec = np.eye(nd) + np.linalg.inv(like)
        prec = 0.5 * (prec + prec.T)
        cov = np.linalg.inv(prec)
        mz = cov @ np.linalg.solve(like, means)
        ev, V = np.linalg.eigh(cov)
        _T.update(nd=nd, sig=sig, Q=Q, like=like, means=means, prec=prec, cov=cov, mz=mz, axes=V, widths=np.sqrt(ev),
                  priors=[{"param": "p%d" % i, "dist": "gauss", "arg1": 0.0, "arg2": 1.0} for i in range(nd)],
                  fg32_device=prior_likelihood_fg(means, np.linalg.inv(like)), const=-0.5 * (means @ np.linalg.solve(like, means) - mz @ prec @ mz),
                  fg64=gaussian_dense_fg(mz, prec), fg32=gaussian_dense_fg(mz.astype(np.float32), prec.astype(np.float32), np.float32))
    return _T


def mode_start(B, seed=2):
    """``B`` chains at the mode +- 0.01 of the narrowest width."""
    t = rotated_target()
    return (t["mz"][None, :] + 0.01 * t["widths"].min() * np.random.RandomState(seed).standard_normal((B, t["nd"]))).astype(np.float32)


def conditions(what, Cl, eps, eps_diag, acc, chain, t):
    """The four conditions of the adaptation test: eigenvalues of C^-1 cov_z C^-T within [0.8, 1.25]; the median frozen step
    size >= 10 x the diagonal adaptation's; acceptance > 0.4; std along the principal axes within 5 %."""
    Ci = np.linalg.inv(np.asarray(Cl, np.float64))
    ev = np.linalg.eigvalsh(Ci @ t["cov"] @ Ci.T)
    ratio = float(np.median(eps) / np.median(eps_diag))
    proj = (chain.reshape(-1, t["nd"]).astype(np.float64) - t["mz"]) @ t["axes"]
    std = proj.std(0) / t["widths"]
    print("  %s: eigenvalues of C^-1 cov C^-T %.3f ... %.3f, step size median %.4g (diagonal %.4g, ratio %.1f), acceptance %.4f, "
          "std / truth along the principal axes %.3f ... %.3f"
          % (what, ev.min(), ev.max(), np.median(eps), np.median(eps_diag), ratio, np.mean(acc), std.min(), std.max()))
    assert np.all((ev >= 0.8) & (ev <= 1.25)), (what, ev)
    assert ratio >= 10, (what, ratio)
    assert np.mean(acc) > 0.4, (what, np.mean(acc))
    assert np.all(np.abs(std - 1.0) <= 0.05), (what, std)
