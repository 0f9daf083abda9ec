"""numpy restatement of the per-chain step size HMC of csrc/hmc.hip, shared by tests/test_hmc_adapt_host.py and
tests/test_gpu_hmc_adapt.py (not a test module).

* ``transition``: one transition of every chain with a step size per chain -- ``oracle.sampling.hmc_batched_step`` with
  ``step_size[B, 1]`` in float32 (bit for bit, pinned by the host test), any dtype otherwise, and the acceptance
  probability ``alpha`` the dual averaging feeds on.
* ``dual_average``: hmc_accept_kernel's update of (eps, epsbar, Hbar, m) -- the reference's NUTSMove.propose,
  sampler.py:229-240, with nalpha = 1, gamma 0.05, t0 10, kappa 0.75.
* ``find_eps``: hmc_find_eps_kernel's state machine, the reference's find_reasonable_epsilon (sampler.py:151-184) for all
  chains at once in a bounded number of rounds.
* ``momenta`` / ``uniforms`` / ``find_eps_momenta``: the Philox draws of the kernels (stream 1 / 2 / 3).
* ``adaptive_run``: find_eps, Madapt adaptive transitions, the freeze, and what follows, on those draws.
"""
import numpy as np

from oracle import sampling

GAMMA, T0, KAPPA = 0.05, 10.0, 0.75
LN2 = 0.693147180559945


def momenta(seed, step, B, ndim):
    """hmc_start_kernel's standard-normal draws [B, ndim] at Philox step ``step`` (normal_draw, stream 1)."""
    return _normals(seed, step, 1, B, ndim)


def find_eps_momenta(seed, step, B, ndim):
    """hmc_find_eps_init_kernel's r0 (stream 3)."""
    return _normals(seed, step, 3, B, ndim)


def _normals(seed, step, stream, B, ndim):
    out = np.empty((B, ndim), np.float32)
    w = np.arange(B)
    for sub in range((ndim + 1) // 2):
        u = sampling.u01(sampling.walker_bits(seed, w, step, stream, sub + 1))
        out[:, 2 * sub] = sampling.normal_from_uniform(u[:, 0], u[:, 1])
        if 2 * sub + 1 < ndim:
            out[:, 2 * sub + 1] = sampling.normal_from_uniform(u[:, 2], u[:, 3])
    return out


def uniforms(seed, step, B):
    """The Metropolis uniforms of hmc_accept_kernel (stream 2, sub 0, first word)."""
    return sampling.u01(sampling.walker_bits(seed, np.arange(B), step, 2, 0))[:, 0]


def transition(fg, x, lnp, grad, mass, num_steps, eps, p0, u, dtype=np.float32, kinetic=None):
    """One transition per row with the step sizes ``eps[B]``; the kernels' order of operations in ``dtype``.
    Returns (x, lnp, grad, accepted, alpha, logaccept); ``kinetic`` (a dict) receives p at the end."""
    f = dtype
    mass = np.asarray(mass, f)[None, :]
    e = np.asarray(eps, f)[:, None]
    ek = f(0.5) * e
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        p = p0.astype(f) * np.sqrt(mass)
        H0 = f(0.5) * np.sum(p * p / mass, -1, dtype=f) - lnp
        q = x.astype(f)
        g = grad
        p = p + ek * g
        for i in range(num_steps):
            q = q + e * (p / mass)
            l, g = fg(q)
            l, g = np.asarray(l, f), np.asarray(g, f)
            if i < num_steps - 1:
                p = p + e * g
        p = p + ek * g
        H1 = f(0.5) * np.sum(p * p / mass, -1, dtype=f) - l
        dH = H0 - H1
        ratio = np.exp(np.minimum(dH, f(0)))
        acc = (u < ratio) & np.isfinite(l)
        alpha = np.where(np.isfinite(l) & np.isfinite(dH), ratio, f(0)).astype(f)
    if kinetic is not None:
        kinetic.update(p=p, q=q, lnp_new=l, g_new=g, H0=H0)
    xn = np.where(acc[:, None], q, x).astype(f)
    ln = np.where(acc, l, lnp).astype(f)
    gn = np.where(acc[:, None], g, grad).astype(f)
    return xn, ln, gn, acc, alpha, dH


def adapt_state(eps, dtype=np.float32):
    """NUTSMove.__init__ (sampler.py:198-208): mu = log(10 eps), epsbar = 1, Hbar = 0, m = 1."""
    eps = np.asarray(eps, dtype)
    return dict(eps=eps.copy(), epsbar=np.ones_like(eps), Hbar=np.zeros_like(eps), mu=np.log(dtype(10) * eps).astype(dtype),
                m=np.ones(len(eps), np.int64))


def dual_average(st, alpha, Madapt, delta, dtype=np.float32):
    """In place: sampler.py:229-240 for every chain (``alpha / nalpha`` with nalpha = 1).  Madapt = 0: only m += 1."""
    f = dtype
    m = st["m"]
    if Madapt > 0:
        on = m <= Madapt
        if on.any():
            fm = m[on].astype(f)
            eta = f(1) / (fm + f(T0))
            Hb = (f(1) - eta) * st["Hbar"][on] + eta * (f(delta) - np.asarray(alpha, f)[on])
            e = np.exp(st["mu"][on] - np.sqrt(fm) / f(GAMMA) * Hb)
            eta = f(1) / (np.sqrt(fm) * np.sqrt(np.sqrt(fm)))
            eb = np.exp((f(1) - eta) * np.log(st["epsbar"][on]) + eta * np.log(e))
            st["Hbar"][on], st["eps"][on], st["epsbar"][on] = Hb.astype(f), e.astype(f), eb.astype(f)
        fr = m == Madapt + 1
        st["eps"][fr] = st["epsbar"][fr]
    st["m"] = m + 1
    return st


def find_eps(fg, x, lnp, grad, mass, r0, max_rounds=40, dtype=np.float32):
    """hmc_find_eps_kernel, round by round.  Returns (eps[B], rounds, nactive): ``rounds`` = the rounds after which no chain
    was searching any more (max_rounds if some still were), ``nactive`` = the chains still searching at the end."""
    f = dtype
    B = len(x)
    eps = np.ones(B, f)
    st = np.zeros(B, np.int64)                     # 0 halving, +1 / -1 direction, 2 finished
    rounds = max_rounds
    for r in range(max_rounds):
        kin = {}
        la = transition(fg, x, lnp, grad, mass, 1, eps, r0, np.zeros(B, f), dtype, kinetic=kin)[5]
        bad = ~np.isfinite(kin["lnp_new"]) | ~np.isfinite(kin["g_new"]).all(-1)
        new_eps, new_st = eps.copy(), st.copy()
        with np.errstate(invalid="ignore"):
            z = st == 0
            halve = z & bad
            new_eps[halve] = eps[halve] * f(0.5)
            go = z & ~bad
            a = np.where(la > -f(LN2), 1, -1)
            cont = a.astype(f) * la > -a.astype(f) * f(LN2)
            new_eps[go] = eps[go] * f(0.5)
            mv = go & cont
            new_eps[mv] = new_eps[mv] * np.where(a[mv] > 0, f(2), f(0.5))
            new_st[go] = np.where(cont[go], a[go], 2)
            on = (st == 1) | (st == -1)
            cont = st.astype(f) * la > -st.astype(f) * f(LN2)
            mv = on & cont
            new_eps[mv] = eps[mv] * np.where(st[mv] > 0, f(2), f(0.5))
            new_st[on & ~cont] = 2
        eps, st = new_eps, new_st
        if (st == 2).all():
            rounds = r + 1
            break
    return eps, rounds, int((st != 2).sum())


def adaptive_run(fg, x0, mass, seed, num_steps, Madapt, delta, nafter, max_rounds=40, dtype=np.float32, store=False):
    """``BatchedHMC.find_reasonable_epsilon()``; ``run(Madapt + 1, Madapt=Madapt)``; ``run(nafter, Madapt=Madapt)`` on the
    Philox draws of a fresh ``BatchedHMC(seed=seed)``.  Returns a dict: eps0 (after the search), rounds, nactive, eps (frozen),
    acc_after[B] (accepted transitions among the last ``nafter``), x, chain (the last ``nafter`` states, with ``store``)."""
    f = dtype
    B, nd = x0.shape
    x = np.asarray(x0, f)
    lnp, g = fg(x)
    lnp, g = np.asarray(lnp, f), np.asarray(g, f)
    eps0, rounds, nactive = find_eps(fg, x, lnp, g, mass, find_eps_momenta(seed, 0, B, nd), max_rounds, dtype)
    st = adapt_state(eps0, dtype)
    acc_after = np.zeros(B, np.int64)
    chain = []
    for i in range(Madapt + 1 + nafter):
        x, lnp, g, acc, alpha, _ = transition(fg, x, lnp, g, mass, num_steps, st["eps"], momenta(seed, i, B, nd), uniforms(seed, i, B), dtype)
        dual_average(st, alpha, Madapt, delta, dtype)
        if i > Madapt:
            acc_after += acc
            if store:
                chain.append(x.copy())
    return dict(eps0=eps0, rounds=rounds, nactive=nactive, eps=st["eps"], acc_after=acc_after, x=x, state=st,
                chain=np.array(chain) if store else None)


def gaussian_fg(mean, sigma, dtype=np.float64):
    """lnP = -|x - mean|^2 / (2 sigma^2) per dimension and its exact gradient."""
    mean, s2 = np.asarray(mean, dtype), np.asarray(sigma, dtype) ** 2

    def fg(q):
        d = np.asarray(q, dtype) - mean
        with np.errstate(over="ignore", invalid="ignore"):
            return -0.5 * np.sum(d * d / s2, -1), -d / s2
    return fg
