"""numpy restatement of the energy diagnostics of csrc/hmc.hip (hmc_accept_kernel's HmcEnergy group and
hmc_energy_finish_kernel), shared by tests/test_hmc_energy_host.py and tests/test_gpu_hmc_energy.py (not a test module).

* ``accept``: one Metropolis launch in float32 -- H1, the test on given uniforms, and behind it E = acc ? H1 : H0, the energy
  error dH = H1 - H0 and the divergence flag ``!(isfinite(lnp_new) && dH <= max_dH)``.
* ``update``: the float64 accumulators {n, mean, M2, D2, Eprev} per chain, the kernel's recurrence in the kernel's order.
* ``finish``: bfmi = D2 / M2 (NaN for n < 2 or M2 == 0) and pooled = {min bfmi ignoring NaN, sum ndiv, chains with ndiv > 0}.
* ``run``: ``update`` over the rows of an energy series, from empty or from a state.
"""
import numpy as np

DOUBLES = 5                       # LINNA_HMC_ENERGY_DOUBLES: n, mean, M2, D2, Eprev


def divergent(lnp_new, dH, max_dH):
    """The flag of a transition from float32 ``dH``: NaN, a proposal that is not finite, or above ``max_dH`` (equality is not)."""
    with np.errstate(invalid="ignore"):
        return ~(np.isfinite(np.asarray(lnp_new, np.float32)) & (np.asarray(dH, np.float32) <= np.float32(max_dH)))


def accept(P, mass, H0, lnp_new, U, max_dH):
    """hmc_accept_kernel on given uniforms: (acc, E, dH, div), float32.  The kinetic energy is summed in float64 and rounded:
    exact where every term and partial sum is a float32 number (the crafted inputs of the tests), whatever the lane order."""
    f = np.float32
    P, mass, H0, ln, U = (np.asarray(a, f) for a in (P, mass, H0, lnp_new, U))
    with np.errstate(invalid="ignore", over="ignore"):
        ke = np.sum(P.astype(np.float64) ** 2 / mass.astype(np.float64)[None, :], -1).astype(f)
        H1 = (f(0.5) * ke - ln).astype(f)
        d = (H0 - H1).astype(f)
        ratio = np.exp(np.where(d > 0, f(0), d)).astype(f)
        acc = np.isfinite(ln) & (U < ratio)
        E = np.where(acc, H1, H0).astype(f)
        dH = (H1 - H0).astype(f)
    return acc, E, dH, divergent(ln, dH, max_dH)


def empty(B):
    return np.zeros((B, DOUBLES), np.float64)


def update(estate, E):
    """In place: one transition's energies ``E[B]`` into ``estate[B][5]``.  A non-finite E changes nothing of its chain."""
    for b, e in enumerate(np.asarray(E, np.float64)):
        if not np.isfinite(e):
            continue
        n0, mean0, _, _, prev = estate[b]
        n1 = n0 + 1.0
        d = e - mean0
        mean = mean0 + d / n1
        estate[b, 2] += d * (e - mean)
        if n0 >= 1.0:
            t = e - prev
            estate[b, 3] += t * t
        estate[b, 0], estate[b, 1], estate[b, 4] = n1, mean, e
    return estate


def run(E, estate=None):
    """``update`` over the rows of ``E[ntrans][B]``."""
    E = np.asarray(E)
    estate = empty(E.shape[1]) if estate is None else estate
    for row in E:
        update(estate, row)
    return estate


# The narrow problem of the divergence test: a Gaussian of standard deviation 0.01 around theta = 0 behind flat priors on
# [-5, 5] (theta = 10 Phi(z) - 5, d theta / d z = 3.99 at z = 0: sigma_z = 0.0025; the leapfrog is unstable beyond 2 sigma_z).
NARROW = dict(ndim=4, sigma=0.01, B=8, ntrans=10, nleap=5, seed=7, eps_stable=1e-3, eps_unstable=2e-2, max_dH=1000.0)


def narrow_problem():
    """(means, cov, priors, z0[B][ndim] float32, fg64) of ``NARROW``; fg64(q) = (lnP, d lnP / d z) in float64."""
    from oracle import likelihood
    nd, s = NARROW["ndim"], NARROW["sigma"]
    means, cov = np.zeros(nd), np.diag(np.full(nd, s * s))
    priors = [{"param": "p%d" % i, "dist": "flat", "arg1": -5.0, "arg2": 5.0} for i in range(nd)]
    z0 = (0.002 * np.random.RandomState(3).standard_normal((NARROW["B"], nd))).astype(np.float32)

    def fg64(q):
        z = np.asarray(q, np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            d = likelihood.prior_map(z, priors) - means
            return -0.5 * np.sum(d * d, -1) / (s * s) - 0.5 * np.sum(z * z, -1), -(d / (s * s)) * likelihood.prior_map_grad(z, priors) - z
    return means, cov, priors, z0, fg64


def narrow_run(eps):
    """dH[ntrans][B] (float64) of ``NARROW`` at the step size ``eps`` on the kernels' Philox draws, by the float64 leapfrog of
    tests/hmc_adapt_emul.py."""
    import hmc_adapt_emul as emul
    _, _, _, z0, fg = narrow_problem()
    B, nd = z0.shape
    x = z0.astype(np.float64)
    lnp, g = fg(x)
    out = []
    for i in range(NARROW["ntrans"]):
        x, lnp, g, _, _, d = emul.transition(fg, x, lnp, g, np.ones(nd), NARROW["nleap"], np.full(B, eps), emul.momenta(NARROW["seed"], i, B, nd),
                                             emul.uniforms(NARROW["seed"], i, B), np.float64)
        out.append(-d)                                      # (transition returns H0 - H1)
    return np.array(out)


def finish(estate, ndiv):
    """(bfmi[B] float64, pooled[3]): hmc_energy_finish_kernel (its bfmi is this one rounded to float32)."""
    estate, ndiv = np.asarray(estate, np.float64), np.asarray(ndiv)
    ok = (estate[:, 0] >= 2.0) & (estate[:, 2] != 0.0)
    bfmi = np.full(len(estate), np.nan)
    bfmi[ok] = estate[ok, 3] / estate[ok, 2]
    pooled = np.array([np.min(bfmi[ok]) if ok.any() else np.nan, float(ndiv.sum()), float((ndiv > 0).sum())])
    return bfmi, pooled
