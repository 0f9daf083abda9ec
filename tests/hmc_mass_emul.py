"""numpy restatement of the diagonal mass adaptation of ``method="hmc"`` (``BatchedHMC.adapt``, hmc_moments_kernel and
hmc_mass_from_moments_kernel of csrc/hmc.hip), on top of tests/hmc_adapt_emul.py; shared by
tests/test_hmc_mass_host.py and tests/test_gpu_hmc_mass.py (not a test module).

* ``mass_windows``: Stan's schedule of "slow" windows, ``BatchedHMC.mass_windows``.
* ``empty_moments`` / ``merge``: the running moments {n, mean, M2} and Chan's merge of one batch of rows into them (batch mean,
  batch M2 about that mean, then the merge -- the kernel's order of operations, float64).
* ``mass_from_moments``: 1 / variance with Stan's shrinkage; entries that are not finite and positive keep their mass.
* ``adapt_run``: ``BatchedHMC.adapt(Madapt)`` and ``nafter`` transitions behind it on the kernels' Philox draws.
"""
import numpy as np

import hmc_adapt_emul as emul

NEVER = 2 ** 30          # the Madapt of the segments that must not freeze


def mass_windows(Madapt, init_buffer=75, term_buffer=50, base_window=25):
    Madapt = int(Madapt)
    if Madapt < 20:
        return []
    init, term, base = init_buffer, term_buffer, base_window
    if init + base + term > Madapt:
        init, term = int(0.15 * Madapt), int(0.1 * Madapt)
        base = Madapt - init - term
    out, start, size = [], init, base
    while start < Madapt - term:
        end = start + size
        if end + 2 * size > Madapt - term:          # the next window would not fit: this one runs up to the closing buffer
            end = Madapt - term
        out.append((start, end))
        start, size = end, 2 * size
    return out


def empty_moments(ndim):
    return dict(n=0.0, mean=np.zeros(ndim), M2=np.zeros(ndim))


def merge(mom, rows):
    """In place: the ``B`` rows [B, ndim] into {n, mean, M2}."""
    x = np.asarray(rows, np.float64)
    nb = float(len(x))
    mb = x.sum(0) / nb
    M2b = ((x - mb) ** 2).sum(0)
    n, n1 = mom["n"], mom["n"] + nb
    delta = mb - mom["mean"]
    mom["mean"] = mom["mean"] + delta * nb / n1
    mom["M2"] = mom["M2"] + (M2b + delta * delta * n * nb / n1)
    mom["n"] = n1
    return mom


def mass_from_moments(mom, mass, dtype=np.float32):
    """The new mass (a copy of ``mass`` where the result is not finite and positive, and everywhere for n < 2)."""
    out = np.array(mass, dtype)
    n = mom["n"]
    if not n >= 2.0:
        return out
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        var = np.asarray(mom["M2"], np.float64) / (n - 1.0)
        shrunk = var * n / (n + 5.0) + 1e-3 * 5.0 / (n + 5.0)
        m = (1.0 / shrunk).astype(dtype)
        ok = np.isfinite(m) & (m > 0)
    out[ok] = m[ok]
    return out


def adapt_run(fg, x0, mass, seed, num_steps, Madapt, delta, nafter, adapt_mass=True, max_rounds=40, dtype=np.float32, store=False):
    """``BatchedHMC(seed=seed).adapt(Madapt, delta, adapt_mass)`` and ``run(nafter)`` behind it.  Returns a dict: mass, eps
    (frozen), windows, acc_after[B] (accepted among the last ``nafter``), x, chain (those states, with ``store``), state."""
    f = dtype
    B, nd = x0.shape
    cur = dict(x=np.asarray(x0, f), step=0, mass=np.array(mass, f))
    cur["lnp"], cur["g"] = (np.asarray(a, f) for a in fg(cur["x"]))

    def search():
        r0 = emul.find_eps_momenta(seed, cur["step"], B, nd)          # (step = the transitions done so far)
        eps0 = emul.find_eps(fg, cur["x"], cur["lnp"], cur["g"], cur["mass"], r0, max_rounds, dtype)[0]
        return emul.adapt_state(eps0, dtype)

    def run(st, n, Ma, mom=None, acc_count=None, chain=None):
        for _ in range(n):
            i = cur["step"]
            cur["x"], cur["lnp"], cur["g"], acc, alpha, _ = emul.transition(
                fg, cur["x"], cur["lnp"], cur["g"], cur["mass"], num_steps, st["eps"], emul.momenta(seed, i, B, nd),
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
    windows = mass_windows(Madapt) if adapt_mass else []
    if not windows:
        if Madapt > 0:
            run(st, Madapt + 1, Madapt)
        Mlast = Madapt
    else:
        run(st, windows[0][0], NEVER)
        for a, b in windows:
            mom = empty_moments(nd)
            run(st, b - a, NEVER, mom=mom)
            cur["mass"] = mass_from_moments(mom, cur["mass"], dtype)
            st = search()
        Mlast = Madapt - windows[-1][1]
        run(st, Mlast + 1, Mlast)
    acc_after, chain = np.zeros(B, np.int64), ([] if store else None)
    run(st, nafter, Mlast, acc_count=acc_after, chain=chain)
    return dict(mass=cur["mass"], eps=st["eps"], windows=windows, acc_after=acc_after, x=cur["x"], state=st,
                chain=np.array(chain) if store else None)
