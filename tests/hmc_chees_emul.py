"""numpy restatement of the trajectory-length adaptation of ``method="hmc"`` (ChEES-HMC, Hoffman, Radul & Sountsov 2021:
hmc_chees_begin_kernel and hmc_chees_end_kernel of csrc/hmc.hip, ``BatchedHMC.adapt_traj``), in float64 on the kernels'
own Philox draws, on top of tests/hmc_adapt_emul.py and tests/hmc_dense_emul.py; shared by tests/test_hmc_chees_host.py and
tests/test_gpu_hmc_chees.py (not a test module).

* ``halton`` / ``steps`` / ``steps_for``: the base-2 van der Corput number, clamp(ceil(h T / eps), 1, max_steps), and the
  leapfrog steps of the transition at Philox step i after the warm-up.
* ``new_state`` / ``pack``: the state the warm-up starts from and its device layout (include/linna_hip.h).
* ``begin``: m0 and r0 of the positions; ``end``: the state update behind a transition (in place) and the shared step size.
* ``adapt_run``: ``BatchedHMC.adapt_traj(M)`` and ``nafter`` transitions behind it; ``sample``: transitions from where a run
  stopped, with any rule for the number of steps.
* ``lag1``: the lag-1 autocorrelation of a parameter pooled over the chains.
"""
import math

import numpy as np

import hmc_adapt_emul as emul
import hmc_dense_emul as demul

# LINNA_HMC_CHEES_* of include/linna_hip.h (linna_amd/_lib.py holds the same numbers)
HEAD, LR, BETA1, BETA2, ADAM_EPS, ALPHA_FLOOR, MAX_STEPS = 12, 0.025, 0.9, 0.999, 1e-8, 1e-3, 64
WORDS = ("t", "logT", "logTbar", "a", "v", "mu", "Hbar", "logeps", "logepsbar", "g", "hm", "nvalid")


def halton(t):
    h, f, t = 0.0, 0.5, int(t)
    while t > 0:
        if t & 1:
            h += f
        f *= 0.5
        t >>= 1
    return h


def steps(h, T, eps, max_steps=MAX_STEPS):
    r = h * T / eps
    return int(math.ceil(min(r, float(max_steps)))) if r >= 1.0 else 1


def steps_for(i, traj, eps, max_steps=MAX_STEPS):
    return steps(halton(int(i) + 1), traj, eps, max_steps)


def lower_median(v):
    """torch.median's: the lower of the two middle values."""
    v = np.sort(np.asarray(v))
    return v[(len(v) - 1) // 2]


def new_state(eps0):
    eps0 = float(eps0)
    st = dict.fromkeys(WORDS, 0.0)
    st.update(t=1.0, logT=math.log(eps0), mu=math.log(10.0 * eps0), logeps=math.log(eps0))
    return st


def pack(st, m0, m1, guard=0, fill=0.0):
    return np.concatenate([[st[k] for k in WORDS], m0, m1, np.full(guard, fill)]).astype(np.float64)


def begin(x):
    x = np.asarray(x, np.float64)
    m0 = x.sum(0) / float(len(x))
    return m0, ((x - m0) ** 2).sum(-1)


def velocity(p, mass=None, chol=None):
    """The float32 velocity the leapfrog moved the chain with: p / mass, or C w under the factor ``chol``."""
    p = np.asarray(p, np.float32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if chol is not None:
            return demul.tri_matvec(chol, p, True, np.float32)
        return (p / np.asarray(mass, np.float32)[None, :]).astype(np.float32)


def end(st, q, p, alpha, r0, M, delta, max_steps=MAX_STEPS, mass=None, chol=None):
    """hmc_chees_end_kernel: ``st`` in place.  Returns a dict: eps (the float32 step size of every chain), valid[B], m1, c[B]
    (with h_t; of the valid chains, 0 elsewhere) and gscale = sum alpha |c| / sum alpha, the size ``g`` cancels from."""
    q64, al = np.asarray(q, np.float32).astype(np.float64), np.asarray(alpha, np.float32).astype(np.float64)
    B = len(q64)
    t = st["t"]
    h = halton(t)
    with np.errstate(invalid="ignore", over="ignore"):
        valid = (al > 0) & np.isfinite(r0) & np.isfinite(q64).all(-1) & np.isfinite(np.asarray(p, np.float64)).all(-1)
    nvalid = int(valid.sum())
    m1, c, gscale = np.zeros(q64.shape[1]), np.zeros(B), 0.0
    if nvalid:
        qv = q64[valid]
        m1 = qv.sum(0) / float(nvalid)
        v = velocity(np.asarray(p)[valid], mass, chol).astype(np.float64)
        e = qv - m1
        c[valid] = h * ((e * e).sum(-1) - np.asarray(r0)[valid]) * (e * v).sum(-1)
        g = float((al[valid] * c[valid]).sum() / al[valid].sum())
        gscale = float((al[valid] * np.abs(c[valid])).sum() / al[valid].sum())
        G = g * math.exp(st["logT"])
        st["a"] = BETA1 * st["a"] + (1.0 - BETA1) * G
        st["v"] = BETA2 * st["v"] + (1.0 - BETA2) * G * G
        ahat, vhat = st["a"] / (1.0 - BETA1 ** t), st["v"] / (1.0 - BETA2 ** t)
        st["logT"] += LR * ahat / (math.sqrt(vhat) + ADAM_EPS)
        st["g"] = g
    hm = B / float((1.0 / np.maximum(np.where(valid, al, 0.0), ALPHA_FLOOR)).sum())
    eta = 1.0 / (t + emul.T0)
    st["Hbar"] = (1.0 - eta) * st["Hbar"] + eta * (delta - hm)
    st["logeps"] = st["mu"] - math.sqrt(t) / emul.GAMMA * st["Hbar"]
    w = t ** -emul.KAPPA
    st["logepsbar"] = (1.0 - w) * st["logepsbar"] + w * st["logeps"]
    if nvalid:
        st["logTbar"] = (1.0 - w) * st["logTbar"] + w * st["logT"]
    st["logT"] = min(max(st["logT"], st["logeps"]), st["logeps"] + math.log(float(max_steps)))
    freeze = int(t) == int(M)
    if freeze:
        st["logT"] = st["logTbar"]
    st["t"], st["hm"], st["nvalid"] = t + 1.0, hm, float(nvalid)
    return dict(eps=np.float32(math.exp(st["logepsbar"] if freeze else st["logeps"])), valid=valid, m1=m1, c=c, gscale=gscale)


def _transition(fg, cur, L, eps, seed, mass, chol, dtype, kin=None):
    B, nd = cur["x"].shape
    i = cur["step"]
    e = np.full(B, eps, np.float32)
    p0, u = emul.momenta(seed, i, B, nd), emul.uniforms(seed, i, B)
    if chol is not None:
        out = demul.transition(fg, cur["x"], cur["lnp"], cur["g"], chol, L, e, p0, u, dtype, kinetic=kin)
    else:
        out = emul.transition(fg, cur["x"], cur["lnp"], cur["g"], mass, L, e, p0, u, dtype, kinetic=kin)
    cur["x"], cur["lnp"], cur["g"] = out[0], out[1], out[2]
    cur["step"] = i + 1
    return out[3], out[4]


def sample(fg, cur, seed, n, eps, nsteps, mass=None, chol=None, dtype=np.float64):
    """``n`` transitions from ``cur`` (advanced in place) with the shared step size ``eps`` and ``nsteps(i)`` leapfrog steps
    at Philox step i.  Returns (chain[n, B, nd], accepted[B], the steps used)."""
    chain, acc, Ls = [], np.zeros(len(cur["x"]), np.int64), []
    mass = np.ones(cur["x"].shape[1], np.float32) if mass is None and chol is None else mass
    for _ in range(n):
        Ls.append(int(nsteps(cur["step"])))
        acc += _transition(fg, cur, Ls[-1], eps, seed, mass, chol, dtype)[0]
        chain.append(cur["x"].copy())
    return np.array(chain), acc, Ls


def adapt_run(fg, x0, seed, M, delta=0.65, nafter=0, max_steps=MAX_STEPS, mass=None, chol=None, step0=0, max_rounds=40,
              dtype=np.float64):
    """``BatchedHMC(mass, seed=seed).adapt_traj(M, delta, max_steps)`` from Philox step ``step0`` and ``run(nafter)`` behind
    it.  Returns a dict: traj, eps (the frozen float32 step size as a float), eps0, Ls (the warm-up's steps), Ls_after,
    acc_after[B], chain (the ``nafter`` states), cur (where it stopped: x, lnp, g, step), state."""
    f = dtype
    B, nd = np.shape(x0)
    mass = np.ones(nd, np.float32) if mass is None and chol is None else mass
    cur = dict(x=np.asarray(x0, f), step=int(step0))
    cur["lnp"], cur["g"] = (np.asarray(a, f) for a in fg(cur["x"]))
    r = emul.find_eps_momenta(seed, cur["step"], B, nd)
    if chol is not None:
        eps_b = demul.find_eps(fg, cur["x"], cur["lnp"], cur["g"], chol, r, max_rounds, dtype)[0]
    else:
        eps_b = emul.find_eps(fg, cur["x"], cur["lnp"], cur["g"], mass, r, max_rounds, dtype)[0]
    eps0 = float(np.float32(lower_median(eps_b)))
    st, eps, Ls = new_state(eps0), np.float32(eps0), []
    for t in range(1, int(M) + 1):
        Ls.append(steps(halton(t), math.exp(st["logT"]), math.exp(st["logeps"]), max_steps))
        _, r0 = begin(cur["x"].astype(np.float32))
        kin = {}
        _, alpha = _transition(fg, cur, Ls[-1], eps, seed, mass, chol, dtype, kin)
        eps = end(st, kin["q"].astype(np.float32), kin["p"].astype(np.float32), alpha, r0, M, delta, max_steps, mass, chol)["eps"]
    traj, eps = math.exp(st["logT"]), float(eps)
    chain, acc, La = sample(fg, cur, seed, nafter, eps, lambda i: steps_for(i, traj, eps, max_steps), mass, chol, dtype)
    return dict(traj=traj, eps=eps, eps0=eps0, Ls=Ls, Ls_after=La, acc_after=acc, chain=chain, cur=cur, state=st)


def lag1(x):
    """The lag-1 autocorrelation of x[n, B], pooled over the chains about each chain's own mean."""
    x = np.asarray(x, np.float64)
    d = x - x.mean(0)
    return float((d[1:] * d[:-1]).sum() / (d * d).sum())


# ---- the target of the adaptation tests: a Gaussian of widths geomspace(0.02, 0.6, 8); 256 chains from the mode, 300 warm-up
# and 300 stored transitions, Philox seeds 1 ... 5
WIDTHS = np.geomspace(0.02, 0.6, 8)
MEAN = np.linspace(-0.2, 0.2, 8)
SEEDS = (1, 2, 3, 4, 5)
# What the float64 emulation gave over those five seeds (tests/test_hmc_chees_host.py prints them):
# traj / the largest width 1.806 ... 1.888; lag-1 autocorrelation of the widest parameter 0.549 ... 0.581 adapted against
# 0.967 ... 0.970 with 5 fixed steps at the same step size.  The band is [min / 2, 2 max] -- the frozen length is a noisy
# average of a jittered stochastic ascent -- and the margin half the gap between the worst adapted seed and the fixed-5 figure.
TRAJ_BAND = (0.5 * 1.806, 2.0 * 1.888)
LAG1_MARGIN = 0.5 * (0.967 - 0.581)


def start(B, seed):
    """``B`` chains at the mode +- 0.01 of the narrowest width."""
    return (MEAN[None, :] + 0.01 * WIDTHS.min() * np.random.RandomState(seed).standard_normal((B, len(WIDTHS)))).astype(np.float32)


def conditions(what, traj, acc, chain, chain5, widths=WIDTHS):
    """The conditions of the adaptation tests on ``chain[n, B, nd]`` (adapted) and ``chain5`` (5 fixed steps at the same step
    size): std of every parameter within 5 %, acceptance above 0.4, the lag-1 autocorrelation of the widest parameter below
    the fixed-5 one by LAG1_MARGIN, and traj / the largest width inside TRAJ_BAND."""
    nd = len(widths)
    std = chain.reshape(-1, nd).astype(np.float64).std(0) / widths
    wide = int(np.argmax(widths))
    r, r5, ratio = lag1(chain[:, :, wide]), lag1(chain5[:, :, wide]), traj / widths.max()
    print("  %s: traj / the largest width %.3f, acceptance %.4f, std / truth %.3f ... %.3f, lag-1 autocorrelation %.3f (5 fixed steps %.3f)"
          % (what, ratio, np.mean(acc), std.min(), std.max(), r, r5))
    assert np.all(np.abs(std - 1.0) <= 0.05), (what, std)
    assert np.mean(acc) > 0.4, (what, np.mean(acc))
    assert r < r5 - LAG1_MARGIN, (what, r, r5)
    assert TRAJ_BAND[0] <= ratio <= TRAJ_BAND[1], (what, ratio)
