"""Non-finite points, shared by tests/test_nonfinite_host.py and tests/test_gpu_nonfinite.py (not a test module).

A "poisoned" problem is a serving problem of tests/cases.py with ``dolog10index`` on parameter 0 (the reference's
cosmolike_run.py sets ``[0, 1]``) and a Gaussian prior N(1, 1) on it: theta0 = 1 + z0, so that z0 < -1 gives
x0 = (log10(theta0) - mean) / std = NaN and z0 == -1 gives -inf, with every z finite (the prior term -|z|^2 / 2 is finite:
only the network sees the non-finite number).  The reference returns NaN and then -inf there (util.py:1013-1016): a rejected
point.  The scenarios below are what both test files run, so that the host test pins, on the oracle alone, that each of them
really meets such points."""
import numpy as np

import cases

# the eight networks of the serving checks (every segment shape the programs of tests/cases.py hold; v2_40_1000 left out:
# the same program as v2_26_457 at twice the cost)
NETWORKS = ["mlp_33_33", "v2_33_33", "mlp_33_33_dense", "simple_6_4", "v2lin_5_3_log10", "mlp_7_5_small", "v2_4_2_ypos",
            "v2_26_457"]
Z_NAN, Z_ZERO, Z_FAR, Z_CLEAN = -1.5, -1.0, -3.0, 0.2          # theta0 = -0.5 (NaN x), 0 exactly (-inf x), -2 (NaN x); 1.2
# B = 37 on the 16-row engine: the last row of a workgroup, the first of the next, the last of the ragged tail
SERVING_B = 37
SERVING_ROWS = {0: Z_NAN, 15: Z_ZERO, 16: Z_FAR, 36: Z_NAN}
GOLDEN = 0x9E3779B97F4A7C15


def poisoned_problem(name, log_idx=(0,)):
    """A copy of ``cases.serving_problem(name)`` with ``dolog10 = log_idx`` and parameter 0 ~ N(1, 1); parameter 1, if
    listed, flat on [0.1, 2.0] (as the log10 case of tests/cases.py)."""
    prob = dict(cases.serving_problem(name))
    priors = [dict(p) for p in prob["priors"]]
    priors[0] = {"param": "p0", "dist": "gauss", "arg1": 1.0, "arg2": 1.0}
    if 1 in log_idx:
        priors[1] = {"param": "p1", "dist": "flat", "arg1": 0.1, "arg2": 2.0}
    prob["priors"] = priors
    prob["dolog10"] = list(log_idx)
    return prob


def diagonal(prob):
    """The same problem with the diagonal of its inverse covariance (what the bf16 engine serves)."""
    return dict(prob, invcov=np.diag(np.diagonal(np.asarray(prob["invcov"], np.float64)).copy()))


def batch(nin, B=SERVING_B, rows=None, seed=0):
    """(z, twin): z ~ 0.3 N(0, 1) float32 with z0 of the rows ``rows`` = {row: z0} set; the twin carries z0 = 0.2 there."""
    rows = SERVING_ROWS if rows is None else rows
    z = (0.3 * np.random.RandomState(seed).standard_normal((B, nin))).astype(np.float32)
    twin = z.copy()
    for r, v in rows.items():
        z[r, 0] = v
        twin[r, 0] = Z_CLEAN
    return z, twin


def oracle_fn(prob, T, dtype=np.float32, counter=None):
    """q -> lnP by the oracle; ``counter`` (a dict) tallies the points evaluated and those that came out -inf."""
    from oracle import likelihood
    emu = cases.oracle_emulator(prob)

    def f(q):
        with np.errstate(invalid="ignore", divide="ignore"):
            out = likelihood.log_prob(q, emu, prob["priors"], prob["data"], prob["invcov"], T, dtype=dtype)
        if counter is not None:
            counter["n"] = counter.get("n", 0) + len(out)
            counter["ninf"] = counter.get("ninf", 0) + int(np.sum(out == -np.inf))
        return out
    return f


def oracle_grad_fn(prob, T):
    from oracle import likelihood
    emu = cases.oracle_emulator(prob)

    def fg(q):
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            return likelihood.grad_log_prob(q, emu, prob["priors"], prob["data"], prob["invcov"], T)
    return fg


# ----------------------------------------------------------------------- stretch move
STRETCH = dict(name="simple_6_4", T=4.0, nw=64, iters=4, seed=11)


def stretch_start():
    """64 walkers just inside theta0 > 0: z0 = 0.6 |0.5 N(0, 1)| - 0.9 (theta0 >= 0.1), the rest 0.5 N(0, 1)."""
    rs = np.random.RandomState(1)
    x0 = (0.5 * rs.standard_normal((STRETCH["nw"], 6))).astype(np.float32)
    x0[:, 0] = (0.6 * np.abs(x0[:, 0]) - 0.9).astype(np.float32)
    return x0


def stretch_half(coords, logp, S, Cc, lib_seed, step, h, f):
    """The oracle's half step with the draws of the HIP kernels (counter (walker, step, stream = h, 0): x -> the stretch,
    y -> the complementary walker, z -> the Metropolis uniform).  Returns (q, new_lp, accepted, coords, logp)."""
    from oracle import sampling
    bits = sampling.walker_bits(lib_seed, S, step, h, 0)
    u = sampling.u01(bits)
    rint = sampling.scaled_index(bits[:, 1], len(Cc))
    q, fac = sampling.stretch_propose(coords[S], coords[Cc], u[:, 0], rint)
    new_lp = f(q)
    acc = sampling.stretch_accept(logp[S], new_lp, fac, u[:, 2])
    coords, logp = coords.copy(), logp.copy()
    coords[S[acc]] = q[acc]
    logp[S[acc]] = new_lp[acc]
    return q, new_lp, acc, coords, logp


def stretch_lib_seed(seed=None):
    return ((STRETCH["seed"] if seed is None else seed) + GOLDEN) & 0xFFFFFFFFFFFFFFFF


# ----------------------------------------------------------------------- HMC
HMC = dict(name="mlp_7_5_small", T=16.0, B=64, nleap=4, eps=0.05)


def hmc_start():
    """(x0, p0, u, mass): 64 chains near the edge theta0 = 0 (z0 = 0.3 |N(0, 1)| - 0.95), momenta and uniforms given."""
    rs = np.random.RandomState(5)
    B, nd = HMC["B"], 7
    x0 = (0.2 * rs.standard_normal((B, nd))).astype(np.float32)
    x0[:, 0] = (0.3 * np.abs(rs.standard_normal(B)) - 0.95).astype(np.float32)
    p0 = rs.standard_normal((B, nd)).astype(np.float32)
    u = rs.uniform(size=B).astype(np.float32)
    mass = np.linspace(0.5, 2.0, nd).astype(np.float32)
    return x0, p0, u, mass


def hmc_table(ndim):
    """The inputs of the acceptance table, B = 11 chains: dict(U, H0, P, lnp_new, Qnew, Gnew, X, lnp, G, mass, what)."""
    f, B = np.float32, 11
    rs = np.random.RandomState(ndim)
    P = (0.1 * rs.standard_normal((B, ndim))).astype(f)
    mass = np.linspace(0.5, 2.0, ndim).astype(f)
    ke = f(0.5) * np.sum(P * P / mass[None, :], -1, dtype=f)
    lnp_new = np.full(B, -3.0, f)
    H0 = (ke + f(3.0)).astype(f)                    # H0 - H1 ~ 0: ratio ~ 1 unless a row says otherwise
    U = np.full(B, 0.5, f)
    what = ["accept", "reject", "lnp_new -inf", "lnp_new NaN", "NaN in P", "inf in P", "H0 NaN", "H0 +inf", "Gnew NaN",
            "accept (second)", "reject (second)"]
    H0[0] += f(1.0)                                  # energy falls: ratio 1
    H0[1] -= f(5.0)                                  # energy rises by 5: ratio e^-5 < u = 0.5
    lnp_new[2] = -np.inf
    lnp_new[3] = np.nan
    P[4, ndim - 1] = np.nan                          # (the last dimension: the second 64-lane pass at ndim = 70)
    P[5, 0] = np.inf
    H0[6] = np.nan
    H0[7] = np.inf
    H0[9] += f(0.2); U[9] = f(0.9)
    H0[10] -= f(1.0); U[10] = f(0.9)                 # ratio e^-1 = 0.37 < 0.9
    Qn = rs.standard_normal((B, ndim)).astype(f)
    Gn = rs.standard_normal((B, ndim)).astype(f)
    Gn[8, ndim // 2] = np.nan
    X = rs.standard_normal((B, ndim)).astype(f)
    G = rs.standard_normal((B, ndim)).astype(f)
    lnp = np.full(B, -4.0, f) - np.arange(B, dtype=f)
    return dict(U=U, H0=H0, P=P, lnp_new=lnp_new, Qnew=Qn, Gnew=Gn, X=X, lnp=lnp, G=G, mass=mass, what=what)


def hmc_table_expected(t):
    """u < exp(minimum(H0 - H1, 0)) & isfinite(lnp_new): HMCSampler.py:54-59 row by row, in numpy."""
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        ke = f(0.5) * np.sum(t["P"] * t["P"] / t["mass"][None, :], -1, dtype=f)
        H1 = ke - t["lnp_new"]
        return (t["U"] < np.exp(np.minimum(t["H0"] - H1, f(0)))) & np.isfinite(t["lnp_new"])


# ----------------------------------------------------------------------- slice move
SLICE = [dict(name="simple_6_4", T=4.0, nw=64, iters=3, seed=31), dict(name="mlp_7_5_small", T=4.0, nw=34, iters=5, seed=31)]
SLICE_MU, SLICE_XSCALE = 1.0, 0.3
# The one-call half step: ONE stepping-out round (so that every fold of the fusion masks is live) of 16 bracket ends per side,
# two shrinking rounds of 16 trials.  A walker that needs more is left in place and set aside by the replay, and the chains
# start away from equilibrium at an untuned mu: the oracle's own run takes up to 12 stepping-out steps and 13 contractions
# per walker (simple_6_4, its first half step), which tests/test_nonfinite_host.py pins below these sizes.
SLICE_SCHEDULE = ([16], [16, 16])


def slice_start(nw, nd):
    """tests/test_gpu_slice_replay.py ``_run``'s start."""
    return (SLICE_XSCALE * np.random.RandomState(nw + 7).standard_normal((nw, nd))).astype(np.float32)


def ensemble_splits(seed, nw, n):
    """The random equal splits of the first ``n`` iterations of an ``EnsembleSampler(seed=seed)`` (sampler.py ``_draw_splits``)."""
    rs = np.random.RandomState(seed ^ 0x5EED)
    idx = np.arange(nw)
    out = []
    for _ in range(n):
        rs.shuffle(idx)
        out.append(idx.reshape(2, nw // 2).copy())
    return out
