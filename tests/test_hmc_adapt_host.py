"""CPU: the HMC sampling method's C ABI, what still raises, and the numpy emulation of the per-chain step size scheme
(tests/hmc_adapt_emul.py) on an analytic Gaussian."""
import os
import re

import numpy as np
import pytest

import hmc_adapt_emul as emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"linna_hmc_start_eps": 23, "linna_hmc_kick_drift_eps": 14, "linna_logprob_grad_leapfrog_eps": 15,
               "linna_hmc_accept_adapt": 32, "linna_hmc_run": 18, "linna_hmc_find_epsilon": 10}


def test_header_declares_the_new_entries_and_the_binding_matches():
    import ctypes
    from linna_amd import _lib
    from test_abi import header_functions
    decl = header_functions()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW_ENTRIES.items():
        assert decl[name] == ("int", nargs), (name, decl.get(name))
        res, args = _lib._SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert hasattr(lib, name)
    # the scalar entries are untouched
    assert decl["linna_hmc_start"] == ("int", 21) and decl["linna_hmc_kick_drift"] == ("int", 13)
    assert decl["linna_logprob_grad_leapfrog"] == ("int", 14) and decl["linna_hmc_accept"] == ("int", 21)
    # struct linna_hmc_state: struct_size, B, ld, (pad), seed, 10 pointers
    assert ctypes.sizeof(_lib.HmcState) == 16 + 8 + 10 * 8
    assert _lib.HmcState._fields_[0][0] == "struct_size" and _lib.HmcState().struct_size == ctypes.sizeof(_lib.HmcState)
    src = open(os.path.join(ROOT, "include", "linna_hip.h")).read()
    body = re.search(r"typedef struct linna_hmc_state \{(.*?)\} linna_hmc_state_t;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl_ in body.split(";") if decl_.strip() for n in decl_.split(",")]
    names = [n.split()[-1].strip("*") for n in names]
    assert names == [f[0] for f in _lib.HmcState._fields_], names


def test_abi_version_is_still_12():
    from linna_amd import _lib
    assert _lib.ABI_VERSION == 12 and _lib.load().linna_abi_version() == 12
    assert re.search(r"#define\s+LINNA_ABI_VERSION\s+12\b", open(os.path.join(ROOT, "include", "linna_hip.h")).read())


def test_bad_arguments_are_refused_without_a_gpu():
    """The entries that take a ``linna_hmc_state_t`` check it before anything is launched."""
    from linna_amd import _lib
    lib = _lib.load()
    assert lib.linna_hmc_run(None, None, None, None, None, None, None, None, 0, 0.65, 0, 1, 1, None, None, None, None, None) == _lib.ERR_INVALID
    assert b"hmc_run" in lib.linna_last_error()
    assert lib.linna_hmc_find_epsilon(None, None, None, None, None, None, None, 0, 40, None) == _lib.ERR_INVALID
    assert lib.linna_hmc_accept_adapt(None, 0, 3, None, 0, None, 0, None, None, 0, None, 0, None, None, 0, None, None, 0, None, None,
                                      None, None, None, None, None, None, None, 0, 0.65, None, None, None) == _lib.ERR_INVALID


def test_nuts_still_raises():
    from linna_amd import sampler, util
    s = sampler.HMCSampler(None, None, None, 3, 8, x0=np.zeros((8, 3)))
    with pytest.raises(NotImplementedError):
        s.sample(None, 10, method="nuts")
    with pytest.raises(NotImplementedError):
        util.run_mcmc(None, ".", "nuts", 3, 8, np.zeros(3), None)


def test_float32_transition_is_the_oracles_with_a_step_size_per_row():
    """``oracle.sampling.hmc_batched_step`` broadcasts a [B, 1] float32 step size: the emulation's float32 transition is that,
    bit for bit, and row b of it is row b of a run at the scalar eps[b]."""
    from oracle import sampling
    rs = np.random.RandomState(3)
    B, nd = 12, 7
    sig = np.linspace(0.05, 0.3, nd)
    fg32 = lambda q: tuple(np.asarray(a, np.float32) for a in emul.gaussian_fg(np.zeros(nd), sig)(q))
    x = (sig * rs.standard_normal((B, nd))).astype(np.float32)
    l, g = fg32(x)
    mass = np.linspace(0.5, 2.0, nd).astype(np.float32)
    p0, u = rs.standard_normal((B, nd)).astype(np.float32), rs.uniform(size=B).astype(np.float32)
    eps = np.array([0.01, 0.02, 0.04, 0.08], np.float32)[np.arange(B) % 4]
    xe, le, ge, acc, alpha, _ = emul.transition(fg32, x, l, g, mass, 3, eps, p0, u)
    xo, lo, go, acco = sampling.hmc_batched_step(fg32, x, l, g, mass, 3, eps[:, None], p0, u)
    assert np.array_equal(xe, xo) and np.array_equal(le, lo) and np.array_equal(ge, go) and np.array_equal(acc, acco)
    assert acc.any() and ((alpha >= 0) & (alpha <= 1)).all()
    for e in np.unique(eps):
        xs, ls, _, accs = sampling.hmc_batched_step(fg32, x, l, g, mass, 3, float(e), p0, u)
        rows = eps == e
        assert np.array_equal(xs[rows], xe[rows]) and np.array_equal(ls[rows], le[rows]) and np.array_equal(accs[rows], acc[rows])


def test_dual_averaging_follows_the_references_recursion():
    """sampler.py:229-240 written out per chain in plain Python floats against the vectorised emulation, across the freeze."""
    rs = np.random.RandomState(1)
    B, Madapt, delta = 5, 6, 0.65
    eps0 = np.array([0.01, 0.1, 1.0, 0.003, 0.5])
    st = emul.adapt_state(eps0, np.float64)
    ref = [dict(eps=e, mu=np.log(10 * e), epsbar=1.0, Hbar=0.0, m=1) for e in eps0]
    for step in range(Madapt + 3):
        alpha = rs.uniform(size=B)
        emul.dual_average(st, alpha, Madapt, delta, np.float64)
        for n, r in enumerate(ref):
            if r["m"] <= Madapt:
                eta = 1.0 / float(r["m"] + 10)
                r["Hbar"] = (1.0 - eta) * r["Hbar"] + eta * (delta - alpha[n] / 1.0)
                r["eps"] = np.exp(r["mu"] - np.sqrt(r["m"]) / 0.05 * r["Hbar"])
                eta = r["m"] ** -0.75
                r["epsbar"] = np.exp((1.0 - eta) * np.log(r["epsbar"]) + eta * np.log(r["eps"]))
            elif r["m"] == Madapt + 1:
                r["eps"] = r["epsbar"]
            r["m"] += 1
        for k in ("eps", "epsbar", "Hbar"):
            np.testing.assert_allclose(st[k], [r[k] for r in ref], rtol=1e-12, err_msg="%s at step %d" % (k, step))
        assert (st["m"] == step + 2).all()
    assert np.array_equal(st["eps"], st["epsbar"])
    # Madapt = 0: the step size is never written
    st = emul.adapt_state(eps0, np.float64)
    emul.dual_average(st, np.full(B, 0.1), 0, delta, np.float64)
    assert np.array_equal(st["eps"], eps0) and (st["m"] == 2).all()


def test_find_eps_is_the_references_search_chain_by_chain():
    """sampler.py:151-184 for one chain at a time (its while loops, float64) against the bounded batched state machine."""
    rs = np.random.RandomState(4)
    B, nd = 40, 7
    sig = np.linspace(2e-3, 0.3, nd)
    gauss = emul.gaussian_fg(np.zeros(nd), sig)

    def fg(q):                                     # a flat prior's wall at |q| = 100: lnP = -inf outside (first trials land there)
        lq, gq = gauss(q)
        return np.where((np.abs(q) > 100).any(-1), -np.inf, lq), gq
    x = sig * rs.standard_normal((B, nd))
    l, g = fg(x)
    r0 = rs.standard_normal((B, nd))
    mass = np.ones(nd)
    got, rounds, left = emul.find_eps(fg, x, l, g, mass, r0, 60, np.float64)
    assert left == 0 and rounds <= 60

    def one(k):
        def la(e):
            out = emul.transition(fg, x[k:k + 1], l[k:k + 1], g[k:k + 1], mass, 1, np.array([e]), r0[k:k + 1], np.zeros(1), np.float64, kinetic=kin)
            return out[5][0]
        kin = {}
        eps, kk = 1.0, 1.0
        v = la(eps)
        while not (np.isfinite(kin["lnp_new"]).all() and np.isfinite(kin["g_new"]).all()):
            kk *= 0.5
            v = la(eps * kk)
        eps = 0.5 * kk * eps
        a = 1.0 if v > np.log(0.5) else -1.0
        while a * v > -a * np.log(2):
            eps = eps * 2.0 ** a
            v = la(eps)
        return eps
    want = np.array([one(k) for k in range(B)])
    assert np.array_equal(got, want), (got, want)
    print("  step sizes found:", dict(zip(*np.unique(got, return_counts=True))), "rounds", rounds)
    assert len(np.unique(got)) > 2


def test_adaptive_run_on_an_analytic_gaussian():
    """The whole scheme in float64 with the exact gradient: 256 chains, 33 dimensions of widths 0.002 ... 0.02, Madapt = 200,
    5 leapfrog steps, 300 transitions on the frozen step sizes."""
    nd, B = 33, 256
    sig = np.linspace(0.002, 0.02, nd)
    fg = emul.gaussian_fg(np.zeros(nd), sig)
    x0 = sig * np.random.RandomState(7).standard_normal((B, nd))
    out = emul.adaptive_run(fg, x0, np.ones(nd), 9, 5, 200, 0.65, 300, dtype=np.float64, store=True)
    assert out["rounds"] <= 40 and out["nactive"] == 0, out["rounds"]
    assert np.isfinite(out["eps"]).all() and (out["eps"] > 0).all() and np.isfinite(out["eps0"]).all() and (out["eps0"] > 0).all()
    e0 = np.log2(out["eps0"])
    assert np.array_equal(e0, np.round(e0))                      # the search moves in powers of two from 1
    assert np.array_equal(out["state"]["eps"], out["state"]["epsbar"]) and (out["state"]["m"] == 502).all()
    std = out["chain"].reshape(-1, nd).std(0)
    print("  rounds %d, eps0 median %.3g, frozen eps median %.3g, acceptance %.3f, std/sigma %.3f ... %.3f"
          % (out["rounds"], np.median(out["eps0"]), np.median(out["eps"]), out["acc_after"].mean() / 300, (std / sig).min(), (std / sig).max()))
    np.testing.assert_allclose(std, sig, rtol=0.05)
