"""CPU: the dense mass of ``method="hmc"`` without a GPU -- the six entries in the header and the binding, their argument
checks, the whitening identity the kernels rest on, the emulated co-moments and Cholesky factor against numpy, the keyword
handling, and the emulated dense adaptation (tests/hmc_dense_emul.py) on the rotated target."""
import ctypes as C
import os

import numpy as np
import pytest

import hmc_adapt_emul as emul
import hmc_dense_emul as demul
import hmc_mass_emul as memul

ENTRIES = {"linna_hmc_comoments_doubles": 1, "linna_hmc_comoments": 7, "linna_hmc_chol_from_comoments": 8,
           "linna_hmc_kick_drift_dense": 17, "linna_hmc_run_dense": 21, "linna_hmc_find_epsilon_dense": 12}


def test_entries_are_declared_and_bound():
    from test_abi import header_functions
    from linna_amd import _lib
    decl = header_functions()
    for name, nargs in ENTRIES.items():
        assert decl[name][1] == nargs == len(_lib._SIGNATURES[name][1]), name
    assert decl["linna_hmc_comoments_doubles"][0] == "size_t" and _lib._SIGNATURES["linna_hmc_comoments_doubles"][0] is C.c_size_t
    assert _lib.ABI_VERSION == 12 and _lib.load().linna_abi_version() == 12
    assert C.sizeof(_lib.HmcState) == 104
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "linna_hip.h")).read()
    assert "#define LINNA_HMC_COMOMENT_SLOTS 8" in src and "#define LINNA_HMC_DENSE_MAX_NDIM 128" in src


def test_entries_validate_without_a_gpu():
    from linna_amd import _lib
    lib = _lib.load()
    assert lib.linna_hmc_comoments_doubles(33) == 1 + 33 + 8 * (33 + 1089) == demul.comoments_doubles(33)
    assert lib.linna_hmc_comoments_doubles(1) == 1 + 1 + 8 * 2 and lib.linna_hmc_comoments_doubles(128) == 1 + 128 + 8 * (128 + 128 * 128)
    assert lib.linna_hmc_comoments_doubles(0) == 0 and lib.linna_hmc_comoments_doubles(129) == 0
    p = C.c_void_p(64)                       # (never dereferenced: every call below is refused before a launch)
    st = _lib.HmcState()
    bad, uns = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    assert lib.linna_hmc_comoments(None, 4, 3, None, 4, p, None) == bad
    assert lib.linna_hmc_comoments(None, 4, 3, p, 4, None, None) == bad
    assert lib.linna_hmc_comoments(None, 0, 3, p, 4, p, None) == bad
    assert lib.linna_hmc_comoments(None, 4, 5, p, 4, p, None) == bad                     # ldx < ndim
    assert lib.linna_hmc_comoments(None, 4, 129, p, 132, p, None) == uns
    assert "128" in lib.linna_last_error().decode()
    assert lib.linna_hmc_chol_from_comoments(None, 3, None, p, 4, p, 1, None) == bad
    assert lib.linna_hmc_chol_from_comoments(None, 3, p, None, 4, p, 1, None) == bad
    assert lib.linna_hmc_chol_from_comoments(None, 3, p, p, 4, None, 1, None) == bad
    assert lib.linna_hmc_chol_from_comoments(None, 3, p, p, 2, p, 1, None) == bad        # ldc < ndim
    assert lib.linna_hmc_chol_from_comoments(None, 129, p, p, 132, p, 1, None) == uns
    kd = lambda B, nd, Cm, ldc, G, W, Q: lib.linna_hmc_kick_drift_dense(None, B, nd, Cm, ldc, None, 0.5, 1.0, G, ldc, W, ldc, None, 0,
                                                                         Q, ldc, None)
    assert kd(4, 3, None, 4, p, p, p) == bad and kd(4, 3, p, 4, None, p, p) == bad and kd(4, 3, p, 4, p, None, p) == bad
    assert kd(4, 3, p, 4, p, p, None) == bad and kd(0, 3, p, 4, p, p, p) == bad and kd(4, 3, p, 2, p, p, p) == bad
    assert kd(4, 129, p, 132, p, p, p) == uns
    run = lambda lp, s, ws, Cm, eps: lib.linna_hmc_run_dense(lp, s, ws, Cm, 36, eps, None, None, None, None, 0, 0.65, 0, 5, 1, None,
                                                             None, None, None, None, None)
    assert run(None, C.byref(st), p, p, p) == bad and run(p, None, p, p, p) == bad and run(p, C.byref(st), None, p, p) == bad
    assert run(p, C.byref(st), p, None, p) == bad and run(None, C.byref(st), p, p, None) == bad
    fe = lambda lp, s, Cm, r0: lib.linna_hmc_find_epsilon_dense(lp, s, p, Cm, 36, r0, p, p, p, 0, 40, None)
    assert fe(None, C.byref(st), p, p) == bad and fe(p, None, p, p) == bad and fe(p, C.byref(st), None, p) == bad
    assert fe(None, C.byref(st), p, None) == bad


def test_whitening_identity():
    """A float64 transition under a random SPD mass in 7 dimensions, 5 steps: the textbook form (p ~ N(0, M), q += eps M^-1 p,
    K = p^T M^-1 p / 2) and the whitened form the kernels use agree to 1e-10 relative in every quantity."""
    nd, B, nleap = 7, 6, 5
    rs = np.random.RandomState(5)
    A = rs.standard_normal((nd, nd))
    M = A @ A.T + 0.5 * np.eye(nd)
    R = rs.standard_normal((nd, nd))
    prec = R @ R.T + np.eye(nd)
    fg = demul.gaussian_dense_fg(rs.standard_normal(nd), prec)
    x = rs.standard_normal((B, nd))
    lnp, g = fg(x)
    n01, u = rs.standard_normal((B, nd)), rs.uniform(size=B)
    eps = rs.uniform(0.05, 0.2, B)
    Cl = np.linalg.cholesky(np.linalg.inv(M))
    kw, kt = {}, {}
    a = demul.transition(fg, x, lnp, g, Cl, nleap, eps, n01, u, np.float64, kinetic=kw)
    b = demul.textbook_transition(fg, x, lnp, g, M, nleap, eps, n01, u, kinetic=kt)
    rel = lambda p, q: float(np.max(np.abs(p - q)) / max(np.max(np.abs(q)), 1e-300))
    errs = dict(x=rel(a[0], b[0]), lnp=rel(a[1], b[1]), g=rel(a[2], b[2]), dH=rel(a[5], b[5]), q=rel(kw["q"], kt["q"]),
                w=rel(kw["p"], kt["w"]), H0=rel(kw["H0"], kt["H0"]))
    print("  whitened against textbook:", errs)
    assert max(errs.values()) <= 1e-10, errs
    assert np.array_equal(a[3], b[3]) and 0 < a[3].sum() and np.max(np.abs(a[5])) > 1e-3


@pytest.mark.parametrize("B,nd", [(3, 7), (67, 33), (130, 5)])
def test_emulated_comoments_and_cholesky(B, nd):
    """Three uneven batches through the shifted sums, the slot reduction, the shrinkage and the Cholesky factor against
    np.cov and np.linalg.cholesky."""
    rs = np.random.RandomState(B + nd)
    A = rs.standard_normal((nd, nd)) * np.geomspace(1e-2, 1.0, nd)
    batches = [(off + rs.standard_normal((b, nd)) @ A.T).astype(np.float32) for off, b in ((0.3, B), (0.5, 2 * B + 1), (0.1, max(1, B // 2)))]
    mom = demul.empty_comoments(nd, batches[0][0])
    for r in batches:
        demul.merge(mom, r)
    rows = np.concatenate(batches).astype(np.float64)
    n = len(rows)
    assert mom["n"] == n
    flat = demul.pack(mom, guard=2, fill=-7.5)
    assert len(flat) == demul.comoments_doubles(nd) + 2
    back = demul.unpack(flat, nd)
    assert all(np.array_equal(back[k], np.tril(mom[k]) if k == "S2" else mom[k]) for k in ("c", "S1", "S2")) and back["n"] == n
    mean, cov = demul.covariance(mom)
    ref = np.cov(rows.T).reshape(nd, nd)
    sd = np.sqrt(np.diag(ref))
    np.testing.assert_allclose(mean, rows.mean(0), rtol=0, atol=1e-12 * (np.abs(rows).max() + 1))
    assert np.max(np.abs(cov - ref) / np.outer(sd, sd)) <= 64 * n * 2.0 ** -53 * (1 + np.max((rows.mean(0) - mom["c"]) ** 2 / sd ** 2))
    Cl, info = demul.chol_from_comoments(mom)
    want = np.linalg.cholesky(demul.shrink(ref, n))
    assert info == 0 and Cl.dtype == np.float32 and np.array_equal(Cl, np.tril(Cl))
    assert np.all(np.abs(Cl - want.astype(np.float32)) <= 4 * 2.0 ** -24 * np.sqrt(np.diag(demul.shrink(ref, n)))[:, None])
    # what cannot be factored: a NaN in S2, too few rows
    sick = demul.unpack(flat, nd)
    sick["S2"][3, nd - 1, 0] = np.nan
    assert demul.chol_from_comoments(sick)[0] is None and demul.chol_from_comoments(sick)[1] > 0
    for n_small in (1.0, 0.0, np.nan):
        sick = demul.unpack(flat, nd)
        sick["n"] = n_small
        assert demul.chol_from_comoments(sick) == (None, -1)


def test_kick_drift_restatement_is_the_matrix_product():
    """The ordered float32 triangle products against float64 matrix products."""
    rs = np.random.RandomState(2)
    B, nd = 5, 33
    Cl = np.tril(rs.standard_normal((nd, nd))).astype(np.float32)
    G, W, X = (rs.standard_normal((B, nd)).astype(np.float32) for _ in range(3))
    eps = rs.uniform(0.1, 0.3, B).astype(np.float32)
    Wn, Qn = demul.kick_drift(Cl, eps, 0.5, 1.0, G, W, X, None)
    W64 = W + 0.5 * eps[:, None] * (G.astype(np.float64) @ Cl.astype(np.float64))
    Q64 = X + eps[:, None] * (W64 @ Cl.astype(np.float64).T)
    assert Wn.dtype == Qn.dtype == np.float32
    np.testing.assert_allclose(Wn, W64, atol=nd * 2.0 ** -23 * 10)
    np.testing.assert_allclose(Qn, Q64, atol=nd * 2.0 ** -23 * 30)
    W0, Q0 = demul.kick_drift(Cl, None, 0.0, 0.0, G, W, X, None)
    assert np.array_equal(W0, W) and np.array_equal(Q0, X)


def test_keywords():
    import inspect
    torch = pytest.importorskip("torch")  # noqa: F841
    from linna_amd import sampler, util
    mode = sampler.BatchedHMC.adapt_mass_mode
    assert mode("dense") == "dense" and mode("diag") == "diag" and mode(True) == "diag" and mode(False) is False
    for bad in ("nonsense", 2, 1.0, "Dense"):
        with pytest.raises(ValueError, match="adapt_mass"):
            mode(bad)
    sig = lambda f: inspect.signature(f).parameters["adapt_mass"].default
    assert sig(sampler.BatchedHMC.adapt) is True
    assert sig(sampler.HMCSampler.sample) is False and sig(sampler.HMCSampler._hmc_chains) is False
    assert sig(util.run_mcmc) is False and sig(util.NN_samplerv1._HMC_sample) is False
    with pytest.raises(ValueError, match="adapt_mass"):
        sampler.HMCSampler(None, None, None, 3, 8).sample(None, 10, method="hmc", adapt_mass="nonsense")
    nd = 4
    A = np.random.RandomState(0).standard_normal((nd, nd))
    M = A @ A.T + np.eye(nd)
    Cl = sampler.BatchedHMC.chol_of_mass(M, nd)
    np.testing.assert_allclose(Cl @ Cl.T, np.linalg.inv(M), rtol=1e-12, atol=1e-14)
    notspd = M.copy(); notspd[0, 0] = -1.0
    asym = M.copy(); asym[0, 1] += 0.1
    for m in (notspd, asym, np.zeros((nd, nd)), np.ones((nd, nd + 1)), np.full((nd, nd), np.nan)):
        with pytest.raises(ValueError, match="dense mass"):
            sampler.BatchedHMC.chol_of_mass(m, nd)
    with pytest.raises(ValueError, match="128"):
        sampler.BatchedHMC.chol_of_mass(np.eye(129), 129)
    s = sampler.HMCSampler(None, None, None, nd, 8, m=notspd)
    with pytest.raises(ValueError, match="dense mass"):
        s._hmc_chains(None, np.zeros((8, nd)), 5, 0.1, 0, None)


def test_sidecar_is_handed_to_its_own_metric_only(tmp_path):
    pytest.importorskip("torch")
    from linna_amd import sampler

    class _Chains(object):
        ndim, B = 3, 4
    load = sampler.HMCSampler._load_adaptation
    base = dict(mass=np.ones(3, np.float32), eps=np.full(4, 0.1, np.float32), num_steps=np.int64(5), Madapt=np.int64(200))
    old, diag, dense = (str(tmp_path / n) for n in ("old.npz", "diag.npz", "dense.npz"))
    np.savez(old, **base)
    np.savez(diag, metric="diag", **base)
    np.savez(dense, metric="dense", chol=np.eye(3, dtype=np.float32) * 0.5, **base)
    assert load(old, _Chains) is not None and load(old, _Chains, "diag") is not None and load(diag, _Chains, "diag") is not None
    assert load(old, _Chains, "dense") is None and load(diag, _Chains, "dense") is None
    assert load(dense, _Chains) is None and load(dense, _Chains, "diag") is None
    kept = load(dense, _Chains, "dense")
    assert kept is not None and np.array_equal(kept["chol"], np.eye(3, dtype=np.float32) * 0.5) and kept["eps"].shape == (4,)
    np.savez(dense, metric="dense", chol=np.eye(2, dtype=np.float32), **base)          # a factor of another size
    assert load(dense, _Chains, "dense") is None
    np.savez(dense, metric="dense", **base)                                            # no factor at all
    assert load(dense, _Chains, "dense") is None


def test_emulated_dense_adaptation():
    """64 chains from the mode of the rotated target, 5 leapfrog steps, Madapt = 200, then 300 transitions, float32 on the
    kernels' Philox draws: the four conditions of the device test (tests/test_gpu_hmc_dense.py)."""
    t = demul.rotated_target()
    B, seed, Madapt, nleap, delta, nafter = 64, 9, 200, 5, 0.65, 300
    z0 = demul.mode_start(B)
    ones = np.ones(t["nd"], np.float32)
    e_d = demul.adapt_run(t["fg32"], z0, ones, seed, nleap, Madapt, delta, nafter, store=True)
    e_m = memul.adapt_run(t["fg32"], z0, ones, seed, nleap, Madapt, delta, 0)
    assert e_d["windows"] == [(75, 100), (100, 150)] and e_d["infos"] == [0, 0]
    demul.conditions("emulation, 64 chains", e_d["chol"], e_d["eps"], e_m["eps"], e_d["acc_after"] / float(nafter), e_d["chain"], t)
