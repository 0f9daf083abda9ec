"""GPU: a step size per chain through every leapfrog form, whole transitions per C call, the Metropolis + dual-averaging
launch, the bounded find_reasonable_epsilon, and ``method="hmc"`` through the drivers -- against ``BatchedHMC.step`` bit for
bit where the arithmetic is the same, against the numpy emulation (tests/hmc_adapt_emul.py) where it adapts."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import hmc_adapt_emul as emul
import poison
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from test_gpu_serving import build_logprob  # noqa: E402
from test_gpu_sampling import identity_emulator_logprob, _gaussian_33  # noqa: E402

# every program form of the gradient launch (test_leapfrog_in_the_gradient_launch_equals_the_separate_entries' cases: GRAD
# program with a partial 16-row tile, forward + dX chain with fewer rows than a workgroup, the layered fallback of a dense
# covariance, the 16-row engine) and the bf16 gradient kernel
CASES = [("mlp_33_33", 70, False), ("v2_33_33", 5, False), ("mlp_33_33_dense", 33, False), ("mlp_33_33", 2100, False),
         ("mlp_33_33", 70, True)]
IDS = ["%s-%d%s" % (n, b, "-bf16" if bf else "") for n, b, bf in CASES]
SCHEDULE = [(1, 1e-2), (5, 2e-2), (3, 5e-2), (4, 1e-2)]
STATE = ("x", "lnp", "g", "p", "q", "H0", "lnp_new", "g_new")
ND = 33
_LP = {}


def logprob(name, bf):
    if (name, bf) not in _LP:
        if bf:
            from test_gpu_bf16 import diag_problem
            from test_gpu_bf16_grad import as_bf16_grad
            _LP[name, bf] = as_bf16_grad(build_logprob(None, 2.0, diag_problem(name)[0])[0])
        else:
            _LP[name, bf] = build_logprob(name, 2.0)[0]
    return _LP[name, bf]


def chains(name, B, bf, **kw):
    from linna_amd import sampler
    x0 = (0.2 * np.random.RandomState(B).standard_normal((B, ND))).astype(np.float32)
    return sampler.BatchedHMC(logprob(name, bf), x0, mass=np.linspace(0.5, 2.0, ND).astype(np.float32), seed=3, **kw)


def assert_same_state(a, b, what, rows=None):
    for nm in STATE:
        ta, tb = getattr(a, nm), getattr(b, nm)
        ta, tb = (ta[:, :ND], tb[:, :ND]) if ta.dim() == 2 else (ta, tb)
        if rows is not None:
            ta, tb = ta[rows], tb[rows]
        assert torch.equal(ta, tb), (what, nm, float((ta - tb).abs().max()))
    na, nb = (a.naccept, b.naccept) if rows is None else (a.naccept[rows], b.naccept[rows])
    assert torch.equal(na, nb), what


@pytest.mark.parametrize("name,B,bf", CASES, ids=IDS)
def test_constant_step_size_array_equals_the_scalar(name, B, bf):
    """EPS[b] = e for every chain: the transitions of ``run`` (linna_hmc_run: start, gradient launches with the kick and the
    drift in their finish -- or behind them, dense covariance --, Metropolis launch, all on the device array) leave every
    state tensor equal to ``step`` with the scalar; 0.5f * e is exact, so the arithmetic is the same."""
    a, b = chains(name, B, bf), chains(name, B, bf)
    for it, (nleap, e) in enumerate(SCHEDULE):
        a.eps.fill_(e)
        a.run(1, nleap, store=False)
        b.step(nleap, e)
        torch.cuda.synchronize()
        assert_same_state(a, b, (it, nleap, e))
    assert 0 < int(a.naccept.sum()) <= 4 * B
    # the separate kick / drift entry with the array against the scalar one
    g = torch.randn(B, a.ld, device="cuda")
    out = []
    for eps in (None, a.eps):
        p, q = a.p.clone(), a.q.clone()
        args = (a.ctx, B, ND, _lib.ptr(a.mass))
        tail = (_lib.ptr(g), a.ld, _lib.ptr(p), a.ld, _lib.ptr(q), a.ld, _lib.stream())
        if eps is None:
            _lib.call("linna_hmc_kick_drift", *args, 0.5 * 1e-2, 1e-2, *tail)
        else:
            _lib.call("linna_hmc_kick_drift_eps", *args, _lib.ptr(eps), 0.5, 1.0, *tail)
        out.append((p, q))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("name,B,bf", CASES, ids=IDS)
def test_rows_are_independent(name, B, bf):
    """EPS[b] cycles through 7 values: row b of the run equals row b of the scalar run at EPS[b] (same start, same seed)."""
    values = [4e-3, 6e-3, 1e-2, 1.5e-2, 2e-2, 3e-2, 5e-2]
    eps = torch.tensor(values, device="cuda")[torch.arange(B, device="cuda") % 7]
    a = chains(name, B, bf)
    a.eps.copy_(eps)
    for nleap in (1, 5, 3, 4):
        a.run(1, nleap, store=False)
    for k, e in enumerate(values):
        if k >= B:
            break
        b = chains(name, B, bf)
        for nleap in (1, 5, 3, 4):
            b.step(nleap, float(np.float32(e)))
        torch.cuda.synchronize()
        rows = torch.arange(k, B, 7, device="cuda")
        assert_same_state(a, b, (k, e), rows)
    assert len(set(a.naccept.cpu().numpy().tolist())) > 1 or B < 7


@pytest.mark.parametrize("name,B,bf", CASES, ids=IDS)
def test_one_call_equals_the_loop(name, B, bf):
    """``run(6, nleap, Madapt=0)``: chain, lnp, the final state and the acceptance counts of six ``step`` calls."""
    nleap, e = 3, 2e-2
    a, b, c = chains(name, B, bf), chains(name, B, bf), chains(name, B, bf)
    a.eps.fill_(e); c.eps.fill_(e)
    chain, lnp = a.run(6, nleap, Madapt=0)
    assert c.run(6, nleap, store=False) == (None, None)
    want_c = torch.empty_like(chain); want_l = torch.empty_like(lnp)
    for i in range(6):
        b.step(nleap, e)
        want_c[i].copy_(b.x[:, :ND]); want_l[i].copy_(b.lnp)
    torch.cuda.synchronize()
    assert chain.shape == (6, B, ND) and lnp.shape == (6, B)
    assert torch.equal(chain, want_c) and torch.equal(lnp, want_l)
    assert_same_state(a, b, "store")
    assert_same_state(c, b, "no store")
    assert a.iteration == b.iteration == 6 and bool((a.m == 7).all()) and bool((a.eps == e).all())
    # and the two routes interleave on one Philox sequence
    a.step(nleap, e); a.run(2, nleap, store=False)
    for _ in range(3):
        b.step(nleap, e)
    torch.cuda.synchronize()
    assert_same_state(a, b, "interleaved")


def _pad(a, ld):
    out = torch.zeros((a.shape[0], ld), device="cuda")
    out[:, :a.shape[1]].copy_(torch.as_tensor(np.ascontiguousarray(a, np.float32)))
    return out


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32), device="cuda")


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("ndim", [7, 70])
def test_accept_adapt_acceptance_table(ndim):
    """linna_hmc_accept_adapt on tests/poison.py ``hmc_table`` (test_hmc_acceptance_table's rows and sizes): accepted exactly
    where numpy says, rejected rows untouched, alpha = exp(min(H0 - H1, 0)) -- 0 where lnp_new or an energy is not finite --
    and the chain row of every chain is its state after the test.  linna_hmc_accept on the same inputs leaves X, lnp, G and naccept
    equal to it bit for bit (ndim = 70: the second pass of the 64-lane kinetic-energy loop)."""
    t = poison.hmc_table(ndim)
    want = poison.hmc_table_expected(t)
    B, ld = 11, _lib.ld4(ndim)
    P, Qn, Gn, X, G = (_pad(t[k], ld) for k in ("P", "Qnew", "Gnew", "X", "G"))
    U, H0, lnp_new, lnp, mass = (_dev(t[k]) for k in ("U", "H0", "lnp_new", "lnp", "mass"))
    nacc = torch.zeros(B, dtype=torch.int32, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    alpha = torch.full((B,), -1.0, device="cuda")
    chain, logps = torch.full((B, ndim), 7.0, device="cuda"), torch.full((B,), 7.0, device="cuda")
    X0, G0, lnp0 = _bits(X).copy(), _bits(G).copy(), _bits(lnp).copy()
    # linna_hmc_accept on clones of the same inputs, same seed and step: the Metropolis test alone is the same test, bit for bit
    Xs, Gs, lnps, naccs = X.clone(), G.clone(), lnp.clone(), nacc.clone()
    _lib.call("linna_hmc_accept", _lib.ctx(), B, ndim, _lib.ptr(mass), C.c_uint64(1), _lib.iptr(step), _lib.ptr(H0), _lib.ptr(P), ld,
              _lib.ptr(Qn), ld, _lib.ptr(lnp_new), _lib.ptr(Gn), ld, _lib.ptr(U), _lib.ptr(Xs), ld, _lib.ptr(lnps), _lib.ptr(Gs),
              _lib.iptr(naccs), _lib.stream())
    _lib.call("linna_hmc_accept_adapt", _lib.ctx(), B, ndim, _lib.ptr(mass), C.c_uint64(1), _lib.iptr(step), 0, _lib.ptr(H0), _lib.ptr(P),
              ld, _lib.ptr(Qn), ld, _lib.ptr(lnp_new), _lib.ptr(Gn), ld, _lib.ptr(U), _lib.ptr(X), ld, _lib.ptr(lnp), _lib.ptr(G),
              _lib.iptr(nacc), _lib.ptr(alpha), None, None, None, None, None, 0, 0.65, _lib.ptr(chain), _lib.ptr(logps), _lib.stream())
    torch.cuda.synchronize()
    got = nacc.cpu().numpy().astype(bool)
    np.testing.assert_array_equal(got, want, err_msg=str(list(zip(t["what"], got, want))))
    rej = ~want
    for now, before, new in ((X, X0, Qn), (G, G0, Gn), (lnp, lnp0, lnp_new)):
        np.testing.assert_array_equal(_bits(now)[rej], before[rej])
        np.testing.assert_array_equal(_bits(now)[want], _bits(new)[want])
    np.testing.assert_array_equal(_bits(chain), _bits(X[:, :ndim]))
    np.testing.assert_array_equal(_bits(logps), _bits(lnp))
    for plain, adapt in ((Xs, X), (lnps, lnp), (Gs, G)):
        np.testing.assert_array_equal(_bits(plain), _bits(adapt))
    np.testing.assert_array_equal(naccs.cpu().numpy(), nacc.cpu().numpy())
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        ke = f(0.5) * np.sum(t["P"] * t["P"] / t["mass"][None, :], -1, dtype=f)
        H1 = ke - t["lnp_new"]
        finite = np.isfinite(t["lnp_new"]) & np.isfinite(t["H0"]) & np.isfinite(H1)
        ref = np.where(finite, np.exp(np.minimum(t["H0"] - H1, f(0))), f(0))
    al = alpha.cpu().numpy()
    print("  alpha: " + ", ".join("%s=%.4g" % (w, v) for w, v in zip(t["what"], al)))
    assert list(np.flatnonzero(~finite)) == [2, 3, 4, 5, 6, 7]
    assert np.all(al[~finite] == 0)
    # H1's sum runs in dimension order on the device as in numpy's float32 accumulation up to the order of the additions:
    # exp of a number of size <= 5 whose float32 error is a few ulp of the energies (~3)
    np.testing.assert_allclose(al[finite], ref[finite], rtol=2e-5)


def test_dual_averaging_state_follows_the_emulation():
    """Given (H0, H1) tables for m = 1 ... Madapt + 2, Madapt = 12 (across the freeze): eps, epsbar, Hbar after every step
    against the float64 emulation, within 8 x the largest relative difference of the float32 numpy recursion from the
    float64 one on the same tables (floor 1e-6)."""
    B, nd, Madapt, delta = 64, 7, 12, 0.65
    ld = _lib.ld4(nd)
    rs = np.random.RandomState(12)
    eps0 = np.exp(rs.uniform(np.log(1e-3), np.log(0.5), B)).astype(np.float32)
    st64, st32 = emul.adapt_state(eps0.astype(np.float64), np.float64), emul.adapt_state(eps0, np.float32)
    st64["mu"] = st32["mu"].astype(np.float64)                     # (one mu for all three: the recursion is what is compared)
    eps, mu = _dev(st32["eps"]), _dev(st32["mu"])
    epsbar, Hbar = torch.ones(B, device="cuda"), torch.zeros(B, device="cuda")
    m = torch.ones(B, dtype=torch.int32, device="cuda")
    mass = torch.ones(nd, device="cuda")
    zeros = torch.zeros((B, ld), device="cuda")
    X, G = zeros.clone(), zeros.clone()
    lnp, nacc = torch.zeros(B, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    alpha = torch.zeros(B, device="cuda")
    worst32, worst = 0.0, 0.0
    for it in range(Madapt + 2):
        # P = 0: H1 = -lnp_new exactly; dH = H0 - H1 in [-3, 1], a few rows not finite
        H0 = rs.uniform(-1.0, 1.0, B).astype(np.float32)
        H1 = (H0 - rs.uniform(-3.0, 1.0, B)).astype(np.float32)
        H1[it % B] = np.inf
        if it % 3 == 0:
            H0[(it + 5) % B] = np.nan
        lnp_new = (-H1).astype(np.float32)
        H0d, lnd = _dev(H0), _dev(lnp_new)
        _lib.call("linna_hmc_accept_adapt", _lib.ctx(), B, nd, _lib.ptr(mass), C.c_uint64(1), _lib.iptr(step), it, _lib.ptr(H0d),
                  _lib.ptr(zeros), ld, _lib.ptr(zeros), ld, _lib.ptr(lnd), _lib.ptr(zeros), ld, None, _lib.ptr(X), ld,
                  _lib.ptr(lnp), _lib.ptr(G), _lib.iptr(nacc), _lib.ptr(alpha), _lib.ptr(eps), _lib.ptr(epsbar), _lib.ptr(Hbar),
                  _lib.ptr(mu), _lib.iptr(m), Madapt, delta, None, None, _lib.stream())
        torch.cuda.synchronize()
        with np.errstate(invalid="ignore", over="ignore"):
            dH = H0 - (-lnp_new)
            a32 = np.where(np.isfinite(lnp_new) & np.isfinite(dH), np.exp(np.minimum(dH, np.float32(0))), np.float32(0)).astype(np.float32)
        got_alpha = alpha.cpu().numpy()
        np.testing.assert_allclose(got_alpha, a32, rtol=1e-6)
        # the recursions are fed the SAME alpha (the device's): what is compared is the recursion
        emul.dual_average(st64, got_alpha.astype(np.float64), Madapt, delta, np.float64)
        emul.dual_average(st32, got_alpha, Madapt, delta, np.float32)
        for k, t in (("eps", eps), ("epsbar", epsbar), ("Hbar", Hbar)):
            ref = st64[k]
            scale = np.maximum(np.abs(ref), 1e-3 if k == "Hbar" else 0.0)          # (Hbar crosses zero)
            worst32 = max(worst32, float(np.max(np.abs(st32[k].astype(np.float64) - ref) / scale)))
            worst = max(worst, float(np.max(np.abs(t.cpu().numpy().astype(np.float64) - ref) / scale)))
        assert np.array_equal(m.cpu().numpy(), st64["m"])
    tol = max(8 * worst32, 1e-6)
    print("  dual averaging, %d steps: device vs float64 %.3g, float32 numpy vs float64 %.3g, tolerance %.3g" % (Madapt + 2, worst, worst32, tol))
    assert worst <= tol, (worst, tol)
    assert torch.equal(eps, epsbar) and int(m[0]) == Madapt + 3


_G33 = {}


def gauss33():
    """The 33-D Gaussian of test_hmc_posterior_33d_gaussian behind the identity-exact emulator, 256 starts around the mode,
    and its log-probability / gradient in numpy (flat priors: theta = a1 + (a2 - a1) Phi(z))."""
    if not _G33:
        from linna_amd import util
        from oracle import likelihood
        ndim, means, cov, priors = _gaussian_33()
        var = np.diag(cov)
        z0 = (util.invTransform(priors)(means)[None, :] + 0.01 * np.random.RandomState(2).standard_normal((256, ndim))).astype(np.float32)

        def make(dtype):
            def fg(q):
                z = np.asarray(q, dtype)
                with np.errstate(over="ignore", invalid="ignore"):
                    d = likelihood.prior_map(z, priors) - means.astype(dtype)
                    lnp = dtype(-0.5) * np.sum(d * d / var.astype(dtype), -1) + dtype(-0.5) * np.sum(z * z, -1)
                    g = -(d / var.astype(dtype)) * likelihood.prior_map_grad(z, priors) - z
                return lnp.astype(dtype), g.astype(dtype)
            return fg
        _G33.update(ndim=ndim, means=means, cov=cov, priors=priors, z0=z0, fg32=make(np.float32), fg64=make(np.float64),
                    lp=identity_emulator_logprob(ndim, means, cov, priors))
    return _G33


def test_find_reasonable_epsilon_and_adaptation_end_to_end():
    """256 chains on the 33-D Gaussian.  The step sizes ``find_reasonable_epsilon`` leaves are the emulation's powers of two on
    >= 95 % of the chains (the cap of the HMC replay tests for fp32 decision flips; the emulation with float32 against float64
    gradients is checked to stay inside it on this input first).  After Madapt = 200 adaptive transitions and the freeze,
    the mean acceptance of the next 100 transitions is within 4 standard errors (of the device's mean, across chains) of the
    emulation's on the same Philox draws, and above 0.4.  Nothing is asserted about target_accept: the averaged step size
    of this scheme is not the one whose mean acceptance is the target."""
    from linna_amd import sampler
    g = gauss33()
    B, nd, seed, Madapt, nleap, delta = 256, g["ndim"], 9, 200, 5, 0.65
    mass = np.ones(nd, np.float32)
    e32 = emul.adaptive_run(g["fg32"], g["z0"], mass, seed, nleap, Madapt, delta, 100)
    l64, g64 = g["fg64"](g["z0"])
    eps64, rounds64, left64 = emul.find_eps(g["fg64"], g["z0"].astype(np.float64), l64, g64, mass, emul.find_eps_momenta(seed, 0, B, nd), 40, np.float64)
    same = float(np.mean(e32["eps0"] == eps64))
    print("  emulation: float32 vs float64 search agree on %.3f of the chains, rounds %d / %d, eps0 %s"
          % (same, e32["rounds"], rounds64, dict(zip(*np.unique(e32["eps0"], return_counts=True)))))
    assert same >= 0.95 and e32["nactive"] == 0 and left64 == 0 and e32["rounds"] <= 40
    h = sampler.BatchedHMC(g["lp"], g["z0"], seed=seed)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        assert h.find_reasonable_epsilon() == 0
    assert not [w for w in caught if "find_reasonable_epsilon" in str(w.message)]
    eps0 = h.eps.cpu().numpy()
    agree = float(np.mean(eps0 == e32["eps0"]))
    print("  device: step sizes equal the emulation's on %.3f of the chains" % agree)
    assert np.all(np.log2(eps0) == np.round(np.log2(eps0))) and agree >= 0.95
    np.testing.assert_allclose(h.mu.cpu().numpy(), np.log(10 * eps0), rtol=1e-5, atol=1e-6)
    h.run(Madapt + 1, nleap, store=False, Madapt=Madapt, target_accept=delta)
    frozen = h.eps.clone()
    n0 = h.naccept.clone()
    h.run(100, nleap, store=False, Madapt=Madapt, target_accept=delta)
    torch.cuda.synchronize()
    assert torch.equal(h.eps, frozen) and torch.equal(h.eps, h.epsbar) and bool((h.m == Madapt + 102).all())
    eps = h.eps.cpu().numpy()
    assert np.isfinite(eps).all() and (eps > 0).all()
    acc = (h.naccept - n0).cpu().numpy() / 100.0
    ref = e32["acc_after"] / 100.0
    se = float(acc.std(ddof=1) / np.sqrt(B))                 # the standard error of the device's mean, across chains
    print("  acceptance over 100 transitions on frozen step sizes: device %.4f, emulation %.4f, standard error %.4f; "
          "step size median device %.4g, emulation %.4g" % (acc.mean(), ref.mean(), se, np.median(eps), np.median(e32["eps"])))
    assert abs(acc.mean() - ref.mean()) <= 4 * se, (acc.mean(), ref.mean(), se)
    assert acc.mean() > 0.4


def test_chains_still_searching_after_the_last_round_are_counted_and_keep_their_step_size():
    """``find_reasonable_epsilon(max_rounds=2)`` on the same input: the search needs 6 rounds, so chains are left searching --
    the device counter says how many (the emulation's number, up to the 5 % of chains an fp32 decision may flip), a
    warning is raised, and every chain keeps the step size two rounds gave it (the emulation's on >= 95 % of the chains)."""
    from linna_amd import sampler
    g = gauss33()
    B, nd, seed = 256, g["ndim"], 9
    mass = np.ones(nd, np.float32)
    l32, g32 = g["fg32"](g["z0"])
    want, rounds, left = emul.find_eps(g["fg32"], g["z0"], l32, g32, mass, emul.find_eps_momenta(seed, 0, B, nd), 2, np.float32)
    assert rounds == 2 and left > 0
    h = sampler.BatchedHMC(g["lp"], g["z0"], seed=seed)
    with pytest.warns(UserWarning, match="find_reasonable_epsilon"):
        n = h.find_reasonable_epsilon(max_rounds=2)
    eps = h.eps.cpu().numpy()
    agree = float(np.mean(eps == want))
    print("  after 2 rounds: %d chains still searching (emulation %d), step sizes equal on %.3f of the chains: %s"
          % (n, left, agree, dict(zip(*np.unique(eps, return_counts=True)))))
    assert 0 < n <= B and abs(n - left) <= 0.05 * B and agree >= 0.95
    np.testing.assert_allclose(h.mu.cpu().numpy(), np.log(10 * eps), rtol=1e-5, atol=1e-6)


def test_posterior_through_the_driver(tmp_path):
    """``HMCSampler.sample(method="hmc", samp_eps=0, Madapt=100)``: chhmc.h5 in the emcee layout, the posterior of
    test_hmc_posterior_33d_gaussian within its thresholds (mean 0.05 sigma, std 8 %), a second call resumes from the file;
    ``run_mcmc(method="hmc")`` once with a tiny cap; a fixed ``samp_eps`` keeps the reference's semantics."""
    from linna_amd import sampler, util
    g = gauss33()
    nd, nw = g["ndim"], 256
    tr = util.Transform(g["priors"])
    out = str(tmp_path)
    s = sampler.HMCSampler(g["lp"], None, None, nd, nw, x0=g["z0"], transform=tr, seed=5)
    prof = {}
    s.sample(None, 400, samp_eps=0, Madapt=100, outdir=out, method="hmc", profile=prof)
    name = os.path.join(out, "chhmc.h5")
    assert os.path.isfile(name) and not os.path.exists(os.path.join(out, "chemcee_256.h5"))
    d = sampler.ChainStore.load(name)
    n1 = len(d["chain"])
    assert d["chain"].shape == (n1, nw, nd) and d["chain_transformed"].shape == (n1, nw, nd) and d["log_prob"].shape == (n1, nw)
    assert 100 <= n1 <= 400 and n1 == prof["iterations"]
    th = np.asarray(d["chain_transformed"], np.float64).reshape(-1, nd)
    sig = np.sqrt(np.diag(g["cov"]))
    acc = np.asarray(d["accepted"], np.float64) / n1
    print("  %d iterations stored, acceptance %.3f, mean shift %.4f sigma, std ratio %.3f ... %.3f"
          % (n1, acc.mean(), np.max(np.abs(th.mean(0) - g["means"]) / sig), (th.std(0) / sig).min(), (th.std(0) / sig).max()))
    assert 0.4 < acc.mean() <= 1.0
    assert np.max(np.abs(th.mean(0) - g["means"]) / sig) < 0.05
    np.testing.assert_allclose(th.std(0), sig, rtol=0.08)
    cut, cut_lp, _ = util.read_chain_and_cut(name, 2, method="emcee")
    assert cut.size and cut.shape[1] == nd and np.isfinite(cut).all() and np.isfinite(cut_lp).all() and np.all(np.abs(cut) < 5.0)
    # resume: the stored chain is kept and continued from its last state
    s2 = sampler.HMCSampler(g["lp"], None, None, nd, nw, x0=g["z0"], transform=tr, seed=6)
    s2.sample(None, n1 + 100, samp_eps=0, Madapt=20, outdir=out, method="hmc")
    d2 = sampler.ChainStore.load(name)
    assert len(d2["chain"]) == n1 + 100 and np.array_equal(d2["chain"][:n1], d["chain"])
    # a fixed step size: the reference's HamiltonianMove semantics, no adaptation
    s3 = sampler.HMCSampler(g["lp"], None, None, nd, nw, x0=g["z0"], transform=tr, seed=7)
    sub = os.path.join(out, "fixed"); os.makedirs(sub)
    s3.sample(None, 100, samp_steps=3, samp_eps=0.004, outdir=sub, method="hmc", overwrite=True)
    assert len(sampler.ChainStore.load(os.path.join(sub, "chhmc.h5"))["chain"]) == 100
    with pytest.raises(ValueError):
        s3.sample(None, 100, samp_eps=-0.004, outdir=sub, method="hmc", overwrite=True)
    # the same through run_mcmc
    sub = os.path.join(out, "run_mcmc"); os.makedirs(sub)
    nns = util.NN_samplerv1(sub, None)
    np.random.seed(3)
    util.run_mcmc(nns, sub, "hmc", nd, nw, g["z0"][0].astype(np.float64), g["lp"], transform=tr, max_n=100)
    d3 = sampler.ChainStore.load(os.path.join(sub, "chhmc.h5"))
    assert d3["chain"].shape == (100, nw, nd) and np.isfinite(d3["log_prob"]).all()
    assert np.all(np.abs(d3["chain_transformed"]) < 5.0)
