"""GPU: the dense mass of ``method="hmc"`` -- the co-moments kernel against numpy's two-pass float64 covariance, the Cholesky
kernel against np.linalg.cholesky, the dense kick and drift against its float32 restatement bit for bit,
``linna_hmc_run_dense`` with C = I against ``run()`` at unit mass bit for bit, ``run()`` against ``step()`` in dense mode,
one trajectory and ``BatchedHMC.adapt(adapt_mass="dense")`` against the numpy emulation (tests/hmc_dense_emul.py) on a
rotated Gaussian, and the keyword through the drivers with its sidecar file."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest

import hmc_adapt_emul as emul
import hmc_dense_emul as demul
import hmc_mass_emul as memul
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from test_gpu_sampling import identity_emulator_logprob  # noqa: E402
from test_gpu_hmc_adapt import logprob, assert_same_state, ND, SCHEDULE  # noqa: E402

U53 = 2.0 ** -53
GUARD = -7.5


def _dev(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda") if dtype is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def _padded(a, fill=float("nan")):
    """[B, nd] -> device [B, ld4(nd)] with ``fill`` in the pad columns."""
    B, nd = a.shape
    X = torch.full((B, _lib.ld4(nd)), fill, device="cuda")
    X[:, :nd].copy_(torch.as_tensor(np.asarray(a, np.float32)))
    return X


def _check_comoments(flat, rows, what):
    """The reduced mean and covariance against numpy's two-pass float64 ones: n exact, the covariance relative to
    sqrt(var_i var_j) within 64 N 2^-53 (1 + max_d (mean_d - c_d)^2 / var_d), the mean within the same on the scale of std."""
    rows = np.asarray(rows, np.float64)
    N, nd = rows.shape
    mom = demul.unpack(flat, nd)
    assert mom["n"] == N, (what, mom["n"], N)
    if N < 2:
        return
    mean = rows.mean(0)
    d = rows - mean
    ref = d.T @ d / (N - 1.0)
    sd = np.sqrt(np.diag(ref))
    factor = 1.0 + float(np.max((mean - mom["c"]) ** 2 / sd ** 2))
    tol = 64.0 * N * U53 * factor
    got_mean, got = demul.covariance(mom)
    ec = float(np.max(np.abs(got - ref) / np.outer(sd, sd)))
    em = float(np.max(np.abs(got_mean - mean) / sd))
    print("  %s: n %d, shift factor %.3g, covariance error %.3g, mean error %.3g, bound %.3g" % (what, N, factor, ec, em, tol))
    assert factor <= 1e4, (what, factor)
    assert ec <= tol and em <= tol, (what, ec, em, tol)


@pytest.mark.parametrize("B,nd", [(1, 1), (3, 7), (67, 33), (256, 65), (130, 128), (4096, 33)])
def test_comoments_kernel(B, nd):
    """Three successive batches with different offsets and scales (in units of each column's width, so that the shift stays
    within 100 widths of the mean), correlated columns, pad columns NaN, guard doubles behind ``mom``, c = row 0 of batch 0."""
    ld = _lib.ld4(nd)
    rs = np.random.RandomState(B + nd)
    width = np.geomspace(1e-2, 1.0, nd)
    mix = np.eye(nd) + rs.standard_normal((nd, nd)) / np.sqrt(nd)
    batches = [(width * (off + sc * rs.standard_normal((B, nd)) @ mix)).astype(np.float32) for off, sc in ((0.3, 1.0), (-2.0, 0.5), (10.0, 3.0))]
    dev = [_padded(b) for b in batches]
    nw = demul.comoments_doubles(nd)
    assert nw == _lib.load().linna_hmc_comoments_doubles(nd)
    out = []
    for rep in range(2):
        mom = torch.full((nw + 8,), GUARD, dtype=torch.float64, device="cuda")
        mom[:nw].zero_()
        mom[1:1 + nd].copy_(torch.as_tensor(batches[0][0].astype(np.float64)))
        for k, X in enumerate(dev):
            _lib.call("linna_hmc_comoments", _lib.ctx(), B, nd, _lib.ptr(X), ld, _lib.ptr(mom, torch.float64), _lib.stream())
            if rep == 0:
                torch.cuda.synchronize()
                _check_comoments(mom.cpu().numpy(), np.concatenate(batches[:k + 1]), "after batch %d" % k)
        torch.cuda.synchronize()
        out.append(mom.cpu().numpy())
    assert np.all(out[0][nw:] == GUARD)
    assert np.array_equal(out[0][1:1 + nd], batches[0][0].astype(np.float64))                # c is read only
    assert np.array_equal(out[0].view(np.int64), out[1].view(np.int64))                      # the same bits from the same input
    got = demul.unpack(out[0], nd)
    assert np.all(np.triu(got["S2"].reshape(-1, nd, nd), 1) == 0)                            # nothing above the diagonal is written
    ref = demul.empty_comoments(nd, batches[0][0])
    for b in batches:
        demul.merge(ref, b)
    scale = np.abs(ref["S2"]).max() + 1e-300                                                  # the emulation deals the rows alike
    assert np.max(np.abs(got["S2"] - ref["S2"])) <= 64.0 * 3 * B * U53 * scale


def _synthetic_comoments(nd, rs, n=2000.0, cond=1e6):
    """Co-moments whose covariance is Q diag(geomspace(1 / cond, 1)) Q^T exactly (up to rounding), spread over the slots."""
    Q = np.linalg.qr(rs.standard_normal((nd, nd)))[0]
    cov = (Q * np.geomspace(1.0 / cond, 1.0, nd)) @ Q.T
    cov = 0.5 * (cov + cov.T)
    S1 = n * 0.3 * np.sqrt(np.diag(cov)) * rs.standard_normal(nd)
    S2 = (n - 1.0) * cov + np.outer(S1, S1) / n
    share = rs.dirichlet(np.ones(demul.SLOTS))
    mom = demul.empty_comoments(nd, rs.standard_normal(nd))
    mom["n"] = n
    for s in range(demul.SLOTS):
        mom["S1"][s], mom["S2"][s] = share[s] * S1, np.tril(share[s] * S2)
    return mom


def _chol_call(nd, mom, Cm, info, reset):
    _lib.call("linna_hmc_chol_from_comoments", _lib.ctx(), nd, _lib.ptr(mom, torch.float64), _lib.ptr(Cm), _lib.ld4(nd), _lib.iptr(info),
              reset, _lib.stream())
    torch.cuda.synchronize()
    return mom.cpu().numpy(), Cm.cpu().numpy(), int(info.item())


@pytest.mark.parametrize("nd", [1, 7, 33, 65, 128])
def test_cholesky_kernel(nd):
    ld = _lib.ld4(nd)
    rs = np.random.RandomState(nd)
    mom0 = _synthetic_comoments(nd, rs)
    host = demul.pack(mom0, guard=4, fill=GUARD)
    nw = demul.comoments_doubles(nd)
    mean, cov = demul.covariance(demul.unpack(host, nd))
    A = demul.shrink(cov, mom0["n"])
    assert np.linalg.cond(A) <= 1e6 * 1.01
    want = np.linalg.cholesky(A)
    old = np.full((2, nd, ld), 3.25, np.float32)
    for reset in (0, 1):
        after, Cm, info = _chol_call(nd, _dev(host), _dev(old), torch.full((1,), 99, dtype=torch.int32, device="cuda"), reset)
        assert info == 0
        err = np.abs(Cm[0, :, :nd].astype(np.float64) - want.astype(np.float32))
        bound = 4 * 2.0 ** -24 * np.sqrt(np.diag(A))[:, None]
        print("  nd %d reset %d: largest |C - chol| / (2^-24 sqrt(cov_ii)) = %.3f (bound 4)" % (nd, reset, float(np.max(err / bound)) * 4))
        assert np.all(err <= bound)
        assert np.array_equal(Cm[1, :, :nd], Cm[0, :, :nd].T)                           # the transpose block, exactly
        assert np.all(np.triu(Cm[0, :, :nd], 1) == 0) and np.all(Cm[:, :, nd:] == 0) and np.all(np.diag(Cm[0, :, :nd]) > 0)
        assert np.all(after[nw:] == GUARD)
        if reset:
            assert after[0] == 0 and np.all(after[1 + nd:nw] == 0)
            np.testing.assert_allclose(after[1:1 + nd], mean, rtol=0, atol=1e-13)
        else:
            assert np.array_equal(after.view(np.int64), host.view(np.int64))
    # the emulation is the same arithmetic
    np.testing.assert_allclose(demul.chol_from_comoments(mom0)[0], Cm[0, :, :nd], rtol=0, atol=float(bound.max()))
    if nd < 2:
        return
    # a NaN in S2: info > 0 and the factor stays; the shift and the zeroing follow all the same
    sick = demul.unpack(host, nd)
    sick["S2"][2, nd - 1, 0] = np.nan
    after, Cm, info = _chol_call(nd, _dev(demul.pack(sick, 4, GUARD)), _dev(old), torch.zeros(1, dtype=torch.int32, device="cuda"), 1)
    assert 0 < info <= nd and np.array_equal(Cm, old) and after[0] == 0 and np.all(after[1 + nd:nw] == 0) and np.all(after[nw:] == GUARD)
    np.testing.assert_allclose(after[1:1 + nd], mean, rtol=0, atol=1e-13)
    neg = demul.unpack(host, nd)
    neg["S2"][:, 1, 1] = -1.0                                                        # a negative variance: pivot 1
    _, Cm, info = _chol_call(nd, _dev(demul.pack(neg, 4, GUARD)), _dev(old), torch.zeros(1, dtype=torch.int32, device="cuda"), 0)
    assert info == 2 and np.array_equal(Cm, old)
    for n_small in (1.0, 0.0, np.nan):
        few = host.copy()
        few[0] = n_small
        after, Cm, info = _chol_call(nd, _dev(few), _dev(old), torch.zeros(1, dtype=torch.int32, device="cuda"), 0)
        assert info == -1 and np.array_equal(Cm, old) and np.array_equal(after.view(np.int64), few.view(np.int64))


def _factor(nd, rs):
    """A lower-triangular factor with a positive diagonal and entries of every sign, as the device pair [2][nd][ld]."""
    Cl = np.tril(rs.standard_normal((nd, nd)) / np.sqrt(nd)).astype(np.float32)
    Cl[np.arange(nd), np.arange(nd)] = np.abs(Cl[np.arange(nd), np.arange(nd)]) + 0.5
    pair = np.zeros((2, nd, _lib.ld4(nd)), np.float32)
    pair[0, :, :nd], pair[1, :, :nd] = Cl, Cl.T
    return Cl, _dev(pair)


@pytest.mark.parametrize("nd", [1, 7, 33, 65, 128])
@pytest.mark.parametrize("B", [1, 5, 67])
def test_kick_drift_kernel(B, nd):
    """Kick only, drift only and both; X given and in place; EPS per chain and null: bit for bit the float32 restatement
    (triangle only, j ascending, product then add, the scale first), pad columns untouched."""
    ld = _lib.ld4(nd)
    rs = np.random.RandomState(100 * B + nd)
    Cl, Cm = _factor(nd, rs)
    G, W, X, Q = (rs.standard_normal((B, nd)).astype(np.float32) for _ in range(4))
    eps = rs.uniform(0.05, 0.5, B).astype(np.float32)
    Gd, Xd, ed = _padded(G), _padded(X), _dev(eps)
    PADW, PADQ = 11.5, -13.25
    for mk, md in ((0.5, 1.0), (1.0, 0.0), (0.0, 1.0), (1.0, 1.0)):
        for with_x in (True, False):
            for with_eps in (True, False):
                Wd, Qd = _padded(W, PADW), _padded(Q, PADQ)
                scale = 1.0 if with_eps else 0.25                        # (a scalar step size rides in the multipliers)
                _lib.call("linna_hmc_kick_drift_dense", _lib.ctx(), B, nd, _lib.ptr(Cm), ld, _lib.ptr(ed) if with_eps else None,
                          mk * scale, md * scale, _lib.ptr(Gd), ld, _lib.ptr(Wd), ld, _lib.ptr(Xd) if with_x else None, ld,
                          _lib.ptr(Qd), ld, _lib.stream())
                torch.cuda.synchronize()
                Ww, Qw = demul.kick_drift(Cl, eps if with_eps else None, mk * scale, md * scale, G, W, X if with_x else None, Q)
                gw, gq = Wd.cpu().numpy(), Qd.cpu().numpy()
                what = (mk, md, with_x, with_eps)
                assert np.array_equal(gw[:, :nd].view(np.int32), Ww.view(np.int32)), (what, np.abs(gw[:, :nd] - Ww).max())
                assert np.array_equal(gq[:, :nd].view(np.int32), Qw.view(np.int32)), (what, np.abs(gq[:, :nd] - Qw).max())
                assert np.all(gw[:, nd:] == PADW) and np.all(gq[:, nd:] == PADQ)
                if mk == 0.0:
                    assert np.array_equal(gw[:, :nd], W)
                if md == 0.0:
                    assert np.array_equal(gq[:, :nd], X if with_x else Q)


def _unit_chains(name, B, bf, dense):
    from linna_amd import sampler
    x0 = (0.2 * np.random.RandomState(B).standard_normal((B, ND))).astype(np.float32)
    return sampler.BatchedHMC(logprob(name, bf), x0, mass=np.eye(ND) if dense else None, seed=3)


@pytest.mark.parametrize("name,B,bf", [("mlp_33_33", 64, False), ("v2_33_33", 5, False), ("mlp_33_33", 70, True),
                                       ("mlp_33_33_dense", 33, False)], ids=["mlp-64", "v2-5", "mlp-70-bf16", "dense-33"])
def test_run_dense_with_the_identity_equals_run_at_unit_mass(name, B, bf):
    """C = I: the dense launches add exact zeros, so the step-size search, the chain, lnP and the dual-averaging state of
    ``linna_hmc_run_dense`` are ``linna_hmc_run``'s at unit mass bit for bit (Madapt > 0: across the freeze)."""
    a, b = _unit_chains(name, B, bf, True), _unit_chains(name, B, bf, False)
    assert a.chol is not None and b.chol is None and torch.equal(a.mass, b.mass)
    assert torch.equal(a.chol[0, :, :ND], torch.eye(ND, device="cuda")) and torch.equal(a.chol[0], a.chol[1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert a.find_reasonable_epsilon(12) == b.find_reasonable_epsilon(12)
    assert torch.equal(a.eps, b.eps) and torch.equal(a.mu, b.mu)
    ca, la = a.run(7, 3, store=True, Madapt=4)
    cb, lb = b.run(7, 3, store=True, Madapt=4)
    torch.cuda.synchronize()
    assert torch.equal(ca, cb) and torch.equal(la, lb)
    for k in ("eps", "epsbar", "Hbar", "naccept", "m", "alpha"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.x, b.x) and torch.equal(a.lnp, b.lnp) and a.iteration == b.iteration == 7
    assert torch.equal(a.eps, a.epsbar) and 0 < int(a.naccept.sum()) and bool(torch.isfinite(ca).all())


def _dense_chains(name, B, bf):
    from linna_amd import sampler
    rs = np.random.RandomState(7)
    A = rs.standard_normal((ND, ND)) / np.sqrt(ND)
    cov = A @ A.T + 0.3 * np.eye(ND)
    x0 = (0.2 * np.random.RandomState(B).standard_normal((B, ND))).astype(np.float32)
    return sampler.BatchedHMC(logprob(name, bf), x0, mass=np.linalg.inv(cov), seed=3), cov


@pytest.mark.parametrize("name,B,bf", [("mlp_33_33", 70, False), ("v2_33_33", 5, False), ("mlp_33_33_dense", 33, False),
                                       ("mlp_33_33", 70, True)], ids=["mlp-70", "v2-5", "dense-33", "mlp-70-bf16"])
def test_run_equals_step_in_dense_mode(name, B, bf):
    """A non-trivial factor: ``run`` leaves every state tensor equal to the dense ``step`` loop through the public entries;
    ``run(moments=True)`` is ``run()`` bit for bit and its co-moments are those of the stored chain."""
    (a, cov), (b, _) = _dense_chains(name, B, bf), _dense_chains(name, B, bf)
    Cl = a.chol[0, :, :ND].cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(Cl @ Cl.T, cov, rtol=1e-5, atol=1e-6)
    assert torch.equal(a.mass, torch.ones_like(a.mass)) and torch.equal(a.chol[1, :, :ND], a.chol[0, :, :ND].T)
    for it, (nleap, e) in enumerate(SCHEDULE):
        a.eps.fill_(e)
        a.run(1, nleap, store=False)
        b.step(nleap, e)
        torch.cuda.synchronize()
        assert_same_state(a, b, (it, nleap, e))
    assert 0 < int(a.naccept.sum()) <= 4 * B
    a.eps.fill_(2e-2); b.eps.fill_(2e-2)
    ca, la = a.run(6, 3, store=True, moments=True)
    cb, lb = b.run(6, 3, store=True)
    torch.cuda.synchronize()
    assert b.comom is None and a.mom is None
    assert torch.equal(ca, cb) and torch.equal(la, lb) and torch.equal(a.naccept, b.naccept) and torch.equal(a.x, b.x)
    _check_comoments(a.comom.cpu().numpy(), ca.cpu().numpy().reshape(-1, ND), "%s B=%d" % (name, B))


_T = {}


def target():
    """tests/hmc_dense_emul.py's rotated target behind the identity-exact emulator: lnP is exactly Gaussian in z."""
    if not _T:
        t = demul.rotated_target()
        _T.update(t, lp=identity_emulator_logprob(t["nd"], t["means"], t["like"], t["priors"]))
    return _T


def test_one_trajectory_against_the_emulation():
    """64 chains drawn from the posterior, a factor that is not the posterior's own, 3 leapfrog steps with a step size per
    chain: the device against the float64 textbook emulation on the same draws, within 8 x the largest relative difference
    of the float32 emulation from the float64 one (the rule of test_dual_averaging_state_follows_the_emulation).  The float32
    emulation evaluates the density the way the device does (priors plus the likelihood about its own mean, which differs
    from the posterior form by a constant).  Measured: see DESIGN section 3.10."""
    from linna_amd import sampler
    t = target()
    B, nd, nleap, seed = 64, t["nd"], 3, 4
    rs = np.random.RandomState(6)
    L = np.linalg.cholesky(t["cov"])
    z0 = (t["mz"] + rs.standard_normal((B, nd)) @ L.T).astype(np.float32)
    S = rs.standard_normal((nd, nd))
    K = np.eye(nd) + 0.15 * (S + S.T) / np.sqrt(2 * nd)        # (off by 15 % or so in the whitened coordinates)
    M = np.linalg.inv(L @ K @ K.T @ L.T)
    M = 0.5 * (M + M.T)
    h = sampler.BatchedHMC(t["lp"], z0, mass=M, seed=seed)
    Cl32 = h.chol[0, :, :nd].cpu().numpy()
    M32 = np.linalg.inv(Cl32.astype(np.float64) @ Cl32.astype(np.float64).T)      # the mass the device runs under
    eps = rs.uniform(0.3, 0.6, B).astype(np.float32)
    h.eps.copy_(_dev(eps))
    h.run(1, nleap, store=False)
    torch.cuda.synchronize()
    n01, u = emul.momenta(seed, 0, B, nd), emul.uniforms(seed, 0, B)
    l64, g64 = t["fg64"](z0.astype(np.float64))
    k64, k32 = {}, {}
    r64 = demul.textbook_transition(t["fg64"], z0, l64, g64, M32, nleap, eps, n01, u, kinetic=k64)
    l32, g32 = t["fg32_device"](z0)
    demul.transition(t["fg32_device"], z0, l32, g32, Cl32, nleap, eps, n01, u, np.float32, kinetic=k32)
    c = t["const"]                                                                 # lnP as the device forms it - the posterior form
    got = dict(q=h.q[:, :nd].cpu().numpy(), w=h.p[:, :nd].cpu().numpy(), lnp_new=h.lnp_new.cpu().numpy() - c, H0=h.H0.cpu().numpy() + c)
    ref = dict(q=k64["q"], w=k64["w"], lnp_new=k64["lnp_new"], H0=k64["H0"])
    e32 = dict(q=k32["q"], w=k32["p"], lnp_new=k32["lnp_new"] - c, H0=k32["H0"] + c)
    rel = lambda a, r: float(np.max(np.abs(np.asarray(a, np.float64) - r)) / np.max(np.abs(r)))
    worst32 = max(rel(e32[k], ref[k]) for k in ref)
    worst = {k: rel(got[k], ref[k]) for k in ref}
    tol = 8 * worst32
    print("  one trajectory: float32 emulation against float64 %.3g (tolerance %.3g); device against float64 %s" % (worst32, tol, worst))
    assert np.max(np.abs(r64[5])) > 1e-3 and 0 < r64[3].sum()                      # (energy errors worth the name; some accepted)
    assert max(worst.values()) <= tol, (worst, tol)
    sure = np.abs(u - r64[4]) > 1e-3                                               # (the test is not at its edge)
    assert np.array_equal((h.naccept.cpu().numpy() > 0)[sure], r64[3][sure])


def test_adapt_against_the_emulation():
    """256 chains from the mode, BatchedHMC(seed=9), 5 leapfrog steps, Madapt = 200, then 300 stored transitions.  The float32
    emulation must satisfy every condition itself (eigenvalues of C^-1 cov C^-T within [0.8, 1.25], frozen step size >= 10 x
    the diagonal adaptation's, acceptance > 0.4, std along the principal axes within 5 %); then the device must, with its
    acceptance within 4 standard errors of the emulation's."""
    from linna_amd import sampler
    t = target()
    B, nd, seed, Madapt, nleap, delta, nafter = 256, t["nd"], 9, 200, 5, 0.65, 300
    z0 = demul.mode_start(B)
    ones = np.ones(nd, np.float32)
    e_d = demul.adapt_run(t["fg32"], z0, ones, seed, nleap, Madapt, delta, nafter, store=True)
    e_m = memul.adapt_run(t["fg32"], z0, ones, seed, nleap, Madapt, delta, 0)
    assert e_d["windows"] == [(75, 100), (100, 150)] and e_d["infos"] == [0, 0]
    demul.conditions("emulation", e_d["chol"], e_d["eps"], e_m["eps"], e_d["acc_after"] / float(nafter), e_d["chain"], t)
    h = sampler.BatchedHMC(t["lp"], z0, seed=seed)
    h.num_steps = nleap
    mass_ptr = h.mass.data_ptr()
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message="adapt:")                 # (no window fails to factor)
        assert h.adapt(Madapt, delta, "dense") == [(75, 100), (100, 150)]
    assert h.iteration == Madapt + 1 and h.mass.data_ptr() == mass_ptr and torch.equal(h.mass, torch.ones_like(h.mass))
    frozen = h.eps.clone()
    n0 = h.naccept.clone()
    chain, _ = h.run(nafter, store=True)
    torch.cuda.synchronize()
    assert torch.equal(h.eps, frozen) and torch.equal(h.eps, h.epsbar) and bool((h.m == 50 + 1 + nafter + 1).all())
    assert float(h.comom[0]) == 0.0 and h.mom is None and h._info == 0      # (the last window's co-moments were consumed)
    d = sampler.BatchedHMC(t["lp"], z0, seed=seed)
    d.num_steps = nleap
    assert d.adapt(Madapt, delta, adapt_mass=True) == [(75, 100), (100, 150)] and d.chol is None
    torch.cuda.synchronize()
    acc = (h.naccept - n0).cpu().numpy() / float(nafter)
    demul.conditions("device", h.chol[0, :, :nd].cpu().numpy(), h.eps.cpu().numpy(), d.eps.cpu().numpy(), acc, chain.cpu().numpy(), t)
    ref = e_d["acc_after"] / float(nafter)
    se = float(acc.std(ddof=1) / np.sqrt(B))
    print("  acceptance: device %.4f, emulation %.4f, standard error %.4f" % (acc.mean(), ref.mean(), se))
    assert abs(acc.mean() - ref.mean()) <= 4 * se, (acc.mean(), ref.mean(), se)
    with pytest.raises(ValueError, match="adapt_mass"):
        h.adapt(20, delta, "nonsense")
    with pytest.raises(ValueError, match="dense"):
        h.adapt(20, delta, True)                                           # (a diagonal adaptation of an object in dense mode)
    with pytest.raises(ValueError, match="dense mass"):
        sampler.BatchedHMC(t["lp"], z0, mass=-np.eye(nd))


def _principal(th, t):
    proj = (np.asarray(th, np.float64).reshape(-1, t["nd"]) - t["mz"]) @ t["axes"]
    return np.abs(proj.mean(0)) / t["widths"], proj.std(0) / t["widths"]


def test_through_the_driver(tmp_path):
    from linna_amd import sampler, util
    t = target()
    nd, nw = t["nd"], 128
    tr = util.Transform(t["priors"])
    z0 = demul.mode_start(nw, 3)
    out = str(tmp_path)
    side, name = os.path.join(out, "chhmc_adapt.npz"), os.path.join(out, "chhmc.h5")
    s = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, transform=tr, seed=5)
    prof = {}
    s.sample(None, 400, samp_eps=0, Madapt=200, outdir=out, method="hmc", profile=prof, adapt_mass="dense")
    assert os.path.isfile(name) and os.path.isfile(side) and prof["host_adapt_s"] > 0
    d = sampler.ChainStore.load(name)
    n1 = len(d["chain"])
    assert d["chain"].shape == (n1, nw, nd) and 100 <= n1 <= 400 and n1 == prof["iterations"]
    shift, std = _principal(d["chain_transformed"], t)
    acc = np.asarray(d["accepted"], np.float64) / n1
    with np.load(side) as f:
        kept = {k: np.array(f[k]) for k in f.files}
    print("  %d iterations stored, acceptance %.3f, mean shift %.4f sigma, std ratio %.3f ... %.3f along the principal axes, "
          "step size median %.3g" % (n1, acc.mean(), shift.max(), std.min(), std.max(), np.median(kept["eps"])))
    assert 0.4 < acc.mean() <= 1.0
    assert shift.max() < 0.05
    np.testing.assert_allclose(std, 1.0, rtol=0.08)
    assert str(kept["metric"]) == "dense" and kept["chol"].shape == (nd, nd) and kept["eps"].shape == (nw,)
    assert kept["mass"].shape == (nd,) and int(kept["num_steps"]) == 5 and int(kept["Madapt"]) == 200
    C64 = kept["chol"].astype(np.float64)
    assert np.array_equal(s.cov, C64 @ C64.T) and np.array_equal(s.mass, 1.0 / np.diag(s.cov))
    assert np.median(kept["eps"]) > 0.3                       # (a diagonal mass leaves 0.06 on this target)
    # a second call resumes: the rows stay, the adaptation comes from the file, no adaptation time
    s2 = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, transform=tr, seed=6)
    prof2 = {}
    s2.sample(None, n1 + 100, samp_eps=0, Madapt=200, outdir=out, method="hmc", profile=prof2, adapt_mass="dense")
    d2 = sampler.ChainStore.load(name)
    n2 = len(d2["chain"])
    assert n2 > n1 and np.array_equal(d2["chain"][:n1], d["chain"])
    assert np.array_equal(s2.cov, s.cov) and "host_adapt_s" not in prof2
    with np.load(side) as f:
        assert np.array_equal(f["chol"], kept["chol"]) and np.array_equal(f["eps"], kept["eps"])
    # a resumed run of the other metric does not take the file: it adapts again and rewrites it
    s3 = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, transform=tr, seed=7)
    prof3 = {}
    s3.sample(None, n2 + 50, samp_eps=0, Madapt=200, outdir=out, method="hmc", profile=prof3, adapt_mass=True)
    assert prof3["host_adapt_s"] > 0 and s3.cov is None
    with np.load(side) as f:
        assert "metric" not in f.files and "chol" not in f.files and np.array_equal(s3.mass, np.asarray(f["mass"], np.float64))
    # overwrite: the file is gone before the run, which adapts again
    np.savez(side, metric="dense", chol=np.eye(nd, dtype=np.float32) * 123.0, mass=np.ones(nd, np.float32),
             eps=np.full(nw, 0.5, np.float32), num_steps=np.int64(5), Madapt=np.int64(200))
    prof4 = {}
    s4 = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, transform=tr, seed=8)
    s4.sample(None, 100, samp_eps=0, Madapt=200, outdir=out, method="hmc", profile=prof4, adapt_mass="dense", overwrite=True)
    with np.load(side) as f:
        assert np.all(np.diag(f["chol"]) < 1.0) and str(f["metric"]) == "dense"
    assert prof4["host_adapt_s"] > 0 and len(sampler.ChainStore.load(name)["chain"]) == 100
    # a 2-D m with a fixed step size: no adaptation, no file, its rows stored
    sub = os.path.join(out, "fixed"); os.makedirs(sub)
    s5 = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, m=np.linalg.inv(s.cov), transform=tr, seed=9)
    s5.sample(None, 100, samp_eps=0.5, outdir=sub, method="hmc")
    d5 = sampler.ChainStore.load(os.path.join(sub, "chhmc.h5"))
    assert d5["chain"].shape == (100, nw, nd) and np.isfinite(d5["log_prob"]).all() and not os.path.exists(os.path.join(sub, "chhmc_adapt.npz"))
    np.testing.assert_allclose(s5.cov, s.cov, rtol=1e-4, atol=1e-9)
    assert 0.4 < np.asarray(d5["accepted"], np.float64).mean() / 100 <= 1.0
    with pytest.raises(ValueError, match="adapt_mass"):
        s5.sample(None, 100, samp_eps=0.5, outdir=sub, method="hmc", adapt_mass="dense")
    # the same through run_mcmc
    sub = os.path.join(out, "run_mcmc"); os.makedirs(sub)
    nns = util.NN_samplerv1(sub, None)
    np.random.seed(3)
    util.run_mcmc(nns, sub, "hmc", nd, nw, t["mz"], t["lp"], transform=tr, max_n=400, adapt_mass="dense")
    d6 = sampler.ChainStore.load(os.path.join(sub, "chhmc.h5"))
    shift, std = _principal(d6["chain_transformed"], t)
    acc = np.asarray(d6["accepted"], np.float64) / len(d6["chain"])
    print("  run_mcmc: %d iterations, acceptance %.3f, mean shift %.4f sigma, std ratio %.3f ... %.3f"
          % (len(d6["chain"]), acc.mean(), shift.max(), std.min(), std.max()))
    assert 0.4 < acc.mean() <= 1.0 and shift.max() < 0.05
    np.testing.assert_allclose(std, 1.0, rtol=0.08)
    with np.load(os.path.join(sub, "chhmc_adapt.npz")) as f:
        assert str(f["metric"]) == "dense" and f["chol"].shape == (nd, nd)
