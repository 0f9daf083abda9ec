"""GPU: the diagonal mass adaptation of ``method="hmc"`` -- the moments kernel against numpy's two-pass float64 moments, the
mass update against its formula, ``run(moments=True)`` against ``run()`` bit for bit, ``BatchedHMC.adapt`` against the numpy
emulation (tests/hmc_mass_emul.py) on a badly scaled Gaussian, and the keyword through the drivers with its sidecar file."""
import os

import numpy as np
import pytest

import hmc_adapt_emul as emul
import hmc_mass_emul as memul
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from test_gpu_sampling import identity_emulator_logprob  # noqa: E402
from test_gpu_hmc_adapt import chains, ND  # noqa: E402

U53 = 2.0 ** -53
GUARD = -7.5


def _moments_call(B, nd, X, ld, mom):
    _lib.call("linna_hmc_moments", _lib.ctx(), B, nd, _lib.ptr(X), ld, _lib.ptr(mom, torch.float64), _lib.stream())


def _check_moments(mom, rows, B, what):
    """mom[1 + 2 nd] (numpy) against the two-pass float64 moments of ``rows``: n exact, mean and M2 within 64 B 2^-53 relative
    (the worst-case error of a float64 sum of length B is (B - 1) 2^-53 of the sum of magnitudes; every term of M2 is
    positive, and the merge adds a handful of roundings), the mean on the scale |mean| + std."""
    rows = np.asarray(rows, np.float64)
    nd = rows.shape[1]
    mean = rows.mean(0)
    M2 = ((rows - mean) ** 2).sum(0)
    tol = 64.0 * B * U53
    em = float(np.max(np.abs(mom[1:1 + nd] - mean) / (np.abs(mean) + rows.std(0) + (len(rows) == 1))))
    e2 = float(np.max(np.abs(mom[1 + nd:1 + 2 * nd] - M2) / np.where(M2 > 0, M2, 1.0)))
    print("  %s: n %d, mean error %.3g, M2 error %.3g, bound %.3g" % (what, mom[0], em, e2, tol))
    assert mom[0] == len(rows)
    assert em <= tol and e2 <= tol, (what, em, e2, tol)


@pytest.mark.parametrize("B,nd", [(1, 1), (3, 7), (67, 33), (256, 65), (4096, 33)])
def test_moments_kernel(B, nd):
    """Three successive batches with different offsets and scales, pad columns NaN, guard doubles behind ``mom``."""
    ld = _lib.ld4(nd)
    rs = np.random.RandomState(B + nd)
    batches = [(off + sc * rs.standard_normal((B, nd)) * np.geomspace(1e-3, 1.0, nd)).astype(np.float32)
               for off, sc in ((0.3, 1.0), (-2.0, 0.05), (10.0, 3.0))]
    dev = []
    for b in batches:
        X = torch.full((B, ld), float("nan"), device="cuda")
        X[:, :nd].copy_(torch.as_tensor(b))
        dev.append(X)
    out = []
    for rep in range(2):
        mom = torch.full((1 + 2 * nd + 8,), GUARD, dtype=torch.float64, device="cuda")
        mom[:1 + 2 * nd].zero_()
        for k, X in enumerate(dev):
            _moments_call(B, nd, X, ld, mom)
            if rep == 0:
                torch.cuda.synchronize()
                _check_moments(mom.cpu().numpy(), np.concatenate(batches[:k + 1]), B, "after batch %d" % k)
        torch.cuda.synchronize()
        out.append(mom.cpu().numpy())
    assert np.all(out[0][1 + 2 * nd:] == GUARD)
    assert np.array_equal(out[0].view(np.int64), out[1].view(np.int64))          # the same bits from the same input
    # the emulation's merge, batch by batch, is the same arithmetic up to the order inside the two sums
    ref = memul.empty_moments(nd)
    for b in batches:
        memul.merge(ref, b)
    np.testing.assert_allclose(out[0][1 + nd:1 + 2 * nd], ref["M2"], rtol=64.0 * B * U53)


def test_mass_update():
    nd = 70
    rs = np.random.RandomState(4)
    n = 1234.0
    M2 = (n - 1) * np.exp(rs.uniform(np.log(1e-7), np.log(10.0), nd))
    M2[3] = 0.0                                      # all rows agree
    M2[5] = np.nan
    M2[7] = np.inf                                   # 1 / inf = 0: not positive
    M2[9] = -1.0                                     # (cannot happen; the shrunk variance is negative)
    old = np.linspace(0.5, 2.0, nd).astype(np.float32)
    host = np.concatenate([[n], rs.standard_normal(nd), M2, np.full(4, GUARD)])
    want = memul.mass_from_moments(dict(n=n, M2=M2), old)
    assert want[3] == np.float32(1.0 / (1e-3 * 5.0 / (n + 5.0))) and want[5] == old[5] and want[7] == old[7] and want[9] == old[9]
    assert np.sum(want != old) == nd - 3
    for reset in (0, 1):
        mom = torch.as_tensor(host, device="cuda")
        mass = torch.as_tensor(old, device="cuda")
        _lib.call("linna_hmc_mass_from_moments", _lib.ctx(), nd, _lib.ptr(mom, torch.float64), _lib.ptr(mass), reset, _lib.stream())
        torch.cuda.synchronize()
        got, after = mass.cpu().numpy(), mom.cpu().numpy()
        ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, ulp.max()
        assert np.array_equal(got[[5, 7, 9]], old[[5, 7, 9]])
        assert np.all(after[1 + 2 * nd:] == GUARD)
        if reset:
            assert np.all(after[:1 + 2 * nd] == 0)
        else:
            assert np.array_equal(after.view(np.int64), host.view(np.int64))
    # n = 1 (and n = 0, NaN): nothing is written
    for n_small in (1.0, 0.0, np.nan):
        host[0] = n_small
        mom = torch.as_tensor(host, device="cuda")
        mass = torch.as_tensor(old, device="cuda")
        _lib.call("linna_hmc_mass_from_moments", _lib.ctx(), nd, _lib.ptr(mom, torch.float64), _lib.ptr(mass), 0, _lib.stream())
        torch.cuda.synchronize()
        assert np.array_equal(mass.cpu().numpy(), old), n_small


@pytest.mark.parametrize("name,B,bf", [("mlp_33_33", 64, False), ("v2_33_33", 5, False), ("mlp_33_33", 70, True),
                                       ("mlp_33_33_dense", 33, False)], ids=["mlp-64", "v2-5", "mlp-70-bf16", "dense-33"])
def test_the_run_does_not_notice_the_moments(name, B, bf):
    nleap, e = 3, 2e-2
    a, b = chains(name, B, bf), chains(name, B, bf)
    a.eps.fill_(e); b.eps.fill_(e)
    ca, la = a.run(6, nleap, store=True, moments=True)
    cb, lb = b.run(6, nleap, store=True)
    torch.cuda.synchronize()
    assert b.mom is None
    assert torch.equal(ca, cb) and torch.equal(la, lb) and torch.equal(a.eps, b.eps) and torch.equal(a.naccept, b.naccept)
    assert torch.equal(a.x, b.x) and torch.equal(a.m, b.m) and a.iteration == b.iteration == 6
    assert 0 < int(a.naccept.sum())
    _check_moments(a.mom.cpu().numpy(), ca.cpu().numpy().reshape(-1, ND), B, "%s B=%d" % (name, B))


_T = {}


def target():
    """8 parameters with Gaussian priors N(0, 1) (theta = z) behind the identity-exact emulator, likelihood widths
    0.003 ... 0.3: lnP is exactly Gaussian in z with variance s^2 / (1 + s^2) about mean / (1 + s^2)."""
    if not _T:
        nd = 8
        sig = np.geomspace(0.003, 0.3, nd)
        means = np.linspace(-0.2, 0.2, nd)
        priors = [{"param": "p%d" % i, "dist": "gauss", "arg1": 0.0, "arg2": 1.0} for i in range(nd)]
        sz, mz = sig / np.sqrt(1.0 + sig ** 2), means / (1.0 + sig ** 2)
        fg64 = emul.gaussian_fg(mz, sz)
        fg32 = emul.gaussian_fg(mz.astype(np.float32), sz.astype(np.float32), np.float32)
        _T.update(nd=nd, sz=sz, mz=mz, priors=priors, fg32=fg32, fg64=fg64, means=means, cov=np.diag(sig ** 2),
                  lp=identity_emulator_logprob(nd, means, np.diag(sig ** 2), priors))
    return _T


def start(B, seed=2):
    t = target()
    return (t["mz"][None, :] + 0.01 * t["sz"].min() * np.random.RandomState(seed).standard_normal((B, t["nd"]))).astype(np.float32)


def _conditions(what, mass, eps, eps_unit, acc, chain, t):
    prod = np.asarray(mass, np.float64) * t["sz"] ** 2
    ratio = float(np.median(eps) / np.median(eps_unit))
    std = chain.reshape(-1, t["nd"]).astype(np.float64).std(0) / t["sz"]
    print("  %s: mass * var %.3f ... %.3f, step size median %.4g (unit mass %.4g, ratio %.1f), acceptance %.4f, std / truth %.3f ... %.3f"
          % (what, prod.min(), prod.max(), np.median(eps), np.median(eps_unit), ratio, acc.mean(), std.min(), std.max()))
    assert np.all((prod >= 0.8) & (prod <= 1.25)), (what, prod)
    assert ratio >= 30, (what, ratio)
    assert acc.mean() > 0.4, (what, acc.mean())
    assert np.all(np.abs(std - 1.0) <= 0.05), (what, std)


def test_adapt_against_the_emulation():
    """256 chains from the mode, 5 leapfrog steps, Madapt = 200, then 300 stored transitions.  The float32 emulation must
    satisfy every condition itself (mass * var within [0.8, 1.25], frozen step size >= 30 x the unit-mass one, acceptance > 0.4,
    std within 5 %); then the device must, with its acceptance within 4 standard errors of the emulation's."""
    from linna_amd import sampler
    t = target()
    B, nd, seed, Madapt, nleap, delta, nafter = 256, t["nd"], 9, 200, 5, 0.65, 300
    z0 = start(B)
    ones = np.ones(nd, np.float32)
    e_m = memul.adapt_run(t["fg32"], z0, ones, seed, nleap, Madapt, delta, nafter, store=True)
    e_u = memul.adapt_run(t["fg32"], z0, ones, seed, nleap, Madapt, delta, 0, adapt_mass=False)
    assert e_m["windows"] == [(75, 100), (100, 150)]
    _conditions("emulation", e_m["mass"], e_m["eps"], e_u["eps"], e_m["acc_after"] / float(nafter), e_m["chain"], t)
    h = sampler.BatchedHMC(t["lp"], z0, seed=seed)
    h.num_steps = nleap
    mass_ptr = h.mass.data_ptr()
    assert h.adapt(Madapt, delta) == [(75, 100), (100, 150)]
    assert h.iteration == Madapt + 1 and h.mass.data_ptr() == mass_ptr
    frozen = h.eps.clone()
    n0 = h.naccept.clone()
    chain, _ = h.run(nafter, store=True)
    torch.cuda.synchronize()
    assert torch.equal(h.eps, frozen) and torch.equal(h.eps, h.epsbar) and bool((h.m == 50 + 1 + nafter + 1).all())
    assert float(h.mom[0]) == 0.0                                     # (the last window's moments were consumed)
    u = sampler.BatchedHMC(t["lp"], z0, seed=seed)
    u.num_steps = nleap
    assert u.adapt(Madapt, delta, adapt_mass=False) == [] and u.iteration == Madapt + 1 and u.mom is None
    cu, _ = u.run(nafter, store=True)
    torch.cuda.synchronize()
    assert torch.equal(u.mass, torch.ones_like(u.mass))
    acc = (h.naccept - n0).cpu().numpy() / float(nafter)
    wide = cu[:, :, nd - 1].cpu().numpy().astype(np.float64).std() / t["sz"][-1]
    print("  unit mass on the device: std / truth of the widest parameter %.3f over the same %d transitions (not asserted)" % (wide, nafter))
    _conditions("device", h.mass.cpu().numpy(), h.eps.cpu().numpy(), u.eps.cpu().numpy(), acc, chain.cpu().numpy(), t)
    ref = e_m["acc_after"] / float(nafter)
    se = float(acc.std(ddof=1) / np.sqrt(B))
    print("  acceptance: device %.4f, emulation %.4f, standard error %.4f" % (acc.mean(), ref.mean(), se))
    assert abs(acc.mean() - ref.mean()) <= 4 * se, (acc.mean(), ref.mean(), se)


def test_through_the_driver(tmp_path):
    from linna_amd import sampler, util
    t = target()
    nd, nw = t["nd"], 128
    tr = util.Transform(t["priors"])
    z0 = start(nw, 3)
    out = str(tmp_path)
    side, name = os.path.join(out, "chhmc_adapt.npz"), os.path.join(out, "chhmc.h5")
    s = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, transform=tr, seed=5)
    prof = {}
    s.sample(None, 400, samp_eps=0, Madapt=200, outdir=out, method="hmc", profile=prof, adapt_mass=True)
    assert os.path.isfile(name) and os.path.isfile(side) and prof["host_adapt_s"] > 0
    d = sampler.ChainStore.load(name)
    n1 = len(d["chain"])
    assert d["chain"].shape == (n1, nw, nd) and d["chain_transformed"].shape == (n1, nw, nd) and d["log_prob"].shape == (n1, nw)
    assert 100 <= n1 <= 400 and n1 == prof["iterations"]
    th = np.asarray(d["chain_transformed"], np.float64).reshape(-1, nd)
    acc = np.asarray(d["accepted"], np.float64) / n1
    with np.load(side) as f:
        kept = {k: np.array(f[k]) for k in f.files}
    print("  %d iterations stored, acceptance %.3f, mean shift %.4f sigma, std ratio %.3f ... %.3f, mass * var %.3f ... %.3f"
          % (n1, acc.mean(), np.max(np.abs(th.mean(0) - t["mz"]) / t["sz"]), (th.std(0) / t["sz"]).min(), (th.std(0) / t["sz"]).max(),
             (kept["mass"] * t["sz"] ** 2).min(), (kept["mass"] * t["sz"] ** 2).max()))
    assert 0.4 < acc.mean() <= 1.0
    assert np.max(np.abs(th.mean(0) - t["mz"]) / t["sz"]) < 0.05
    np.testing.assert_allclose(th.std(0), t["sz"], rtol=0.08)
    assert kept["mass"].shape == (nd,) and kept["eps"].shape == (nw,) and int(kept["num_steps"]) == 5 and int(kept["Madapt"]) == 200
    assert np.array_equal(s.mass, kept["mass"].astype(np.float64)) and np.all(kept["mass"] > 10.0)
    # a second call resumes: the rows stay, the adaptation comes from the file, no adaptation time
    s2 = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, transform=tr, seed=6)
    prof2 = {}
    s2.sample(None, n1 + 100, samp_eps=0, Madapt=200, outdir=out, method="hmc", profile=prof2, adapt_mass=True)
    d2 = sampler.ChainStore.load(name)
    assert len(d2["chain"]) > n1 and np.array_equal(d2["chain"][:n1], d["chain"])
    assert np.array_equal(s2.mass, kept["mass"].astype(np.float64)) and "host_adapt_s" not in prof2
    with np.load(side) as f:
        assert np.array_equal(f["mass"], kept["mass"]) and np.array_equal(f["eps"], kept["eps"])
    # overwrite: the file is gone before the run, which adapts again
    np.savez(side, mass=np.full(nd, 123.0, np.float32), eps=np.full(nw, 0.5, np.float32), num_steps=np.int64(5), Madapt=np.int64(200))
    prof3 = {}
    s3 = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, transform=tr, seed=7)
    s3.sample(None, 100, samp_eps=0, Madapt=200, outdir=out, method="hmc", profile=prof3, adapt_mass=True, overwrite=True)
    with np.load(side) as f:
        assert np.all(f["mass"] != 123.0) and np.array_equal(s3.mass, np.asarray(f["mass"], np.float64))
    assert prof3["host_adapt_s"] > 0 and len(sampler.ChainStore.load(name)["chain"]) == 100
    # without adapt_mass: no file, the mass given
    sub = os.path.join(out, "plain"); os.makedirs(sub)
    m = np.linspace(0.5, 2.0, nd)
    s4 = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, m=m, transform=tr, seed=8)
    s4.sample(None, 100, samp_eps=0, Madapt=20, outdir=sub, method="hmc")
    assert not os.path.exists(os.path.join(sub, "chhmc_adapt.npz"))
    np.testing.assert_array_equal(s4.mass, m.astype(np.float32).astype(np.float64))
    with pytest.raises(ValueError, match="adapt_mass"):
        s4.sample(None, 100, samp_eps=0.004, outdir=sub, method="hmc", adapt_mass=True)
    # the same through run_mcmc
    sub = os.path.join(out, "run_mcmc"); os.makedirs(sub)
    nns = util.NN_samplerv1(sub, None)
    np.random.seed(3)
    util.run_mcmc(nns, sub, "hmc", nd, nw, t["mz"], t["lp"], transform=tr, max_n=100, adapt_mass=True)
    d3 = sampler.ChainStore.load(os.path.join(sub, "chhmc.h5"))
    assert d3["chain"].shape == (100, nw, nd) and np.isfinite(d3["log_prob"]).all()
    assert os.path.isfile(os.path.join(sub, "chhmc_adapt.npz"))
