"""GPU: the energy diagnostics of ``method="hmc"`` -- hmc_accept_kernel's energy group and hmc_energy_finish_kernel on crafted
inputs bit for bit against the numpy restatement (tests/hmc_energy_emul.py), linna_hmc_run_energy against the entries it
extends (the chains do not notice; one call equals the loop), divergences found where the float64 leapfrog finds them, and
the driver with its file, its resume and its gates."""
import ctypes as C
import os

import numpy as np
import pytest

import hmc_energy_emul as en
import logprob_routes
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from test_gpu_sampling import identity_emulator_logprob  # noqa: E402

f32 = np.float32
MAX_DH = 1000.0
ABOVE = np.nextafter(f32(MAX_DH), f32(np.inf))                  # 1000 + 2^-14
LAUNCHES = 7
# what row b of the crafted launches is (b % 10): (energy error H1 - H0, uniform, lnp_new override, H0 override)
ROWS = [("accepted", -1.0, 0.5, None, None), ("rejected", 1.0, 0.9, None, None), ("dH == max_dH", MAX_DH, 0.5, None, None),
        ("dH just above max_dH", ABOVE, 0.5, None, None), ("lnp_new NaN", 0.0, 0.5, np.nan, None), ("lnp_new -inf", 0.0, 0.5, -np.inf, None),
        ("lnp_new +inf", 0.0, 0.5, np.inf, None), ("H0 NaN", 0.0, 0.5, None, np.nan), ("E never changes", 1.0, 0.99, None, 2.5),
        ("accepted uphill", 0.25, 0.5, None, None)]


def _dev(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype), device="cuda")


def _padded(a, ld):
    """[B][ld] on the device, the pad columns NaN: nothing of them may be read."""
    out = np.full((a.shape[0], ld), np.nan, f32)
    out[:, :a.shape[1]] = a
    return _dev(out)


def _bits(a):
    """The bit patterns of float32 numbers, every NaN as one (its sign and payload are not part of any definition)."""
    a = np.ascontiguousarray(a, f32)
    return np.where(np.isnan(a), np.int32(0x7FC00000), a.view(np.int32))


def crafted(B, ndim, it):
    """Launch ``it`` of the crafted series: P small integers, masses powers of two, H0 and lnp_new dyadic -- the kinetic energy,
    H1 and E are exact in float32 in any summation order (checked here in float64)."""
    rs = np.random.RandomState(1000 * ndim + 10 * B + it)
    P = rs.randint(-3, 4, (B, ndim)).astype(f32)
    mass = np.array([0.5, 1.0, 2.0, 4.0], f32)[np.arange(ndim) % 4]
    half_ke = 0.5 * np.sum(P.astype(np.float64) ** 2 / mass.astype(np.float64), -1)
    H0 = (0.25 * rs.randint(-16, 17, B)).astype(f32)
    err, U = np.zeros(B, np.float64), np.zeros(B, f32)
    for b in range(B):
        _, err[b], U[b], _, h0 = ROWS[b % 10]
        if h0 is not None and np.isfinite(h0):
            H0[b] = h0
    H1 = H0.astype(np.float64) + err
    ln = half_ke - H1
    assert np.all(H1 == H1.astype(f32)) and np.all(ln == ln.astype(f32)) and np.all(half_ke == half_ke.astype(f32))
    ln = ln.astype(f32)
    for b in range(B):
        _, _, _, l, h0 = ROWS[b % 10]
        if l is not None:
            ln[b] = l
        if h0 is not None and not np.isfinite(h0):
            H0[b] = h0
    return dict(P=P, mass=mass, H0=H0, lnp_new=ln, U=U, Qn=rs.standard_normal((B, ndim)).astype(f32),
                Gn=rs.standard_normal((B, ndim)).astype(f32))


def device_inputs(t, ld):
    return {k: _padded(v, ld) if v.ndim == 2 else _dev(v) for k, v in t.items()}


@pytest.mark.parametrize("ndim", [1, 33, 65, 130])
@pytest.mark.parametrize("B", [1, 5, 64])
def test_kernel_on_crafted_inputs(B, ndim):
    """linna_hmc_accept_energy, 7 launches on one state (ld > ndim, the pad NaN): energy, dH, ndiv, X, lnp, naccept bit for bit the
    restatement's after every launch; estate, bfmi and the pooled values within rtol 1e-9 after launches 1 (n < 2: NaN), 2
    (the first D2 term is the second energy's) and 7."""
    ld = _lib.ld4(ndim) + 4
    rs = np.random.RandomState(B + ndim)
    X, G, lnp = rs.standard_normal((B, ndim)).astype(f32), rs.standard_normal((B, ndim)).astype(f32), rs.standard_normal(B).astype(f32)
    Xd, Gd, lnpd = _padded(X, ld), _padded(G, ld), _dev(lnp)
    nacc = torch.zeros(B, dtype=torch.int32, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    estate = torch.zeros((B, en.DOUBLES), dtype=torch.float64, device="cuda")
    ndiv = torch.zeros(B, dtype=torch.int32, device="cuda")
    bfmi = torch.empty(B, device="cuda")
    pooled = torch.empty(3, dtype=torch.float64, device="cuda")
    want_est, want_ndiv, want_nacc = en.empty(B), np.zeros(B, np.int64), np.zeros(B, np.int64)
    seen = set()
    for it in range(LAUNCHES):
        t = crafted(B, ndim, it)
        Ed, dHd = torch.full((B,), 7.0, device="cuda"), torch.full((B,), 7.0, device="cuda")
        d = device_inputs(t, ld)                              # (named: the tensors live until the launch has run)
        _lib.call("linna_hmc_accept_energy", _lib.ctx(), B, ndim, _lib.ptr(d["mass"]), C.c_uint64(1), _lib.iptr(step), it,
                  _lib.ptr(d["H0"]), _lib.ptr(d["P"]), ld, _lib.ptr(d["Qn"]), ld, _lib.ptr(d["lnp_new"]),
                  _lib.ptr(d["Gn"]), ld, _lib.ptr(d["U"]), _lib.ptr(Xd), ld, _lib.ptr(lnpd), _lib.ptr(Gd),
                  _lib.iptr(nacc), None, None, None, None, None, None, 0, 0.65, None, None, _lib.ptr(estate, torch.float64),
                  _lib.iptr(ndiv), MAX_DH, _lib.ptr(Ed), _lib.ptr(dHd), _lib.stream())
        _lib.call("linna_hmc_energy_finish", _lib.ctx(), B, _lib.ptr(estate, torch.float64), _lib.iptr(ndiv), _lib.ptr(bfmi),
                  _lib.ptr(pooled, torch.float64), _lib.stream())
        torch.cuda.synchronize()
        acc, E, dH, div = en.accept(t["P"], t["mass"], t["H0"], t["lnp_new"], t["U"], MAX_DH)
        for b in range(B):
            seen.add((ROWS[b % 10][0], bool(acc[b]), bool(div[b])))
        X, G, lnp = np.where(acc[:, None], t["Qn"], X), np.where(acc[:, None], t["Gn"], G), np.where(acc, t["lnp_new"], lnp)
        want_nacc += acc
        want_ndiv += div
        en.update(want_est, E)
        what = (B, ndim, it)
        np.testing.assert_array_equal(_bits(Ed.cpu().numpy()), _bits(E), err_msg=str(what))
        np.testing.assert_array_equal(_bits(dHd.cpu().numpy()), _bits(dH), err_msg=str(what))
        np.testing.assert_array_equal(ndiv.cpu().numpy(), want_ndiv, err_msg=str(what))
        np.testing.assert_array_equal(nacc.cpu().numpy(), want_nacc, err_msg=str(what))
        np.testing.assert_array_equal(_bits(Xd[:, :ndim].cpu().numpy()), _bits(X), err_msg=str(what))
        np.testing.assert_array_equal(_bits(Gd[:, :ndim].cpu().numpy()), _bits(G), err_msg=str(what))
        np.testing.assert_array_equal(_bits(lnpd.cpu().numpy()), _bits(lnp), err_msg=str(what))
        assert bool(torch.isnan(Xd[:, ndim:]).all()) and bool(torch.isnan(Gd[:, ndim:]).all())
        if it in (0, 1, LAUNCHES - 1):
            want_bfmi, want_pooled = en.finish(want_est, want_ndiv)
            np.testing.assert_allclose(estate.cpu().numpy(), want_est, rtol=1e-9, atol=0.0, err_msg=str(what))
            np.testing.assert_allclose(bfmi.cpu().numpy(), want_bfmi.astype(f32), rtol=1e-9, atol=0.0, err_msg=str(what))
            np.testing.assert_allclose(pooled.cpu().numpy(), want_pooled, rtol=1e-9, atol=0.0, err_msg=str(what))
            if it == 0:
                assert np.isnan(bfmi.cpu().numpy()).all() and np.all(want_est[:, 3] == 0.0)
    # the rows did what their names say
    rows = {ROWS[b % 10][0] for b in range(B)}
    for name, a, d in (("accepted", True, False), ("rejected", False, False), ("dH == max_dH", False, False),
                       ("dH just above max_dH", False, True), ("lnp_new NaN", False, True), ("lnp_new -inf", False, True),
                       ("lnp_new +inf", False, True), ("H0 NaN", False, True), ("E never changes", False, False),
                       ("accepted uphill", True, False)):
        if name in rows:
            assert {s for s in seen if s[0] == name} == {(name, a, d)}, (name, seen)
    got = bfmi.cpu().numpy()
    for b in range(B):
        if ROWS[b % 10][0] == "E never changes":
            assert np.isnan(got[b]) and want_est[b, 0] == LAUNCHES and want_est[b, 2] == 0.0
        if ROWS[b % 10][0] == "H0 NaN":
            assert np.all(estate[b].cpu().numpy() == 0.0) and int(ndiv[b]) == LAUNCHES        # a non-finite E changes nothing
        if ROWS[b % 10][0] == "accepted":
            assert np.isfinite(got[b])


def test_energy_and_dH_without_the_accumulators_and_the_other_way_round():
    """``energy`` and ``dH`` are each optional, and so are the accumulators as a pair: every combination writes the same values."""
    B, ndim, ld = 5, 33, 40
    t = crafted(B, ndim, 0)
    out = {}
    for what in ("all", "E", "dH", "state"):
        X, G, lnp = _padded(np.zeros((B, ndim), f32), ld), _padded(np.zeros((B, ndim), f32), ld), torch.zeros(B, device="cuda")
        nacc, step = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        estate, ndiv = torch.zeros((B, en.DOUBLES), dtype=torch.float64, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
        Ed, dHd = torch.full((B,), 7.0, device="cuda"), torch.full((B,), 7.0, device="cuda")
        st = what in ("all", "state")
        d = device_inputs(t, ld)
        _lib.call("linna_hmc_accept_energy", _lib.ctx(), B, ndim, _lib.ptr(d["mass"]), C.c_uint64(1), _lib.iptr(step), 0,
                  _lib.ptr(d["H0"]), _lib.ptr(d["P"]), ld, _lib.ptr(d["Qn"]), ld, _lib.ptr(d["lnp_new"]),
                  _lib.ptr(d["Gn"]), ld, _lib.ptr(d["U"]), _lib.ptr(X), ld, _lib.ptr(lnp), _lib.ptr(G),
                  _lib.iptr(nacc), None, None, None, None, None, None, 0, 0.65, None, None,
                  _lib.ptr(estate, torch.float64) if st else None, _lib.iptr(ndiv) if st else None, MAX_DH,
                  _lib.ptr(Ed) if what in ("all", "E") else None, _lib.ptr(dHd) if what in ("all", "dH") else None, _lib.stream())
        torch.cuda.synchronize()
        out[what] = (Ed.cpu().numpy(), dHd.cpu().numpy(), estate.cpu().numpy(), ndiv.cpu().numpy(), X.cpu().numpy(), nacc.cpu().numpy())
    full = out["all"]
    np.testing.assert_array_equal(_bits(out["E"][0]), _bits(full[0]))
    np.testing.assert_array_equal(_bits(out["dH"][1]), _bits(full[1]))
    np.testing.assert_array_equal(out["state"][2], full[2])
    np.testing.assert_array_equal(out["state"][3], full[3])
    assert np.all(out["E"][1] == 7.0) and np.all(out["dH"][0] == 7.0) and np.all(out["state"][0] == 7.0) and np.all(out["E"][2] == 0.0)
    for what in ("E", "dH", "state"):
        np.testing.assert_array_equal(_bits(out[what][4]), _bits(full[4]))
        np.testing.assert_array_equal(out[what][5], full[5])


_LP = {}


def small_mlp():
    if "mlp" not in _LP:
        _LP["mlp"] = logprob_routes.create(logprob_routes.problem("MLP", 5, 7, 41, width=64, depth=2))
    return _LP["mlp"]


def small_chains(dense, B=8):
    from linna_amd import sampler
    nd = 5
    x0 = (0.2 * np.random.RandomState(B).standard_normal((B, nd))).astype(f32)
    mass = np.linspace(0.5, 2.0, nd)
    if dense:
        A = np.random.RandomState(1).standard_normal((nd, nd))
        mass = np.diag(mass) + 0.05 * (A @ A.T)
    h = sampler.BatchedHMC(small_mlp(), x0, mass=mass.astype(np.float64 if dense else f32), seed=3)
    h.eps.fill_(0.05)
    h.mu.fill_(float(np.log(0.5)))
    return h


STATE = ("x", "lnp", "g", "naccept", "alpha", "eps", "epsbar", "Hbar", "m")


def same_bits(a, b):
    a, b = a.detach().contiguous(), b.detach().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                                                                           b.view(torch.int32) if b.dtype == torch.float32 else b))


@pytest.mark.parametrize("dense", [False, True], ids=["diag", "dense"])
def test_the_chains_do_not_notice(dense):
    """8 chains on MLP(5, 7), 6 transitions of 3 steps, Madapt = 3 (across the freeze), with the moments: linna_hmc_run_moments /
    linna_hmc_run_dense against linna_hmc_run_energy with estate == NULL (the rows alone) and with the full group -- chain,
    logps, naccept, alpha, EPS, EPSBAR (and Hbar, m, x, lnp, g) and the moments bit for bit."""
    out = []
    for mode in ("parent", "rows", "full"):
        h = small_chains(dense)
        if mode == "full":
            h.energy_stats(True, MAX_DH)
        r = h.run(6, 3, Madapt=3, moments=True, energy=mode != "parent")
        torch.cuda.synchronize()
        out.append((h, r))
    (h0, r0) = out[0]
    assert len(r0) == 2 and int(h0.naccept.sum()) > 0
    for h, r in out[1:]:
        assert len(r) == 4 and r[2].shape == r[3].shape == (6, 8)
        assert same_bits(r[0], r0[0]) and same_bits(r[1], r0[1])
        for nm in STATE:
            assert same_bits(getattr(h, nm), getattr(h0, nm)), nm
        assert torch.equal(h.comom if dense else h.mom, h0.comom if dense else h0.mom)
    # the rows are the same with and without the accumulators, and E is the energy the chain ends the transition in
    assert same_bits(out[1][1][2], out[2][1][2]) and same_bits(out[1][1][3], out[2][1][3])
    s = out[2][0].energy_summary()
    assert np.all(s["n"] == 6) and s["ndivergent_total"] == 0 and s["chains_divergent"] == 0 and s["max_dH"] == MAX_DH
    want = en.run(out[2][1][2].cpu().numpy())
    np.testing.assert_allclose(out[2][0].estate.cpu().numpy(), want, rtol=1e-9, atol=0.0)
    wb, wp = en.finish(want, np.zeros(8, np.int64))
    np.testing.assert_allclose(s["bfmi"], wb.astype(f32), rtol=1e-9)
    np.testing.assert_allclose(s["bfmi_min"], wp[0], rtol=1e-9)


@pytest.mark.parametrize("dense", [False, True], ids=["diag", "dense"])
def test_one_call_equals_the_loop(dense):
    """One linna_hmc_run_energy call of 6 transitions against 6 calls of one: energy[i], dH[i], the accumulators (Eprev carries
    across the calls) and the divergence counts bit for bit."""
    a, b = small_chains(dense), small_chains(dense)
    a.energy_stats(True, 0.125)                       # (a bound that small: some of these transitions count as divergent)
    b.energy_stats(True, 0.125)
    _, _, Ea, da = a.run(6, 3, energy=True)
    rows = [b.run(1, 3, energy=True) for _ in range(6)]
    torch.cuda.synchronize()
    assert same_bits(Ea, torch.cat([r[2] for r in rows])) and same_bits(da, torch.cat([r[3] for r in rows]))
    assert torch.equal(a.estate, b.estate) and torch.equal(a.ndiv, b.ndiv) and same_bits(a.x, b.x)
    flags = en.divergent(np.zeros((6, 8), f32), da.cpu().numpy(), 0.125)
    np.testing.assert_array_equal(a.ndiv.cpu().numpy(), flags.sum(0))
    assert 0 < flags.sum() < flags.size
    assert np.all(a.estate[:, 0].cpu().numpy() == 6) and np.array_equal(a.estate[:, 4].cpu().numpy(), Ea[-1].cpu().numpy().astype(np.float64))
    # a warm-up does not count, a reset empties
    n0 = a.estate.clone()
    a.adapt(3, adapt_mass=False)
    assert torch.equal(a.estate, n0) and a.iteration > 6
    a.energy_reset()
    assert float(a.estate.abs().sum()) == 0.0 and int(a.ndiv.sum()) == 0


def test_divergences_are_found_where_they_are():
    """The narrow Gaussian of tests/hmc_energy_emul.py (sigma_z = 0.0025), 8 chains x 10 transitions of 5 steps: at the step size
    0.001 no transition is divergent, at 0.02 (beyond the leapfrog's stability limit) every one is, as the float64 leapfrog says;
    the counts are the restatement's flags of the returned dH."""
    from linna_amd import sampler
    N = en.NARROW
    means, cov, priors, z0, _ = en.narrow_problem()
    lp = identity_emulator_logprob(N["ndim"], means, cov, priors)
    total = {}
    for key in ("eps_stable", "eps_unstable"):
        with np.errstate(invalid="ignore"):
            ref = ~(en.narrow_run(N[key]) <= N["max_dH"])
        h = sampler.BatchedHMC(lp, z0, seed=N["seed"])
        h.eps.fill_(N[key])
        h.energy_stats(True, N["max_dH"])
        chain, lnp, E, dH = h.run(N["ntrans"], N["nleap"], energy=True)
        torch.cuda.synchronize()
        d = dH.cpu().numpy()
        flags = sampler._EnergyLog.divergent(d, N["max_dH"])
        s = h.energy_summary()
        print("  eps %g: %d of %d transitions divergent (float64 leapfrog: %d), accepted %d, max finite |dH| %.4g"
              % (N[key], flags.sum(), flags.size, ref.sum(), int(h.naccept.sum()), np.max(np.abs(d[np.isfinite(d)]), initial=0.0)))
        np.testing.assert_array_equal(s["ndivergent"], flags.sum(0))
        np.testing.assert_array_equal(flags, ref)
        assert s["ndivergent_total"] == flags.sum() and s["chains_divergent"] == int((flags.sum(0) > 0).sum())
        # a divergent transition is a rejection: the chain row is the one before it
        c = np.concatenate([z0[None], chain.cpu().numpy()])
        assert np.all(c[1:][flags] == c[:-1][flags])
        assert np.isfinite(chain.cpu().numpy()).all() and np.isfinite(lnp.cpu().numpy()).all()
        np.testing.assert_allclose(h.estate.cpu().numpy(), en.run(E.cpu().numpy()), rtol=1e-9, atol=0.0)
        total[key] = flags
    assert total["eps_stable"].sum() == 0 and total["eps_unstable"].all()


def _problem8():
    rs = np.random.RandomState(0)
    nd = 8
    means, cov = rs.uniform(size=nd), np.diag(0.1 * rs.uniform(0.2, 1.0, size=nd))
    priors = [{"param": "test_%d" % i, "dist": "flat", "arg1": -5.0, "arg2": 5.0} for i in range(nd)]
    return nd, means, cov, priors


def test_through_the_driver(tmp_path, monkeypatch):
    """``HMCSampler.sample(method="hmc", energy_stats=True, criterion="rhat")``, 8 parameters, 16 chains, ncheck = 20: the
    diagnostics, chhmc_energy.npz against ``energy_summary()`` and against the restatement over the rows ``run(energy=True)``
    returned (the warm-up is not in them), resume, overwrite, the ``bfmi_min`` gate, and the chain of a run without the
    diagnostics byte for byte."""
    from linna_amd import sampler, util
    nd, means, cov, priors = _problem8()
    lp = identity_emulator_logprob(nd, means, cov, priors)
    tr = util.Transform(priors)
    nw = 16
    z0 = (util.invTransform(priors)(means)[None, :] + 0.01 * np.random.RandomState(2).standard_normal((nw, nd))).astype(f32)
    rows, summaries = [], []
    run0, save0 = sampler.BatchedHMC.run, sampler._EnergyLog.save

    def run(self, *a, **kw):
        r = run0(self, *a, **kw)
        if kw.get("energy") and self.estate is not None and not self._warm:
            rows.append((r[2].cpu().numpy(), r[3].cpu().numpy()))
        return r

    def save(self):
        summaries.append(self.ens.energy_summary())
        return save0(self)

    monkeypatch.setattr(sampler.BatchedHMC, "run", run)
    monkeypatch.setattr(sampler._EnergyLog, "save", save)
    common = dict(samp_eps=0, Madapt=30, method="hmc", ncheck=20, burnin=20)
    never = dict(criterion="rhat", ess_min=1e9)                       # (a rule that never stops: the run goes to nsamp)

    def drive(sub, nsamp, seed=5, **kw):
        out = os.path.join(str(tmp_path), sub)
        os.makedirs(out, exist_ok=True)
        s = sampler.HMCSampler(lp, None, None, nd, nw, x0=z0, transform=tr, seed=seed)
        np.random.seed(11)                                            # (the burn-in's restart draws from numpy's generator)
        s.sample(None, nsamp, outdir=out, **dict(common, **kw))
        return s, out

    s, out = drive("a", 60, energy_stats=True, **never)
    name = os.path.join(out, "chhmc_energy.npz")
    assert {"bfmi", "ndivergent", "divergent_fraction", "rhat", "ess", "n"} <= set(s.diagnostics) and s.diagnostics["n"] == 60
    assert s.diagnostics["bfmi"].shape == (nw,) and s.diagnostics["ndivergent"].shape == (nw,)
    f = dict(np.load(name))
    assert set(f) == {"bfmi", "ndivergent", "divergent_at", "n", "max_dH", "estate"}
    E, dH = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
    assert E.shape == (60, nw) and np.all(f["n"] == 60) and float(f["max_dH"]) == 1000.0          # the warm-up is not counted
    want = en.run(E)
    flags = sampler._EnergyLog.divergent(dH, 1000.0)
    np.testing.assert_allclose(f["estate"], want, rtol=1e-9, atol=0.0)
    np.testing.assert_allclose(f["bfmi"], en.finish(want, flags.sum(0))[0].astype(f32), rtol=1e-9)
    np.testing.assert_array_equal(f["ndivergent"], flags.sum(0))
    np.testing.assert_array_equal(f["divergent_at"], np.argwhere(flags))
    sm = summaries[-1]
    np.testing.assert_array_equal(f["bfmi"], sm["bfmi"])
    np.testing.assert_array_equal(f["ndivergent"], sm["ndivergent"])
    np.testing.assert_array_equal(f["n"], sm["n"])
    np.testing.assert_array_equal(s.diagnostics["bfmi"], f["bfmi"])
    assert s.diagnostics["divergent_fraction"] == flags.sum() / flags.size
    print("  60 stored transitions x %d chains: E-BFMI min %.3f median %.3f, %d divergent" % (nw, np.nanmin(f["bfmi"]), np.nanmedian(f["bfmi"]), flags.sum()))
    assert np.isfinite(f["bfmi"]).all() and np.all(f["bfmi"] > 0)
    d_a = sampler.ChainStore.load(os.path.join(out, "chhmc.h5"))
    bytes_a = open(os.path.join(out, "chhmc.h5"), "rb").read()

    # the same run without the diagnostics: the same file
    s0, out0 = drive("plain", 60, **never)
    assert not os.path.exists(os.path.join(out0, "chhmc_energy.npz")) and "bfmi" not in s0.diagnostics
    d_0 = sampler.ChainStore.load(os.path.join(out0, "chhmc.h5"))
    for k in ("chain", "chain_transformed", "log_prob", "accepted"):
        np.testing.assert_array_equal(np.asarray(d_a[k]), np.asarray(d_0[k]), err_msg=k)
    assert open(os.path.join(out0, "chhmc.h5"), "rb").read() == bytes_a

    # resume continues the accumulators and the list (a tau run: a diagnostics dict of its own)
    del rows[:]
    s2, _ = drive("a", 100, seed=6, energy_stats=True, ntimes=1e9)
    f2 = dict(np.load(name))
    assert np.all(f2["n"] == 100) and len(sampler.ChainStore.load(os.path.join(out, "chhmc.h5"))["chain"]) == 100
    assert set(s2.diagnostics) == {"n", "bfmi", "ndivergent", "divergent_fraction"}
    E2, dH2 = np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows])
    assert E2.shape == (40, nw)
    np.testing.assert_allclose(f2["estate"], en.run(E2, f["estate"].copy()), rtol=1e-9, atol=0.0)
    flags2 = sampler._EnergyLog.divergent(dH2, 1000.0)
    at2 = np.argwhere(flags2)
    at2[:, 0] += 60
    np.testing.assert_array_equal(f2["divergent_at"], np.concatenate([f["divergent_at"], at2]))
    np.testing.assert_array_equal(f2["ndivergent"], f["ndivergent"] + flags2.sum(0))

    # overwrite removes the file
    drive("a", 20, overwrite=True, **never)
    assert not os.path.exists(name)

    # a rule that is met at once stops early; a bfmi_min above every chain's value keeps the same run going to nsamp, and a
    # block that was sampled during the deciding check is not counted
    loose = dict(criterion="rhat", rhat_tol=100.0, ess_min=1e-9, energy_stats=True)
    s3, out3 = drive("loose", 100, **loose)
    n3 = len(sampler.ChainStore.load(os.path.join(out3, "chhmc.h5"))["chain"])
    f3 = dict(np.load(os.path.join(out3, "chhmc_energy.npz")))
    assert n3 < 100 and np.all(f3["n"] == n3)
    np.testing.assert_array_equal(summaries[-1]["n"], f3["n"])
    s4, out4 = drive("gated", 100, bfmi_min=1e9, **loose)
    assert len(sampler.ChainStore.load(os.path.join(out4, "chhmc.h5"))["chain"]) == 100
    s5, out5 = drive("gated_div", 100, max_divergent=0.0, max_dH=1e-6, **loose)      # (nearly every transition is "divergent" then)
    assert len(sampler.ChainStore.load(os.path.join(out5, "chhmc.h5"))["chain"]) == 100 and s5.diagnostics["divergent_fraction"] > 0.1
