"""GPU: split-R-hat from block moments and the multi-chain ESS from the running sums (csrc/autocorr.hip through
``DeviceChain``) against the plain-loop restatement of the definitions (tests/rhat_emul.py), and ``criterion="rhat"`` through
the driver.

Tolerance: the device and the restatement add the same float64 terms in another order (per-lane sums of x - x_0 and their
squares, in pieces; lagged products with the mean taken out through prefix sums), so ``rtol=1e-9`` -- the bar of
tests/test_gpu_autocorr.py for this file's statistics.  Truncation indices are discrete and must agree exactly."""
import contextlib
import io
import os

import numpy as np
import pytest

import rhat_emul as emul
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_autocorr import ar1  # noqa: E402

RHO = np.array([0.5, 0.9, 0.97])
WINDOWS = [(0, 1200), (90, 450), (90, 451), (5, 1199), (1100, 1200), (1150, 1177), (100, 500), (128, 384), (0, 256), (127, 1025)]


def _chain(nw, nt=1200):
    """The AR(1) chains of test_gpu_autocorr: a large common offset with a small scale, float32 as the device stores them."""
    return ar1(nt, nw, RHO, seed=nw, mean=np.array([0.0, 30.0, -7.0]), scale=np.array([1.0, 1e-2, 3.0]))


def _rel(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.abs(np.asarray(a) / np.asarray(b) - 1.0)))


def _assert_rhat(dc, ref, **kw):
    """``dc.rhat(**kw)`` with the records and from the stored chain alone: both equal the restatement (R-hat, W, var+ to 1e-9
    relative, the grand mean to 1e-9 of the parameter's scale), and a second call of either gives the same bits."""
    worst = 0.0
    for records in (True, False):
        dc.rhat(records=records, **kw)
        got = dc.last_rhat.copy()
        dc.rhat(records=records, **kw)
        assert np.array_equal(got, dc.last_rhat, equal_nan=True), (records, kw)
        np.testing.assert_allclose(got[:, :3], ref[:, :3], rtol=1e-9, err_msg=str((records, kw)))
        np.testing.assert_allclose(got[:, 3], ref[:, 3], rtol=1e-9, atol=1e-9 * float(np.sqrt(ref[:, 2].max())))
        worst = max(worst, _rel(got[:, :3], ref[:, :3]))
    return worst


@pytest.mark.parametrize("nw", [24, 64, 100, 130])
def test_rhat_matches_the_restatement_on_ar1_chains(nw):
    """1200 rows appended in blocks of 100 as the driver does, R-hat at the checks 100, 200, 600, 1200 (windows shorter than
    one record, then records plus ragged ends); then windows with odd N, a start that is no multiple of the record size, a
    window shorter than a record, windows holding exactly one complete record, an earlier ``upto`` and a ``discard``.
    Measured on MI355X: largest relative difference of R-hat, W, var+ over all cases and both routes 2.0e-14."""
    from linna_amd import sampler
    x = _chain(nw)
    xf = x.astype(np.float64)
    dc = sampler.DeviceChain()
    worst = 0.0
    for n0 in range(0, 1200, 100):
        dc.append(torch.as_tensor(x[n0:n0 + 100], device="cuda"))
        if n0 + 100 in (100, 200, 600, 1200):
            worst = max(worst, _assert_rhat(dc, emul.split_rhat(xf[:n0 + 100])))
            assert dc._mb == (n0 + 100) // _lib.RHAT_BLOCK
    for lo, hi in WINDOWS:
        worst = max(worst, _assert_rhat(dc, emul.split_rhat(xf[lo:hi]), discard=lo, upto=hi))
    print("  nw %d: largest relative difference %.3g" % (nw, worst))
    assert np.all(np.abs(dc.rhat() - 1.0) < 0.2)
    with pytest.raises(_lib.LinnaHipError):
        dc.rhat(discard=10, upto=13)                           # n = 1


def test_subset_rhat_on_all_walkers_ess_on_the_subset_lanes():
    """2100 walkers: the running sums cover every third walker (700 lanes), R-hat all 2100."""
    from linna_amd import sampler
    x = ar1(300, 2100, [0.5, 0.8], seed=7, mean=np.array([1.0, -2.0]))
    xf = x.astype(np.float64)
    dc = sampler.DeviceChain()
    dc.append(torch.as_tensor(x[:200], device="cuda"))
    dc.append(torch.as_tensor(x[200:], device="cuda"))
    assert dc.subset and dc.wstride == 3 and dc.nws == 700
    _assert_rhat(dc, emul.split_rhat(xf))
    _assert_rhat(dc, emul.split_rhat(xf[31:290]), discard=31, upto=290)
    e, last = emul.multichain_ess(xf[:, ::3])
    np.testing.assert_allclose(dc.ess(), e, rtol=1e-9)
    assert np.array_equal(dc.last_pair, last)
    e, last = emul.multichain_ess(xf)
    np.testing.assert_allclose(dc.ess(all_walkers=True), e, rtol=1e-9)
    assert np.array_equal(dc.last_pair, last)
    np.testing.assert_allclose(dc.ess(), emul.multichain_ess(xf[:, ::3])[0], rtol=1e-9)      # the running sums are untouched


@pytest.mark.parametrize("nw", [24, 130])
def test_ess_matches_the_restatement_and_grows_the_lags(nw):
    """The ESS of the chain so far at the checks 100, 200, 600, 1200 and of two other windows; the last pair of Geyer's
    sequence agrees exactly.  With 32 lags to start from, rho = 0.97 needs more: they are added on demand.
    Measured on MI355X: largest relative difference of the ESS 1.2e-13."""
    from linna_amd import sampler
    x = _chain(nw)
    xf = x.astype(np.float64)
    dc = sampler.DeviceChain()
    dc.LAGS0 = 32
    worst = 0.0
    for n0 in range(0, 1200, 100):
        dc.append(torch.as_tensor(x[n0:n0 + 100], device="cuda"))
        got = dc.ess()
        if n0 + 100 in (100, 200, 600, 1200):
            e, last = emul.multichain_ess(xf[:n0 + 100])
            np.testing.assert_allclose(got, e, rtol=1e-9)
            assert np.array_equal(dc.last_pair, last), (n0, dc.last_pair, last)
            worst = max(worst, _rel(got, e))
    assert dc.lag_growths > 0 and len(dc._S) > 32
    for lo, hi in ((0, 450), (90, 451)):
        e, last = emul.multichain_ess(xf[lo:hi])
        np.testing.assert_allclose(dc.ess(discard=lo, upto=hi), e, rtol=1e-9)
        assert np.array_equal(dc.last_pair, last)
    np.testing.assert_allclose(dc.ess(), emul.multichain_ess(xf)[0], rtol=1e-9)
    np.testing.assert_allclose(dc.integrated_time(), sampler.integrated_time(xf), rtol=1e-9)   # tau from the same sums
    print("  nw %d: largest relative difference of the ESS %.3g, lags %d after %d growths" % (nw, worst, len(dc._S), dc.lag_growths))
    want = nw * 1200 * (1 - RHO) / (1 + RHO)                  # (rho = 0.97: too few independent rows for a band)
    assert np.all(np.abs(got[:2] / want[:2] - 1.0) < 0.5)


def test_what_the_tau_rule_cannot_see():
    """Case 4: 3 of 64 chains shifted by three standard deviations (tests/test_rhat_host.py checks the float64 inputs: R-hat
    1.180 and 1.194).  On the device tau and the drift test give the shifted run the verdict of the unshifted one; R-hat is
    above 1.1 and equals the host's value -- asserted against it less 1e-6, a thousand times the parity bar."""
    from linna_amd import sampler
    from test_rhat_host import stuck_chains
    x, y = stuck_chains()
    host = sampler.split_rhat(y.astype(np.float64))
    assert np.all(host > 1.15)
    dx, dy = sampler.DeviceChain(), sampler.DeviceChain()
    dx.append(torch.as_tensor(x, device="cuda"))
    dy.append(torch.as_tensor(y, device="cuda"))
    tx, ty = dx.integrated_time(), dy.integrated_time()
    np.testing.assert_allclose(ty, tx, rtol=1e-6)
    assert np.all(tx * 50 < 400) and np.all(ty * 50 < 400)
    with contextlib.redirect_stdout(io.StringIO()):
        assert dx.checkmeanstd(400, 0.1, 0.1) and dy.checkmeanstd(400, 0.1, 0.1)
    rx, ry = dx.rhat(), dy.rhat()
    assert np.all(rx < 1.01) and np.all(ry > 1.1) and np.all(ry >= host - 1e-6)
    np.testing.assert_allclose(ry, host, rtol=1e-9)
    assert sampler.HMCSampler.rhat_rule(rx, dx.ess()) and not sampler.HMCSampler.rhat_rule(ry, dy.ess())


def test_a_nan_spoils_its_parameter_only_and_never_stops_a_run():
    from linna_amd import sampler
    x = ar1(300, 70, [0.3, 0.5, 0.6], seed=13)
    y = x.copy()
    y[123, 5, 1] = np.nan
    dx, dy = sampler.DeviceChain(), sampler.DeviceChain()
    dx.append(torch.as_tensor(x, device="cuda"))
    dy.append(torch.as_tensor(y, device="cuda"))
    for records in (True, False):
        rx, ry = dx.rhat(records=records), dy.rhat(records=records)
        assert np.isnan(ry[1]) and np.array_equal(ry[[0, 2]], rx[[0, 2]]) and np.all(np.isfinite(rx))
    ex, ey = dx.ess(), dy.ess()
    assert np.isnan(ey[1]) and np.array_equal(ey[[0, 2]], ex[[0, 2]]) and np.all(np.isfinite(ex))
    assert sampler.HMCSampler.rhat_rule(rx, ex, 1.05, 400) and not sampler.HMCSampler.rhat_rule(ry, ey, 1.05, 400)
    assert not sampler.HMCSampler.rhat_rule(ry, ey, np.inf, 0)


def _problem():
    """The 8-parameter Gaussian of test_gpu_hmc_mass (the smallest one the HMC tests build an emulator for), 64 starts drawn
    from it, and a mass that preconditions every parameter but the widest, which it leaves 3 x too wide: with 4 leapfrog
    steps that parameter has an autocorrelation of about 0.55.  The float64 emulation of this run (tests/hmc_adapt_emul.py:
    ``adaptive_run`` with Madapt = 50, seeds 0-4) meets R-hat < 1.01 and ESS >= 400 at 150 or 200 rows, never at 50 or 100;
    5 and 7 leapfrog steps resonate with the preconditioned parameters and are not used."""
    from test_gpu_hmc_mass import target
    t = target()
    x0 = (t["mz"] + t["sz"] * np.random.RandomState(3).standard_normal((64, t["nd"]))).astype(np.float32)
    mass = 1.0 / t["sz"] ** 2
    mass[-1] *= 9.0
    return t, x0, mass


def test_driver_stops_on_rhat_and_ess(tmp_path, monkeypatch):
    """``sample(method="hmc", criterion="rhat", ncheck=50, Madapt=50)`` with a cap of 2000: the run stops before the cap; the
    chain in chhmc.h5 satisfies both thresholds by the restatement at its stored length and not one check earlier;
    ``diagnostics`` holds those numbers."""
    from linna_amd import sampler, util
    t, x0, mass = _problem()
    made = []

    base = sampler.DeviceChain

    class Spy(base):
        def __init__(self, *a, **k):
            base.__init__(self, *a, **k)
            made.append(self)

    monkeypatch.setattr(sampler, "DeviceChain", Spy)
    np.random.seed(1)
    drv = sampler.HMCSampler(t["lp"], None, None, t["nd"], 64, x0=x0, m=mass, transform=util.Transform(t["priors"]), seed=5)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        drv.sample(None, 2000, samp_steps=4, samp_eps=0, Madapt=50, outdir=str(tmp_path), method="hmc", criterion="rhat", ncheck=50)
    d = sampler.ChainStore.load(os.path.join(str(tmp_path), "chhmc.h5"))
    z = np.asarray(d["chain"], np.float64)
    n = len(z)
    print("  stopped at %d rows; %d progress lines" % (n, buf.getvalue().count("max rhat, min ess")))
    assert 50 <= n < 2000 and n % 50 == 0
    rule = sampler.HMCSampler.rhat_rule
    r, e = emul.split_rhat(z)[:, 0], emul.multichain_ess(z)[0]
    print("  at %d: max R-hat %.4f, min ESS %.0f" % (n, r.max(), e.min()))
    assert rule(r, e, 1.01, 400)
    for earlier in range(50, n, 50):
        assert not rule(emul.split_rhat(z[:earlier])[:, 0], emul.multichain_ess(z[:earlier])[0], 1.01, 400), earlier
    assert n > 50                                                  # (a check before the last one exists and failed)
    assert drv.diagnostics["n"] == n
    np.testing.assert_allclose(drv.diagnostics["rhat"], r, rtol=1e-9)
    np.testing.assert_allclose(drv.diagnostics["ess"], e, rtol=1e-9)
    assert buf.getvalue().count("max rhat, min ess") == n // 50
    assert len(made) == 1 and made[0]._M is not None and made[0]._mb == n // _lib.RHAT_BLOCK


def test_the_default_criterion_did_not_move(tmp_path, monkeypatch):
    """``criterion="tau"`` spelled out and no keyword at all: the same chain, log-probabilities and acceptance counts, and no
    block records in either run."""
    from linna_amd import sampler, util
    t, x0, mass = _problem()
    made = []

    base = sampler.DeviceChain

    class Spy(base):
        def __init__(self, *a, **k):
            base.__init__(self, *a, **k)
            made.append(self)

    monkeypatch.setattr(sampler, "DeviceChain", Spy)
    got = []
    for name, kw in (("a", {}), ("b", {"criterion": "tau"})):
        out = os.path.join(str(tmp_path), name)
        os.makedirs(out)
        np.random.seed(1)
        drv = sampler.HMCSampler(t["lp"], None, None, t["nd"], 64, x0=x0, m=mass, transform=util.Transform(t["priors"]), seed=5)
        with contextlib.redirect_stdout(io.StringIO()):
            drv.sample(None, 200, samp_steps=4, samp_eps=0, Madapt=20, outdir=out, method="hmc", ncheck=50, **kw)
        assert drv.diagnostics is None
        got.append(sampler.ChainStore.load(os.path.join(out, "chhmc.h5")))
    a, b = got
    assert len(a["chain"]) >= 50
    for key in ("chain", "log_prob", "accepted"):
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    assert len(made) == 2 and all(m._M is None and m._mb == 0 for m in made)
