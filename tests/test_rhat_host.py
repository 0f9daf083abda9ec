"""CPU: split-R-hat and the multi-chain effective sample size on the host (``sampler.split_rhat`` / ``sampler.multichain_ess``)
against the plain-loop restatement of the definitions (tests/rhat_emul.py), their behaviour on chains whose answer is known,
the case the tau rule cannot see, and the validation of the ``criterion`` keyword."""
import contextlib
import io

import numpy as np
import pytest

import rhat_emul as emul
from linna_amd import sampler, util

SIGMA05 = 1.0 / np.sqrt(1.0 - 0.5 ** 2)         # stationary standard deviation of AR(1) with rho = 0.5 and unit innovations


def stuck_chains():
    """Case 4 of the issue: 64 chains of AR(1) with rho = 0.5, 400 rows, 2 parameters, as float32 (what the device stores);
    in the second array 3 of the chains are shifted by three stationary standard deviations."""
    x = emul.ar1(400, 64, [0.5, 0.5], seed=11).astype(np.float32)
    y = x.copy()
    y[:, [5, 20, 41], :] += np.float32(3.0 * SIGMA05)
    return x, y


@pytest.mark.parametrize("N", [101, 200])
def test_host_functions_equal_the_restatement(N):
    """Odd and even N, a large offset with a small scale: the vectorised host functions (variances by numpy, autocovariances
    by FFT) against loops over chains and lags.  Same float64 inputs, another order of the sums: 1e-12."""
    x = emul.ar1(N, 7, [0.5, 0.9, 0.97], seed=N, mean=np.array([0.0, 30.0, -7.0]), scale=np.array([1.0, 1e-2, 3.0]))
    r = emul.split_rhat(x)
    np.testing.assert_allclose(sampler.split_rhat(x), r[:, 0], rtol=1e-12)
    e, last = emul.multichain_ess(x)
    e2, last2 = sampler.multichain_ess(x, return_pairs=True)
    np.testing.assert_allclose(e2, e, rtol=1e-12)
    assert np.array_equal(last, last2)
    # the middle row of an odd window is dropped: changing it changes nothing
    if N % 2:
        y = x.copy()
        y[N // 2] += 100.0
        assert np.array_equal(sampler.split_rhat(y), sampler.split_rhat(x))
    with pytest.raises(ValueError):
        sampler.split_rhat(x[:3])


def test_iid_and_ar1_chains_give_the_known_answers():
    """i.i.d. normal chains, 16 x 400 x 2: R-hat within 0.01 of 1; ESS / (nw N) measured with the restatement over 40 seeds:
    0.893 ... 1.061, mean 0.999, standard deviation 0.035 -- asserted band [0.8, 1.2], 5.7 standard deviations.
    AR(1) with rho = 0.9, 16 x 1000: ESS / (nw N (1 - rho) / (1 + rho)) over 40 seeds: 0.842 ... 1.143, mean 0.984, standard
    deviation 0.081 -- asserted band [0.6, 1.4], 5 standard deviations.  (R-hat of the i.i.d. chains over those seeds: 0.9988 ...
    1.0016.)"""
    for seed in range(5):
        x = np.random.RandomState(seed).standard_normal((400, 16, 2))
        r, e = sampler.split_rhat(x), sampler.multichain_ess(x)
        assert np.all(np.abs(r - 1.0) < 0.01), r
        assert np.all((e > 0.8 * 16 * 400) & (e < 1.2 * 16 * 400)), e
        y = emul.ar1(1000, 16, [0.9], seed=seed)
        e = sampler.multichain_ess(y) / (16 * 1000 * 0.1 / 1.9)
        assert np.all((e > 0.6) & (e < 1.4)), e


def test_nonfinite_and_constant_chains_give_nan_for_that_parameter_only():
    x = emul.ar1(120, 6, [0.5, 0.7], seed=4)
    r0, e0 = sampler.split_rhat(x), sampler.multichain_ess(x)
    y = x.copy()
    y[17, 2, 1] = np.nan
    r, e = sampler.split_rhat(y), sampler.multichain_ess(y)
    assert np.isnan(r[1]) and np.isnan(e[1]) and r[0] == r0[0] and e[0] == e0[0]
    assert np.isnan(emul.split_rhat(y)[1, 0]) and np.isnan(emul.multichain_ess(y)[0][1])
    z = x.copy()
    z[:, :, 0] = 2.5                                        # no within-chain variance: W = 0
    assert np.isnan(sampler.split_rhat(z)[0]) and np.isnan(emul.split_rhat(z)[0, 0])
    assert np.isnan(sampler.multichain_ess(z)[0]) and sampler.split_rhat(z)[1] == r0[1]


def test_what_the_tau_rule_cannot_see():
    """Three of 64 chains sit three standard deviations away.  tau removes every chain's own mean, and the drift test pools
    the walkers and compares two time halves: both give the shifted run the verdict of the unshifted one.  By the definitions
    B / n grows by about (3 / 64)(61 / 64) 9 W, so R-hat is about sqrt(1 + 0.40) = 1.18 -- far above 1.01 and above 1.1."""
    x, y = stuck_chains()
    xf, yf = x.astype(np.float64), y.astype(np.float64)
    tx, ty = sampler.integrated_time(xf), sampler.integrated_time(yf)
    np.testing.assert_allclose(ty, tx, rtol=1e-6)           # (float32 storage of the shifted values)
    assert np.all(tx * 50 < 400)                            # the tau rule's length condition holds for both
    with contextlib.redirect_stdout(io.StringIO()):
        assert sampler.checkmeanstd(xf, 0.1, 0.1) and sampler.checkmeanstd(yf, 0.1, 0.1)
    rx, ry = sampler.split_rhat(xf), sampler.split_rhat(yf)
    print("  R-hat unshifted %s, shifted %s; ESS %s -> %s" % (rx, ry, sampler.multichain_ess(xf), sampler.multichain_ess(yf)))
    assert np.all(rx < 1.01) and np.all(ry > 1.1) and np.all(np.abs(ry - 1.18) < 0.03)
    assert np.all(sampler.multichain_ess(yf) < 400) and np.all(sampler.multichain_ess(xf) > 400)
    np.testing.assert_allclose(ry, emul.split_rhat(yf)[:, 0], rtol=1e-12)


def test_criterion_keyword_is_validated():
    """No GPU is touched: the keywords are checked first.  ``"rhat"`` belongs to independent chains."""
    s = sampler.HMCSampler(None, None, None, 2, 8)
    with pytest.raises(ValueError, match="criterion"):
        s.sample(None, 100, method="hmc", criterion="gelman")
    with pytest.raises(ValueError, match="independent chains"):
        s.sample(None, 100, method="emcee", criterion="rhat")
    with pytest.raises(ValueError, match="rhat_tol"):
        s.sample(None, 100, method="hmc", criterion="rhat", rhat_tol=1.0)
    with pytest.raises(NotImplementedError):
        s.sample(None, 100, method="nuts")
    with pytest.raises(NotImplementedError):
        s.sample(None, 100, method="nuts", criterion="rhat")
    for method in ("emcee", "zeus"):
        with pytest.raises(ValueError, match="independent chains"):
            util.run_mcmc(None, ".", method, 2, 8, np.zeros(2), None, criterion="rhat")
    with pytest.raises(ValueError, match="criterion"):
        util.run_mcmc(None, ".", "hmc", 2, 8, np.zeros(2), None, criterion="gelman")
