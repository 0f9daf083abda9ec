"""CPU: the mass adaptation of ``method="hmc"`` -- the window schedule on the product and on the emulation
(tests/hmc_mass_emul.py), the three new C entries in the header and the binding at ABI 12, the emulation's Chan merge
against numpy's two-pass variance, and the keyword through the drivers."""
import inspect
import os
import re

import numpy as np
import pytest

import hmc_mass_emul as memul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = {1000: [(75, 100), (100, 150), (150, 250), (250, 450), (450, 950)], 200: [(75, 100), (100, 150)], 150: [(75, 100)],
           100: [(15, 90)], 20: [(3, 18)], 19: [], 0: []}
NEW_ENTRIES = {"linna_hmc_moments": 7, "linna_hmc_mass_from_moments": 6, "linna_hmc_run_moments": 19}


@pytest.mark.parametrize("Madapt", sorted(WINDOWS))
def test_mass_windows_pinned(Madapt):
    from linna_amd import sampler
    assert sampler.BatchedHMC.mass_windows(Madapt) == WINDOWS[Madapt]
    assert memul.mass_windows(Madapt) == WINDOWS[Madapt]


def test_mass_windows_tile_the_slow_phase():
    """Every warm-up length from 20 to 1200: windows are contiguous, start at the initial buffer, end at the closing one, never
    shrink, and the product and the emulation agree."""
    from linna_amd import sampler
    for M in range(20, 1201):
        w = sampler.BatchedHMC.mass_windows(M)
        assert w == memul.mass_windows(M) and w, M
        assert all(a < b for a, b in w) and all(w[i][1] == w[i + 1][0] for i in range(len(w) - 1)), (M, w)
        init, term = (75, 50) if M >= 150 else (int(0.15 * M), int(0.1 * M))
        assert w[0][0] == init and w[-1][1] == M - term, (M, w)
        sizes = [b - a for a, b in w]
        assert sizes == sorted(sizes), (M, w)


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
    # linna_hmc_run_moments = linna_hmc_run's arguments with `double* mom` in front of the stream
    assert decl["linna_hmc_run"] == ("int", 18)
    run, mom = _lib._SIGNATURES["linna_hmc_run"][1], _lib._SIGNATURES["linna_hmc_run_moments"][1]
    assert mom[:17] == run[:17] and mom[17] is ctypes.c_void_p and mom[18] is run[17]
    assert _lib.ABI_VERSION == 12 and _lib.load().linna_abi_version() == 12
    assert re.search(r"#define\s+LINNA_ABI_VERSION\s+12\b", open(os.path.join(ROOT, "include", "linna_hip.h")).read())
    assert ctypes.sizeof(_lib.HmcState) == 16 + 8 + 10 * 8


def test_bad_arguments_are_refused_without_a_gpu():
    from linna_amd import _lib
    lib = _lib.load()
    assert lib.linna_hmc_moments(None, 0, 3, None, 4, None, None) == _lib.ERR_INVALID
    assert b"hmc_moments" in lib.linna_last_error()
    assert lib.linna_hmc_mass_from_moments(None, 3, None, None, 1, None) == _lib.ERR_INVALID
    assert b"hmc_mass_from_moments" in lib.linna_last_error()
    assert lib.linna_hmc_run_moments(None, None, None, None, None, None, None, None, 0, 0.65, 0, 1, 1, None, None, None, None, None,
                                     None) == _lib.ERR_INVALID


def test_chan_merge_equals_the_two_pass_variance():
    """Three uneven batches with different offsets and scales: n exact, mean and M2 within 1e-13 relative of numpy's two-pass
    float64 result over all rows."""
    rs = np.random.RandomState(0)
    nd = 9
    batches = [3.0 + 0.1 * rs.standard_normal((5, nd)), -1.0 + 2.0 * rs.standard_normal((131, nd)), 0.5 + 1e-3 * rs.standard_normal((64, nd))]
    mom = memul.empty_moments(nd)
    for b in batches:
        memul.merge(mom, b.astype(np.float32))
    rows = np.concatenate([b.astype(np.float32) for b in batches]).astype(np.float64)
    mean = rows.mean(0)
    M2 = ((rows - mean) ** 2).sum(0)
    assert mom["n"] == 200.0
    np.testing.assert_allclose(mom["M2"], M2, rtol=1e-13)
    assert np.all(np.abs(mom["mean"] - mean) <= 1e-13 * (np.abs(mean) + rows.std(0)))
    np.testing.assert_allclose(mom["M2"] / (mom["n"] - 1), rows.var(0, ddof=1), rtol=1e-13)


def test_mass_formula_keeps_what_it_cannot_compute():
    mom = dict(n=100.0, mean=np.zeros(4), M2=np.array([99.0 * 0.04, 0.0, np.nan, 99.0 * 1e-6]))
    old = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    got = memul.mass_from_moments(mom, old)
    want0 = 1.0 / (0.04 * 100 / 105 + 1e-3 * 5 / 105)
    assert got.dtype == np.float32 and got[0] == np.float32(want0) and got[2] == 3.0
    assert got[1] == np.float32(1.0 / (1e-3 * 5 / 105))                 # all rows agree: the shrinkage term alone
    assert np.array_equal(memul.mass_from_moments(dict(mom, n=1.0), old), old)
    assert np.array_equal(old, [1.0, 2.0, 3.0, 4.0])                      # (the input is not written)


def test_emulated_adaptation_on_a_badly_scaled_gaussian():
    """The issue's numbers, on a smaller run: 4-D Gaussian of widths 0.003 ... 0.3, 64 chains from the mode, Madapt = 200.  The
    adapted mass times the variance is near one, and the frozen step size is tens of times the unit-mass one."""
    nd, B = 4, 64
    sig = np.geomspace(0.003, 0.3, nd)
    fg = emul_fg(sig)
    x0 = 0.01 * sig.min() * np.random.RandomState(1).standard_normal((B, nd))
    out = memul.adapt_run(fg, x0, np.ones(nd), 3, 5, 200, 0.65, 100, dtype=np.float64, store=True)
    unit = memul.adapt_run(fg, x0, np.ones(nd), 3, 5, 200, 0.65, 0, adapt_mass=False, dtype=np.float64)
    assert out["windows"] == [(75, 100), (100, 150)] and unit["windows"] == []
    ratio = np.median(out["eps"]) / np.median(unit["eps"])
    print("  mass * sigma^2 %s, step size ratio %.1f, acceptance %.3f" % (np.round(out["mass"] * sig ** 2, 3), ratio, out["acc_after"].mean() / 100))
    assert np.all(np.abs(np.log(out["mass"] * sig ** 2)) < np.log(1.5)) and ratio > 30
    assert (out["state"]["m"] == 50 + 1 + 100 + 1).all() and np.array_equal(out["state"]["eps"], out["state"]["epsbar"])
    assert np.array_equal(unit["mass"], np.ones(nd))


def emul_fg(sig):
    import hmc_adapt_emul as emul
    return emul.gaussian_fg(np.zeros(len(sig)), sig)


def test_adapt_mass_is_a_trailing_keyword_that_defaults_to_off():
    from linna_amd import sampler, util
    for fn in (sampler.HMCSampler.sample, sampler.HMCSampler._hmc_chains, util.NN_samplerv1._HMC_sample, util.run_mcmc):
        p = inspect.signature(fn).parameters["adapt_mass"]
        assert p.default is False, fn
    assert inspect.signature(sampler.BatchedHMC.run).parameters["moments"].default is False
    assert inspect.signature(sampler.BatchedHMC.adapt).parameters["adapt_mass"].default is True
    s = sampler.HMCSampler(None, None, None, 3, 8, x0=np.zeros((8, 3)))
    with pytest.raises(ValueError, match="adapt_mass"):
        s.sample(None, 10, samp_eps=0.004, method="hmc", adapt_mass=True)
