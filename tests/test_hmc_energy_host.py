"""CPU: the energy diagnostics of ``method="hmc"`` (divergent transitions, E-BFMI) -- the numpy restatement
(tests/hmc_energy_emul.py) against closed forms, the new ABI entries' declarations and the argument checks that come before
any launch, and the drivers' keywords and ``ValueError``s."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import hmc_energy_emul as en

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"linna_hmc_energy_doubles": ("size_t", 1), "linna_hmc_accept_energy": ("int", 37), "linna_hmc_run_energy": ("int", 26),
               "linna_hmc_energy_finish": ("int", 7)}
KEYWORDS = [("energy_stats", False), ("max_dH", 1000.0), ("bfmi_min", None), ("max_divergent", None)]


def bfmi_of(E):
    est = en.run(np.asarray(E, np.float64)[:, None])
    return en.finish(est, np.zeros(1, np.int64))[0][0], est[0]


def test_a_constant_series_has_no_bfmi():
    for n in (1, 2, 9):
        b, est = bfmi_of(np.full(n, 3.25))
        assert np.isnan(b) and est[0] == n and est[2] == 0.0 and est[3] == 0.0 and est[4] == 3.25
    assert np.isnan(bfmi_of([1.0])[0])                       # n < 2
    assert np.isnan(en.finish(en.empty(3), np.zeros(3, np.int64))[1][0])


@pytest.mark.parametrize("N", [2, 3, 8, 101])
def test_an_alternating_series(N):
    """a, b, a, b, ...: D2 = (N - 1)(a - b)^2 and, for even N, M2 = N (a - b)^2 / 4, so D2 / M2 = 4 (N - 1) / N; for odd N
    M2 = (N^2 - 1)(a - b)^2 / (4 N) and D2 / M2 = 4 N / (N + 1)."""
    a, b = 1.5, -2.25
    got, est = bfmi_of([a if i % 2 == 0 else b for i in range(N)])
    want = 4.0 * (N - 1) / N if N % 2 == 0 else 4.0 * N / (N + 1)
    assert est[0] == N and est[3] == (N - 1) * (a - b) ** 2
    np.testing.assert_allclose(got, want, rtol=1e-12)


def test_a_float64_series_against_the_two_pass_form():
    rs = np.random.RandomState(4)
    for N in (2, 7, 500):
        E = 40.0 + 3.0 * np.cumsum(rs.standard_normal(N)) * 0.1 + rs.standard_normal(N)
        got, est = bfmi_of(E)
        np.testing.assert_allclose(got, np.sum(np.diff(E) ** 2) / np.sum((E - E.mean()) ** 2), rtol=1e-12)
        np.testing.assert_allclose(est[1], E.mean(), rtol=1e-12)
        assert est[4] == E[-1]


def test_a_non_finite_energy_changes_nothing_and_the_state_continues():
    E = np.array([[1.0, 2.0], [np.nan, 2.5], [3.0, np.inf], [0.5, -np.inf], [2.0, 1.0]])
    est = en.run(E)
    np.testing.assert_array_equal(est[0], en.run(np.array([[1.0], [3.0], [0.5], [2.0]]))[0])
    np.testing.assert_array_equal(est[1], en.run(np.array([[2.0], [2.5], [1.0]]))[0])
    # one call equals the loop: Eprev carries
    a = en.run(E[:2])
    en.run(E[2:], a)
    np.testing.assert_array_equal(a, est)


def test_the_divergence_predicate_and_the_pooled_values():
    f = np.float32
    up = np.nextafter(f(1000), f(np.inf))
    dH = np.array([1000.0, up, -5.0, np.nan, 1.0, 1.0, 1.0, np.inf, -np.inf], f)
    ln = np.array([0.0, 0.0, 0.0, 0.0, np.nan, -np.inf, np.inf, 0.0, 0.0], f)
    assert list(en.divergent(ln, dH, 1000.0)) == [False, True, False, True, True, True, True, True, False]
    est = np.array([[3, 0, 2.0, 1.0, 0], [1, 0, 0.0, 0.0, 0], [4, 0, 1.0, 3.0, 0], [5, 0, 0.0, 0.0, 0]], np.float64)
    bfmi, pooled = en.finish(est, np.array([0, 2, 0, 5]))
    assert bfmi[0] == 0.5 and np.isnan(bfmi[1]) and bfmi[2] == 3.0 and np.isnan(bfmi[3])
    assert list(pooled) == [0.5, 7.0, 2.0]
    # the accept restatement on exact inputs: E = acc ? H1 : H0, dH = H1 - H0
    acc, E, d, div = en.accept(np.array([[2.0, 0.0], [1.0, 1.0], [0.0, 0.0]]), [1.0, 0.5], [1.0, 1.0, 0.0], [1.0, -0.5, np.nan],
                               [0.5, 0.9, 0.0], 1000.0)
    assert list(acc) == [True, False, False] and list(E[:2]) == [1.0, 1.0] and E[2] == 0.0
    assert list(d[:2]) == [0.0, 1.0] and np.isnan(d[2]) and list(div) == [False, False, True]


def test_header_declares_the_new_entries_and_the_binding_matches():
    from linna_amd import _lib
    from test_abi import header_functions
    decl = header_functions()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, nargs) in NEW_ENTRIES.items():
        assert decl[name] == (ret, nargs), (name, decl.get(name))
        res, args = _lib._SIGNATURES[name]
        assert res is (ctypes.c_size_t if ret == "size_t" else ctypes.c_int) and len(args) == nargs
        assert hasattr(lib, name)
    # the argument lists the new entries extend
    assert _lib._SIGNATURES["linna_hmc_accept_energy"][1][:31] == _lib._SIGNATURES["linna_hmc_accept_adapt"][1][:31]
    assert _lib._SIGNATURES["linna_hmc_run_energy"][1][:20] == _lib._SIGNATURES["linna_hmc_run_dense"][1][:20]
    for name in ("linna_hmc_accept_energy", "linna_hmc_run_energy"):
        assert _lib._SIGNATURES[name][1][-4] is ctypes.c_float                        # max_dH
    header = open(os.path.join(ROOT, "include", "linna_hip.h")).read()
    m = re.search(r"#define\s+LINNA_HMC_ENERGY_DOUBLES\s+(\d+)", header)
    assert m and int(m.group(1)) == 5 == _lib.ENERGY_DOUBLES == en.DOUBLES
    assert "N / (N - 1)" in header                              # (the header says which E-BFMI this is)
    assert [_lib.load().linna_hmc_energy_doubles(n) for n in (-1, 0, 1, 5, 4096)] == [0, 0, 5, 25, 20480]
    assert _lib.ABI_VERSION == 12                               # (entries were added, none changed)


def test_bad_arguments_are_refused_without_a_gpu():
    from linna_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(64)                                  # (a pointer that is never followed: every call fails before a launch)
    assert lib.linna_hmc_energy_finish(None, 0, one, one, one, one, None) == _lib.ERR_INVALID
    assert b"hmc_energy_finish" in lib.linna_last_error()
    for miss in range(4):
        args = [one] * 4
        args[miss] = None
        assert lib.linna_hmc_energy_finish(None, 4, *args, None) == _lib.ERR_INVALID
    base = [None, 4, 3, one, 1, one, 0, one, one, 4, one, 4, one, one, 4, None, one, 4, one, one, one, one, None, None, None, None,
            None, 0, 0.65, None, None]
    accept = lambda *tail: lib.linna_hmc_accept_energy(*(base + list(tail) + [None]))
    assert accept(one, None, 1000.0, None, None) == _lib.ERR_INVALID and b"estate and ndiv" in lib.linna_last_error()
    assert accept(None, one, 1000.0, None, None) == _lib.ERR_INVALID and b"estate and ndiv" in lib.linna_last_error()
    for bad in (0.0, -1.0, float("nan")):
        assert accept(one, one, bad, None, None) == _lib.ERR_INVALID and b"max_dH" in lib.linna_last_error()
    assert lib.linna_hmc_accept_energy(*([None, 0] + base[2:] + [one, one, 1000.0, None, None, None])) == _lib.ERR_INVALID
    assert b"hmc_accept_energy" in lib.linna_last_error()
    # linna_hmc_run_energy: hmc_run's own checks, then the group's, all before the state is looked at
    run = lambda *tail: lib.linna_hmc_run_energy(one, one, one, None, 0, one, None, None, None, None, 0, 0.65, 0, 3, 2, None, None, None,
                                                 None, None, *tail, None)
    assert lib.linna_hmc_run_energy(None, None, None, None, 0, None, None, None, None, None, 0, 0.65, 0, 3, 2, None, None, None, None,
                                    None, None, None, 1000.0, None, None, None) == _lib.ERR_INVALID
    assert b"hmc_run" in lib.linna_last_error()
    assert run(one, None, 1000.0, None, None) == _lib.ERR_INVALID and b"estate and ndiv" in lib.linna_last_error()
    assert run(one, one, 0.0, None, None) == _lib.ERR_INVALID and b"max_dH" in lib.linna_last_error()


def test_the_keywords_are_appended_and_default_to_off():
    from linna_amd import sampler, util
    for fn in (sampler.HMCSampler.sample, util.NN_samplerv1._HMC_sample, util.run_mcmc):
        p = inspect.signature(fn).parameters
        assert [(k, p[k].default) for k in list(p)[-4:]] == KEYWORDS, fn
        assert list(p)[-5] == "ess_rank", fn
    p = inspect.signature(sampler.BatchedHMC.run).parameters
    assert list(p)[-1] == "energy" and p["energy"].default is False
    p = inspect.signature(sampler.BatchedHMC.energy_stats).parameters
    assert p["on"].default is True and p["max_dH"].default == 1000.0


def test_argument_errors_come_before_any_gpu_work():
    from linna_amd import sampler, util
    s = sampler.HMCSampler(None, None, None, 3, 8, x0=np.zeros((8, 3)))
    with pytest.raises(ValueError, match="energy_stats"):
        s.sample(None, 10, method="emcee", energy_stats=True)
    for kw in (dict(bfmi_min=0.3), dict(max_divergent=0.01)):
        name = list(kw)[0]
        with pytest.raises(ValueError, match=name):                               # without energy_stats
            s.sample(None, 10, method="hmc", criterion="rhat", **kw)
        with pytest.raises(ValueError, match=name):                               # without criterion="rhat"
            s.sample(None, 10, method="hmc", energy_stats=True, **kw)
        with pytest.raises(ValueError, match=name):
            util.run_mcmc(None, ".", "hmc", 3, 8, np.zeros(3), None, energy_stats=True, **kw)
        with pytest.raises(ValueError, match=name):
            util.run_mcmc(None, ".", "hmc", 3, 8, np.zeros(3), None, criterion="rhat", **kw)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_dH"):
            s.sample(None, 10, method="hmc", energy_stats=True, max_dH=bad)
        with pytest.raises(ValueError, match="max_dH"):
            util.run_mcmc(None, ".", "hmc", 3, 8, np.zeros(3), None, energy_stats=True, max_dH=bad)
    with pytest.raises(ValueError, match="energy_stats"):
        util.run_mcmc(None, ".", "zeus", 3, 8, np.zeros(3), None, energy_stats=True)
    # a multi-rank run says so
    args = (None, "hmc", 0, 10, False, False, 64, "rhat", 1.01, 400, 0.0, False, False)
    with pytest.raises(ValueError, match="single-rank"):
        sampler.HMCSampler._check(*args, True, 1000.0, None, None, world=2)
    assert sampler.HMCSampler._check(*args, True, 1000.0, 0.3, 0.01, world=1) is False
    assert sampler.HMCSampler._check(*args) is False                              # (the parent's call)
    # BatchedHMC.energy_stats checks max_dH before it touches the device
    h = sampler.BatchedHMC.__new__(sampler.BatchedHMC)
    h.estate = h.ndiv = None
    with pytest.raises(ValueError, match="max_dH"):
        h.energy_stats(True, 0.0)
    with pytest.raises(ValueError, match="energy_stats"):
        h.energy_summary()


def test_the_driver_flags_from_dH_alone_are_the_kernels_on_a_chain_that_started_finite():
    """``_EnergyLog.divergent`` sees only dH: with a finite H0 the kernel's flag is a function of dH (lnp_new = +inf gives
    dH = -inf, NaN gives NaN, -inf gives +inf)."""
    from linna_amd import sampler
    f = np.float32
    H0 = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -3.0], f)
    ln = np.array([0.0, np.nan, -np.inf, np.inf, -2000.0, -1001.0, -997.0], f)
    with np.errstate(invalid="ignore"):
        dH = (-ln - H0).astype(f)                                   # (P = 0: H1 = -lnp_new)
    want = en.divergent(ln, dH, 1000.0)
    assert list(want) == [False, True, True, True, True, False, False]
    np.testing.assert_array_equal(sampler._EnergyLog.divergent(dH, 1000.0), want)
