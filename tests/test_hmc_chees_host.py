"""CPU: the trajectory-length adaptation of ``method="hmc"`` (ChEES) -- the three new C entries and their constants in the
header and the binding at ABI 12, the van der Corput numbers and the step counts with their clamps on the product and on the
emulation (tests/hmc_chees_emul.py), the keywords through the drivers with their argument errors, the emulation's state
update by hand on a small case, and the emulation itself on the Gaussian the GPU test runs."""
import copy
import inspect
import math
import os
import re

import numpy as np
import pytest

import hmc_adapt_emul as emul
import hmc_chees_emul as chees

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"linna_hmc_chees_doubles": ("size_t", 1), "linna_hmc_chees_begin": ("int", 8), "linna_hmc_chees_end": ("int", 18)}
CONSTANTS = {"HEAD": 12, "LR": 0.025, "BETA1": 0.9, "BETA2": 0.999, "ADAM_EPS": 1e-8, "ALPHA_FLOOR": 1e-3, "MAX_STEPS": 64}


def test_header_declares_the_new_entries_and_the_binding_matches():
    import ctypes
    from linna_amd import _lib
    from test_abi import header_functions
    decl = header_functions()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, (ret, nargs) in NEW_ENTRIES.items():
        assert decl[name] == (ret, nargs), (name, decl.get(name))
        res, args = _lib._SIGNATURES[name]
        assert res is (ctypes.c_size_t if ret == "size_t" else ctypes.c_int) and len(args) == nargs
        assert hasattr(lib, name)
    assert _lib._SIGNATURES["linna_hmc_chees_end"][1][15] is ctypes.c_double          # delta
    header = open(os.path.join(ROOT, "include", "linna_hip.h")).read()
    for name, value in CONSTANTS.items():
        m = re.search(r"#define\s+LINNA_HMC_CHEES_%s\s+(\S+)" % name, header)
        assert m and float(m.group(1)) == value, name
        assert getattr(_lib, "CHEES_" + name) == value and getattr(chees, name) == value, name
    assert _lib.ABI_VERSION == 12 and _lib.load().linna_abi_version() == 12
    assert re.search(r"#define\s+LINNA_ABI_VERSION\s+12\b", header)
    lib = _lib.load()
    assert [lib.linna_hmc_chees_doubles(n) for n in (-1, 0, 1, 33, 1000)] == [0, 0, 14, 12 + 66, 2012]


def test_bad_arguments_are_refused_without_a_gpu():
    from linna_amd import _lib
    lib = _lib.load()
    assert lib.linna_hmc_chees_begin(None, 0, 3, None, 4, None, None, None) == _lib.ERR_INVALID
    assert b"hmc_chees_begin" in lib.linna_last_error()
    assert lib.linna_hmc_chees_end(None, 4, 3, None, None, 0, None, 4, None, 4, None, None, None, None, 10, 0.65, 64, None) == _lib.ERR_INVALID
    assert b"hmc_chees_end" in lib.linna_last_error()


def test_halton_and_the_step_counts():
    from linna_amd import sampler
    H = sampler.BatchedHMC.halton
    want = [0.5, 0.25, 0.75, 0.125, 0.625, 0.375, 0.875, 0.0625]
    assert [H(t) for t in range(1, 9)] == want == [chees.halton(t) for t in range(1, 9)]
    assert H(2 ** 20) == 2.0 ** -21 and H(2 ** 20 - 1) == 1.0 - 2.0 ** -20
    for t in (1, 7, 300, 12345, 2 ** 31 - 1):
        assert H(t) == chees.halton(t) and 0.0 < H(t) < 1.0
    S = sampler.BatchedHMC.traj_steps
    cases = [((0.5, 1.0, 0.1, 64), 5), ((0.5, 1.0, 0.1 + 1e-12, 64), 5), ((0.5, 1.0, 0.1 - 1e-12, 64), 6), ((0.25, 0.03, 0.03, 64), 1),
             ((0.875, 100.0, 0.1, 64), 64), ((0.875, 100.0, 0.1, 7), 7), ((0.5, 0.0, 0.1, 64), 1), ((0.5, float("nan"), 0.1, 64), 1),
             ((0.5, float("inf"), 0.1, 64), 64), ((1.0, 6.4, 0.1, 64), 64), ((0.5, 0.2, 0.1, 64), 1), ((0.5, 0.2 + 1e-9, 0.1, 64), 2)]
    for args, n in cases:
        assert S(*args) == n == chees.steps(*args), (args, S(*args), chees.steps(*args))
    # steps_for: Philox step i uses h_{i + 1}
    h = sampler.BatchedHMC.__new__(sampler.BatchedHMC)
    h.traj, h._traj_eps, h.max_steps = 0.9, 0.05, 16
    got = [h.steps_for(i) for i in range(8)]
    assert got == [9, 5, 14, 3, 12, 7, 16, 2] == [chees.steps_for(i, 0.9, 0.05, 16) for i in range(8)]
    h.traj = None
    with pytest.raises(ValueError, match="trajectory length"):
        h.steps_for(0)


def test_adapt_traj_is_a_trailing_keyword_that_defaults_to_off():
    from linna_amd import sampler, util
    for fn in (sampler.HMCSampler.sample, sampler.HMCSampler._hmc_chains, util.NN_samplerv1._HMC_sample, util.run_mcmc,
               sampler.BatchedHMC.adapt):
        p = inspect.signature(fn).parameters
        assert p["adapt_traj"].default is False and "max_steps" in p, fn
        names = list(p)
        assert names.index("adapt_traj") > names.index("adapt_mass"), fn
    assert inspect.signature(sampler.BatchedHMC.run).parameters["num_steps"].default is None
    p = inspect.signature(sampler.BatchedHMC.adapt_traj).parameters
    assert p["target_accept"].default == 0.65 and p["max_steps"].default in (None, 64)
    # the reference's positional order stays in front
    assert list(inspect.signature(util.NN_samplerv1._HMC_sample).parameters)[:12] == [
        "self", "log_prob", "dlnp", "ddlnp", "ndim", "nwalkers", "init", "pool", "transform", "samp_steps", "samp_eps", "Madapt"]


def test_argument_errors_come_before_any_gpu_work():
    from linna_amd import sampler, util
    s = sampler.HMCSampler(None, None, None, 3, 8, x0=np.zeros((8, 3)))
    with pytest.raises(ValueError, match="adapt_traj"):
        s.sample(None, 10, samp_eps=0.004, method="hmc", adapt_traj=True)
    with pytest.raises(ValueError, match="adapt_traj"):
        s.sample(None, 10, method="emcee", adapt_traj=True)
    with pytest.raises(ValueError, match="max_steps"):
        s.sample(None, 10, method="hmc", adapt_traj=True, max_steps=0)
    with pytest.raises(ValueError, match="Madapt"):
        s.sample(None, 10, Madapt=0, method="hmc", adapt_traj=True)
    with pytest.raises(ValueError, match="adapt_traj"):
        util.run_mcmc(None, ".", "emcee", 3, 8, np.zeros(3), None, adapt_traj=True)
    with pytest.raises(ValueError, match="max_steps"):
        util.run_mcmc(None, ".", "hmc", 3, 8, np.zeros(3), None, adapt_traj=True, max_steps=0)


def test_a_file_without_a_trajectory_length_is_not_taken(tmp_path):
    """``_load_adaptation(traj=True)``: the file of a mass-only run, or one whose ``traj`` is not finite and positive, is not
    handed to an ``adapt_traj`` run; a run without the keyword takes either as before."""
    from linna_amd import sampler

    class Ens(object):
        ndim, B = 3, 4
    name = str(tmp_path / "chhmc_adapt.npz")
    base = dict(mass=np.ones(3, np.float32), eps=np.full(4, 0.1, np.float32), num_steps=np.int64(5), Madapt=np.int64(20))
    load = sampler.HMCSampler._load_adaptation
    np.savez(name, **base)
    assert load(name, Ens, "diag", traj=True) is None and set(load(name, Ens, "diag")) == {"mass", "eps"}
    for bad in (np.nan, 0.0, -1.0, np.inf):
        np.savez(name, traj=np.float64(bad), max_steps=np.int64(64), iteration=np.int64(21), **base)
        assert load(name, Ens, "diag", traj=True) is None and set(load(name, Ens, "diag")) == {"mass", "eps"}
    np.savez(name, traj=np.float64(0.7), max_steps=np.int64(32), iteration=np.int64(21), **base)
    got = load(name, Ens, "diag", traj=True)
    assert got["traj"] == 0.7 and got["max_steps"] == 32 and got["iteration"] == 21
    assert set(load(name, Ens, "diag")) == {"mass", "eps"}
    assert load(name, Ens, "dense", traj=True) is None


def test_the_state_update_by_hand():
    """Three chains in two dimensions, one of them invalid, at t = 1 with M = 1: every word of the state against the formulas of
    include/linna_hip.h written out here, and the freeze."""
    q = np.array([[0.5, -0.25], [1.5, 0.75], [np.nan, 0.0]], np.float32)
    p = np.array([[1.0, 2.0], [-0.5, 0.25], [0.0, 0.0]], np.float32)
    mass = np.array([2.0, 0.5], np.float32)
    alpha = np.array([0.5, 1.0, 0.9], np.float32)
    x = np.array([[0.0, 0.0], [1.0, 1.0], [2.0, -1.0]], np.float32)
    m0, r0 = chees.begin(x)
    assert np.array_equal(m0, [1.0, 0.0]) and np.array_equal(r0, [1.0, 1.0, 2.0])
    eps0 = 0.125
    for M, frozen in ((5, False), (1, True)):
        st = chees.new_state(eps0)
        out = chees.end(st, q, p, alpha, r0, M, 0.65, 64, mass=mass)
        assert list(out["valid"]) == [True, True, False] and np.array_equal(out["m1"], [1.0, 0.25])
        e = np.array([[-0.5, -0.5], [0.5, 0.5]])
        v = np.array([[0.5, 4.0], [-0.25, 0.5]])
        c = 0.5 * ((e * e).sum(1) - 1.0) * (e * v).sum(1)
        g = (0.5 * c[0] + 1.0 * c[1]) / 1.5
        assert np.allclose(out["c"][:2], c, rtol=1e-15) and st["g"] == pytest.approx(g, rel=1e-15)
        G = g * eps0
        a, vv = 0.1 * G, 0.001 * G * G
        logT = math.log(eps0) + 0.025 * (a / 0.1) / (math.sqrt(vv / (1 - 0.999)) + 1e-8)
        hm = 3.0 / (1 / 0.5 + 1 / 1.0 + 1 / 1e-3)
        Hbar = (0.65 - hm) / 11.0
        logeps = math.log(10 * eps0) - 1.0 / 0.05 * Hbar
        assert st["a"] == pytest.approx(a, rel=1e-14) and st["v"] == pytest.approx(vv, rel=1e-14)
        assert st["hm"] == pytest.approx(hm, rel=1e-15) and st["Hbar"] == pytest.approx(Hbar, rel=1e-15)
        assert st["logeps"] == pytest.approx(logeps, rel=1e-14) and st["logepsbar"] == pytest.approx(logeps, rel=1e-14)   # w = 1 at t = 1
        assert st["logTbar"] == pytest.approx(logT, rel=1e-13) and st["t"] == 2.0 and st["nvalid"] == 2.0
        clamped = min(max(logT, logeps), logeps + math.log(64.0))
        assert st["logT"] == pytest.approx(logT if frozen else clamped, rel=1e-13)
        assert out["eps"] == np.float32(math.exp(logeps)) and out["eps"].dtype == np.float32
    # no valid chain: Adam and the average of log T are skipped, the step size still moves, log T is only clamped
    st = chees.new_state(eps0)
    st.update(a=0.3, v=0.2, logTbar=-1.0, g=7.0)
    before = copy.deepcopy(st)
    out = chees.end(st, q, p, np.zeros(3, np.float32), r0, 5, 0.65, 64, mass=mass)
    assert not out["valid"].any()
    assert all(st[k] == before[k] for k in ("a", "v", "logTbar", "g", "mu")) and st["nvalid"] == 0.0 and st["hm"] == pytest.approx(1e-3)
    assert st["logeps"] != before["logeps"] and st["logT"] == max(before["logT"], st["logeps"])


@pytest.mark.parametrize("seed", chees.SEEDS)
def test_the_emulation_meets_the_conditions(seed):
    """The float64 emulation on the Gaussian of widths geomspace(0.02, 0.6, 8): 256 chains, 300 warm-up and 300 stored
    transitions at unit mass.  std within 5 %, acceptance above 0.4, the lag-1 autocorrelation of the widest parameter
    below that of 5 fixed steps at the same frozen step size by the recorded margin, traj / the largest width in the
    recorded band (the figures are in tests/hmc_chees_emul.py and DESIGN.md section 3.10)."""
    B, M, N = 256, 300, 300
    fg = emul.gaussian_fg(chees.MEAN, chees.WIDTHS)
    r = chees.adapt_run(fg, chees.start(B, seed), seed, M, 0.65, 0)
    assert r["Ls"][0] == 1 and r["state"]["t"] == M + 1.0 and r["cur"]["step"] == M
    assert 1 <= min(r["Ls"]) and max(r["Ls"]) <= 64
    cur5 = copy.deepcopy(r["cur"])
    chain, acc, Ls = chees.sample(fg, r["cur"], seed, N, r["eps"], lambda i: chees.steps_for(i, r["traj"], r["eps"]))
    chain5, acc5, _ = chees.sample(fg, cur5, seed, N, r["eps"], lambda i: 5)
    assert Ls == [chees.steps_for(i, r["traj"], r["eps"]) for i in range(M, M + N)]
    print("  seed %d: step size %.4g (the search's median %.4g), mean leapfrog steps %.1f in the warm-up, %.1f afterwards"
          % (seed, r["eps"], r["eps0"], np.mean(r["Ls"]), np.mean(Ls)))
    chees.conditions("emulation, seed %d" % seed, r["traj"], acc / float(N), chain, chain5)
