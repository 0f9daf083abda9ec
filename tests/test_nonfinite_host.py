"""Host (no GPU): the side conditions tests/test_gpu_nonfinite.py rests on, pinned on the oracle alone -- which rows of a
poisoned batch the reference rejects, that every move scenario of tests/poison.py really meets rejected points, and what
``np.minimum`` / ``np.exp`` (HMCSampler.py:57-59) decide on a NaN energy."""
import numpy as np
import pytest

import cases
import poison


@pytest.mark.parametrize("name", poison.NETWORKS)
def test_the_poisoned_rows_and_only_those_are_minus_inf(name):
    from oracle import likelihood
    prob = poison.poisoned_problem(name, (0, 1))
    assert prob["dolog10"] == [0, 1] and cases.serving_problem(name)["priors"][0]["dist"] == "flat"      # (a copy: the case stands)
    z, twin = poison.batch(prob["nin"])
    bad = np.zeros(len(z), bool)
    bad[list(poison.SERVING_ROWS)] = True
    th = likelihood.prior_map(z, prob["priors"])
    np.testing.assert_array_equal(th[[0, 15, 16, 36], 0], np.float32([-0.5, 0.0, -2.0, -0.5]))
    assert np.all(th[~bad, 0] > 0) and np.all(th[:, 1] >= 0.1)
    emu = cases.oracle_emulator(prob)
    for dt in (np.float32, np.float64):
        with np.errstate(invalid="ignore", divide="ignore"):
            lnp = likelihood.log_prob(z, emu, prob["priors"], prob["data"], prob["invcov"], 1.0, dtype=dt)
            lg, g = likelihood.grad_log_prob(z, emu, prob["priors"], prob["data"], prob["invcov"], 1.0, dtype=dt)
        for v in (lnp, lg):
            assert np.all(v[bad] == -np.inf), (name, dt, v[bad])
            assert np.all(np.isfinite(v[~bad])), (name, dt)
        assert np.all(np.isfinite(g[~bad]))
        clean = likelihood.log_prob(twin, emu, prob["priors"], prob["data"], prob["invcov"], 1.0, dtype=dt)
        assert np.all(np.isfinite(clean))
        np.testing.assert_array_equal(clean[~bad], lnp[~bad])          # rows are independent in the oracle


def test_the_stretch_scenario_proposes_rejected_points():
    """64 walkers of poisoned simple_6_4 just inside theta0 > 0, 4 iterations of the oracle's own replay: at least 10 of the
    256 proposals are -inf, none is taken, every lnP stays finite."""
    s = poison.STRETCH
    prob = poison.poisoned_problem(s["name"])
    f = poison.oracle_fn(prob, s["T"])
    coords = poison.stretch_start()
    assert np.all(1.0 + coords[:, 0] >= 0.1 - 1e-6)
    logp = f(coords)
    assert np.all(np.isfinite(logp))
    halves = np.arange(s["nw"]).reshape(2, s["nw"] // 2)
    npois = nacc = 0
    for it in range(s["iters"]):
        for h in (0, 1):
            S, Cc = halves[h], halves[1 - h]
            q, new_lp, acc, coords, logp = poison.stretch_half(coords, logp, S, Cc, poison.stretch_lib_seed(), it, h, f)
            pois = new_lp == -np.inf
            assert not np.any(acc & pois)
            assert np.array_equal(pois, ~(1.0 + q[:, 0] > 0))           # -inf exactly where theta0 <= 0
            npois += int(pois.sum()); nacc += int(acc.sum())
            assert np.all(np.isfinite(logp)) and np.all(1.0 + coords[:, 0] > 0)
    print("stretch scenario: %d of %d proposals -inf, %d accepted" % (npois, s["iters"] * s["nw"], nacc))
    assert npois >= 10 and 20 <= nacc <= s["iters"] * s["nw"] - 20


def test_the_hmc_scenario_ends_a_share_of_its_chains_at_minus_inf():
    from oracle import sampling
    s = poison.HMC
    prob = poison.poisoned_problem(s["name"])
    fg = poison.oracle_grad_fn(prob, s["T"])
    x0, p0, u, mass = poison.hmc_start()
    l0, g0 = fg(x0)
    assert np.all(np.isfinite(l0)) and np.all(np.isfinite(g0))
    det = {}
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xn, ln, gn, acc = sampling.hmc_batched_step(fg, x0, l0, g0, mass, s["nleap"], s["eps"], p0, u, details=det)
    share = float(np.mean(det["lnp_new"] == -np.inf))
    print("hmc scenario: %.0f %% of the chains end at -inf, %d of %d accepted" % (100 * share, acc.sum(), s["B"]))
    assert 0.10 <= share <= 0.60, share
    assert not np.any(acc & ~np.isfinite(det["lnp_new"]))
    assert np.all(np.isfinite(ln)) and np.all(np.isfinite(xn)) and np.all(np.isfinite(gn))
    assert 5 <= acc.sum() < s["B"]


@pytest.mark.parametrize("k", range(len(poison.SLICE)))
def test_the_slice_scenarios_evaluate_rejected_points(k):
    """The oracle's own chain (the ensemble's splits, zeus' move at mu = 1) from the replay's start: at least 50 of its
    evaluations come out -inf, no walker ever sits on one."""
    from oracle import sampling
    s = poison.SLICE[k]
    prob = poison.poisoned_problem(s["name"])
    cnt = {}
    f = poison.oracle_fn(prob, s["T"], counter=cnt)
    nd = prob["nin"]
    coords = poison.slice_start(s["nw"], nd)
    logp = f(coords)
    assert np.all(np.isfinite(logp))
    cnt.clear()
    lib_seed = (s["seed"] + poison.GOLDEN) & 0xFFFFFFFFFFFFFFFF
    worst_exp = worst_con = 0
    for it, halves in enumerate(poison.ensemble_splits(s["seed"], s["nw"], s["iters"])):
        traces = []
        coords, logp, nexp, ncon = sampling.slice_iteration(coords, logp, halves, poison.SLICE_MU, lib_seed, it, f, traces=traces)
        assert np.all(np.isfinite(logp)) and np.all(1.0 + coords[:, 0] > 0)
        worst_exp = max([worst_exp] + [int(t["nexp"].max()) for t in traces])
        worst_con = max([worst_con] + [int(t["ncon"].max()) for t in traces])
    print("slice scenario %s: %d of %d evaluations -inf; at most %d stepping-out steps and %d contractions per walker" % (
        s["name"], cnt["ninf"], cnt["n"], worst_exp, worst_con))
    assert cnt["ninf"] >= 50, cnt
    # the rounds of the one-call half step the GPU test runs hold every walker's update (poison.SLICE_SCHEDULE)
    m_sched, nt_sched = poison.SLICE_SCHEDULE
    assert worst_exp <= m_sched[0] and worst_con < sum(nt_sched)


@pytest.mark.parametrize("ndim", [7, 70])
def test_numpy_rejects_every_nan_energy_row_of_the_acceptance_table(ndim):
    t = poison.hmc_table(ndim)
    want = poison.hmc_table_expected(t)
    #                      accept reject -inf   NaN    NaN P  inf P  H0 NaN H0 inf Gnew   accept reject
    expected = np.array([True, False, False, False, False, False, False, True, True, True, False])
    assert len(t["what"]) == len(expected) == 11
    np.testing.assert_array_equal(want, expected, err_msg=str(t["what"]))
    f = np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        H1 = f(0.5) * np.sum(t["P"] * t["P"] / t["mass"][None, :], -1, dtype=f) - t["lnp_new"]
        dH = t["H0"] - H1
        ratio = np.exp(np.minimum(dH, f(0)))
    assert np.isnan(dH[[3, 4, 6]]).all() and np.isnan(ratio[[3, 4, 6]]).all()          # np.minimum keeps the NaN ...
    assert np.isfinite(t["lnp_new"][[4, 6]]).all() and not want[[4, 6]].any()          # ... and u < NaN rejects a FINITE proposal
    assert dH[7] == np.inf and ratio[7] == 1.0 and dH[5] == -np.inf and ratio[5] == 0.0
    # away from every knife edge: the decision does not depend on rounding of the energies
    ok = np.isfinite(ratio)
    assert np.all(np.abs(ratio[ok] - t["U"][ok]) > 0.05)
