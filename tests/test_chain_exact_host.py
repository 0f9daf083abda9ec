"""CPU: pins tests/chain_exact.py -- the exact integer chains and the references tests/test_gpu_chain_stats.py holds the
chain-statistics kernels (csrc/autocorr.hip) to.

 * exactness: every chain meets N A^2 < 2^53 (and the int64 condition of the integer numerators), asserted with the magnitudes;
 * the references agree with what the project already trusts, at the existing 1e-9: ``tau_ref`` with
   oracle.sampling.integrated_time, ``rhat_ref`` and ``ess_ref`` with tests/rhat_emul.py, ``meanstd_ref`` with
   oracle.sampling.checkmeanstd_stats; the integer references with a second, slower statement of the definition;
 * conditions on the inputs: the derived error bound of every GPU case stays below that 1e-9 bar, and every discrete decision
   of the reference (the window and status of tau, the last pair and status of the ESS, NaN versus finite of R-hat) has a
   positive margin -- no case excused.
"""
import numpy as np
import pytest

import chain_exact as ce
import rhat_emul
from oracle import sampling

BAR = ce.BAR


def window_f64(case):
    x = ce.tau_case_chain(case)
    _, _, _, _, _, nlive, lo, hi, _ = case
    return x[lo:hi, :, :nlive].transpose(0, 2, 1).astype(np.float64)          # [N][walker][parameter], as the oracle takes it


# ----------------------------------------------------------------------------------------------- exactness
def test_every_chain_meets_the_exactness_condition():
    seen = set()
    for case in ce.TAU_CASES:
        x = ce.tau_case_chain(case)
        if id(x) in seen:
            continue
        seen.add(id(x))
        nmax = max(c[7] - c[6] for c in ce.TAU_CASES if ce.tau_case_chain(c) is x)
        assert ce.exact_ok(x, len(x)) and ce.numerators_ok(x, nmax, x.shape[2]), (case[0], ce.amplitude(x))
        assert ce.amplitude(x) >= 1 and int(np.abs(x).max()) < 2 ** 24
    nmax = max((w[2] - w[1]) // 2 for w in ce.RHAT_WINDOWS)
    for x, nmax in ((ce.rhat_chain(ce.RHAT_NWP), nmax), (ce.meanstd_chain(), ce.MEANSTD_ROWS)):
        assert ce.exact_ok(x, len(x)) and ce.numerators_ok(x, nmax, 2 * x.shape[2]), ce.amplitude(x)
        assert int(np.abs(x).max()) < 2 ** 24
    # the large offset is there and the reference point removes it: the same chain without x[0] taken out would not be exact at 2^24
    x = ce.tau_case_chain(ce.TAU_CASES[0])
    assert int(np.abs(x).min()) > 100 * ce.amplitude(x)
    # a float64 accumulation of the products in a scrambled order gives the integer sums bit for bit
    y = ce.rel0(x)[3:643].astype(np.float64)
    S, T = ce.sums_ref(x, 3, 643, 40)
    perm = ce.rng("perm").permutation(640 - 39)
    got = np.zeros(x.shape[1:])
    for t in perm:
        got += y[t + 39] * y[t]
    assert np.array_equal(got, S[39].astype(np.float64)) and np.array_equal(y.sum(axis=0), T.astype(np.float64))


def test_chains_are_pure_functions_of_their_key():
    a, b = ce.chain("k", 40, 5, ce.TAU_PARAMS), ce.chain("k", 40, 5, ce.TAU_PARAMS)
    assert np.array_equal(a, b) and not np.array_equal(a, ce.chain("k2", 40, 5, ce.TAU_PARAMS))
    assert np.all(a[:, 1] == a[0, 1, 0])                                      # the constant series
    ct = ce.ct_image(a, 64, np.nan, rows=41)
    assert ct.shape == (41, 4, 64) and np.isnan(ct[:, :, 5:]).all() and np.isnan(ct[40]).all()
    assert np.isnan(ce.with_nan_row(ct, 3, 2)[3, 2]).all() and not np.isnan(ct[3, 2, :5]).any()


# ----------------------------------------------------------------------------------------------- integer references
def test_integer_references_against_a_second_statement():
    x = ce.chain("ints", 300, 3, (("ar", 0.8), ("const",)))
    y = ce.rel0(x)
    S, T = ce.sums_ref(x, 7, 50, 64)
    for k in (0, 1, 5, 42, 43, 63):
        want = sum(y[t] * y[t - k] for t in range(7 + k, 50))
        assert np.array_equal(S[k], want if k < 43 else np.zeros_like(S[k]))
    assert np.array_equal(T, sum(y[t] for t in range(7, 50)))
    M = ce.moments_ref(x, 1, 2)
    assert np.array_equal(M[0, 0], y[128:256].sum(0)) and np.array_equal(M[0, 1], (y[128:256] ** 2).sum(0))
    # the lane permutation: every wstride-th walker first
    blk = np.arange(2 * 7 * 4, dtype=np.float32).reshape(2, 7, 4)
    out = ce.append_ref(blk, 7, 3, 3, 64)
    assert ce.lane_order(7, 3) == [0, 3, 6, 1, 2, 4, 5] and ce.lane_order(4, 1) == [0, 1, 2, 3] and ce.lane_order(3, 8) == [0, 1, 2]
    for lane, w in enumerate(ce.lane_order(7, 3)):
        assert np.array_equal(out[:, :, lane], blk[:, w, :3])
    assert out.shape == (2, 3, 64) and not out[:, :, 7:].any()


# ----------------------------------------------------------------------------------------------- tau and ESS
@pytest.mark.parametrize("case", ce.TAU_CASES, ids=[c[0] for c in ce.TAU_CASES])
def test_tau_and_ess_references_and_the_conditions_on_their_cases(case):
    tau, ess = ce.tau_case_refs(case)
    _, params, _, _, _, nlive, lo, hi, kuse = case
    n = hi - lo
    w = window_f64(case)
    live = [d for d, p in enumerate(params) if p[0] != "const"]
    assert len(live) < len(params) or params == ce.ALT_PARAMS
    # ---- conditions: bounds below the bar, margins positive
    for d in range(len(params)):
        if d in live:
            assert tau["bound"][d] <= BAR * abs(tau["tau"][d]) and tau["margin"][d] > 0, (d, tau)
            assert ess["bound"][d] <= BAR * abs(ess["ess"][d]) and ess["margin"][d] > 0, (d, ess)
        else:
            assert np.isnan(tau["tau"][d]) and tau["window"][d] == 0 and tau["status"][d] == 0
            assert np.isnan(ess["ess"][d]) and ess["last"][d] == -1 and ess["status"][d] == 0
    # ---- agreement with the oracle / the emulation where they compute the same thing: every lag of the window available
    with np.errstate(invalid="ignore", divide="ignore"):
        want = sampling.integrated_time(w)
    for d in live:
        if tau["status"][d] == 0:
            np.testing.assert_allclose(tau["tau"][d], want[d], rtol=BAR)
        else:
            assert kuse < n - 1 and tau["window"][d] == kuse
    if kuse == n - 1:
        assert not tau["status"].any() and not ess["status"].any()
    want_ess, want_last = rhat_emul.multichain_ess(w)
    for d in live:
        if ess["status"][d] == 0:                                 # the sequence ended within the lags given
            np.testing.assert_allclose(ess["ess"][d], want_ess[d], rtol=BAR)
            assert ess["last"][d] == want_last[d]


def test_the_case_list_reaches_every_decision():
    """What the GPU module's docstring promises of the cases: both statuses, windows past 256 lags, an unpaired last lag, the
    floored tau with no pair, one chain."""
    refs = [ce.tau_case_refs(c) for c in ce.TAU_CASES]
    assert any(t["status"].any() for t, _ in refs) and any(e["status"].any() for _, e in refs)
    assert any(np.nanmax(t["window"]) > 256 for t, _ in refs)
    assert any(c[8] % 2 == 0 and e["status"].any() and np.max(e["last"]) == c[8] // 2 - 1 for c, (_, e) in zip(ce.TAU_CASES, refs))
    alt = [e for c, (_, e) in zip(ce.TAU_CASES, refs) if c[1] == ce.ALT_PARAMS]
    assert alt and all(e["last"][0] == -1 and e["status"][0] == 0 and np.isfinite(e["ess"][0]) for e in alt)
    c = next(c for c in ce.TAU_CASES if c[1] == ce.ALT_PARAMS)
    assert alt[0]["ess"][0] == pytest.approx(c[5] * 40 * np.log10(c[5] * 40), rel=1e-12)      # ESS = nl N / (1 / log10(nl N))


# ----------------------------------------------------------------------------------------------- split-R-hat
@pytest.mark.parametrize("win", ce.RHAT_WINDOWS, ids=[w[0] for w in ce.RHAT_WINDOWS])
@pytest.mark.parametrize("nw", ce.RHAT_NW)
def test_rhat_reference_and_the_conditions_on_its_cases(win, nw):
    _, lo, hi, _, nanrow = win
    xf = ce.rhat_image(nw, nanrow)
    out, bound, margin = ce.rhat_ref(xf, lo, hi, ce.RHAT_NWP)
    n = (hi - lo) // 2
    dropped = (hi - lo) % 2 == 1 and nanrow == lo + n
    with np.errstate(invalid="ignore"):
        want = rhat_emul.split_rhat(xf[lo:hi].transpose(0, 2, 1))
    for d, p in enumerate(ce.RHAT_PARAMS):
        if p[0] == "const":
            assert np.isnan(out[d, 0]) and out[d, 1] == 0 and out[d, 2] == 0 and out[d, 3] == ce.OFFSET + 3
            assert np.isnan(want[d, 0]) and np.array_equal(bound[d, 1:3], [0, 0])
        elif d == 3 and not dropped:
            assert np.isnan(out[d, 0]) and np.isnan(want[d, 0])
        else:
            np.testing.assert_allclose(out[d], want[d], rtol=BAR)
            assert np.all(bound[d] <= BAR * np.abs(out[d])) and margin[d] > 0, (d, out[d], bound[d], margin[d])
    assert np.isfinite(out[3, 0]) == dropped


# ----------------------------------------------------------------------------------------------- checkmeanstd's moments
@pytest.mark.parametrize("case", ce.MEANSTD_CASES, ids=lambda c: "%s" % (c,))
def test_meanstd_reference_and_the_conditions_on_its_cases(case):
    (t0, tm, t1), nws = case
    x = ce.meanstd_chain()
    out, bound = ce.meanstd_ref(x, nws, t0, tm, t1)
    for h, (r0, r1) in enumerate(((t0, tm), (tm, t1))):
        if r1 == r0:
            assert np.isnan(out[:, h]).all()
            continue
        blk = x[r0:r1, :, :nws].astype(np.float64)
        np.testing.assert_allclose(out[:, h, 0], blk.mean(axis=(0, 2)), rtol=BAR)
        np.testing.assert_allclose(out[:, h, 1], blk.std(axis=(0, 2)), rtol=BAR, atol=1e-12)
        # the existing bar of the checkmeanstd comparison (tests/test_gpu_autocorr.py): rtol 1e-9, atol 1e-12
        assert np.all(bound[:, h] <= BAR * np.abs(out[:, h]) + 1e-12), (out[:, h], bound[:, h])
        assert np.all(out[:, h, 1] > 0)
    if tm - t0 == (t1 - t0) // 2 and tm > t0:                      # the split checkmeanstd makes: the oracle's two numbers
        a, b = sampling.checkmeanstd_stats(x[t0:t1, :, :nws].transpose(0, 2, 1).astype(np.float64))
        ga = np.median(np.abs(out[:, 0, 0] - out[:, 1, 0]) / out[:, 1, 1])
        gb = np.median((out[:, 0, 1] - out[:, 1, 1]) / out[:, 1, 1])
        np.testing.assert_allclose([ga, gb], [a, b], rtol=BAR, atol=1e-12)
