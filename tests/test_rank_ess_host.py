"""CPU: ``sampler.rank_ess`` (numpy float64: average ranks by argsort, Phi^-1 by Wichura's AS 241, autocovariances by FFT)
against the restatement of the definition (tests/rank_ess_emul.py: scipy's ``rankdata`` and ``ndtri``, lagged products as
plain sums, a Geyer loop of its own), what the statistic is for (sticky tails, heavy tails, monotone maps), the quantile's
integer position arithmetic and the C entries' declarations.

Tolerance ``chain_exact.BAR`` = 1e-9, the project's bar for chain statistics.  The discrete outputs (last pairs) are compared
where the restatement's margin -- the smallest |P_t| up to the pair that ends Geyer's sequence -- is above 1e-6; every case
here has every series above it (asserted: a case that cannot meet it gets another seed)."""
import os
import re

import numpy as np
import pytest

import chain_exact as ce
import csrc_text
import rank_ess_emul as emul
import rhat_emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(x):
    from linna_amd import sampler
    ref, margin = emul.rank_ess(x)
    assert np.all(margin > emul.MARGIN), margin
    bulk, tail, e05, e95, last = sampler.rank_ess(x, return_all=True)
    got = np.stack([bulk, tail, e05, e95], axis=1)
    assert np.array_equal(np.isnan(got), np.isnan(ref[:, :4])), (got, ref)
    np.testing.assert_allclose(got, ref[:, :4], rtol=ce.BAR)
    assert np.array_equal(last, ref[:, 4:7]) and np.all(ref[:, 7] == 0)
    b2, t2 = sampler.rank_ess(x)
    assert np.array_equal(b2, bulk, equal_nan=True) and np.array_equal(t2, tail, equal_nan=True)
    return ref


@pytest.mark.parametrize("nw,nt", [(1, 40), (3, 101), (24, 300)])
def test_rank_ess_equals_the_restatement_on_ar1_chains(nw, nt):
    x = rhat_emul.ar1(nt, nw, [0.5, 0.9, 0.97], seed=nw, mean=np.array([0.0, 30.0, -7.0]), scale=np.array([1.0, 1e-2, 3.0]))
    ref = _check(x.astype(np.float32))
    assert np.all(np.isfinite(ref))


def test_iid_chains_agree_in_all_three():
    """On iid chains bulk-ESS, tail-ESS and the raw ESS agree within 5 %: the confirmation costs converged runs nothing in
    verdict."""
    from linna_amd import sampler
    x = np.random.RandomState(3).standard_normal((400, 64, 1)).astype(np.float32)
    bulk, tail = sampler.rank_ess(x)
    raw = sampler.multichain_ess(x.astype(np.float64))
    print("  iid: raw %.0f bulk %.0f tail %.0f" % (raw[0], bulk[0], tail[0]))
    assert abs(bulk[0] / raw[0] - 1) < 0.05 and abs(tail[0] / raw[0] - 1) < 0.05


def test_a_sticky_upper_tail_passes_the_raw_ess_and_fails_the_tail_ess():
    """64 chains of 1000 rows N(0, 1) in which a value above 1.8 stays with probability 0.98: raw ESS >= 1000 > tail-ESS, and
    the 5 % quantile's ESS is more than 10 x the 95 % quantile's."""
    from linna_amd import sampler
    x = emul.sticky_tail(1)
    raw = sampler.multichain_ess(x.astype(np.float64))[0]
    bulk, tail, e05, e95, last = sampler.rank_ess(x, return_all=True)
    print("  sticky: raw %.0f bulk %.0f tail %.0f q05 %.0f q95 %.0f last pairs %s" % (raw, bulk[0], tail[0], e05[0], e95[0], last[0]))
    assert raw >= 1000 > tail[0] and e05[0] > 10 * e95[0] and tail[0] == e95[0]
    _check(x)


def test_cauchy_chains_have_a_finite_bulk_ess():
    """No variance, no mean: the raw ESS is meaningless; the normal scores of iid draws are iid whatever the law."""
    from linna_amd import sampler
    x = np.random.RandomState(5).standard_cauchy((400, 32, 1)).astype(np.float32)
    bulk, tail = sampler.rank_ess(x)
    assert np.isfinite(bulk[0]) and abs(bulk[0] / (2 * 32 * 200) - 1) < 0.05


def test_bulk_ess_does_not_see_a_monotone_map():
    """x and exp(x) have the same ranks (values far enough apart that float32 exp adds no ties: asserted): bit-equal."""
    from linna_amd import sampler
    x = rhat_emul.ar1(200, 16, [0.3, 0.8], seed=4).astype(np.float32)
    y = np.exp(x.astype(np.float64)).astype(np.float32)
    for d in range(2):
        assert np.array_equal(np.argsort(x[:, :, d], axis=None, kind="stable"), np.argsort(y[:, :, d], axis=None, kind="stable"))
    a, b = sampler.rank_ess(x, return_all=True), sampler.rank_ess(y, return_all=True)
    assert np.array_equal(a[0], b[0]) and np.all(np.isfinite(a[0]))
    assert np.array_equal(a[1], b[1])                                             # (the indicators of a quantile are the same sets)


def test_nan_and_short_windows():
    from linna_amd import sampler
    x = rhat_emul.ar1(60, 5, [0.3, 0.5], seed=9).astype(np.float32)
    y = x.copy()
    y[7, 2, 1] = np.inf
    a, b = sampler.rank_ess(x, return_all=True), sampler.rank_ess(y, return_all=True)
    assert all(np.isnan(v[1]) for v in b[:4]) and np.all(b[4][1] == -1)
    assert all(u[0] == v[0] for u, v in zip(a[:4], b[:4])) and np.array_equal(a[4][0], b[4][0])
    z = np.concatenate([x[:30], np.full((1, 5, 2), np.nan, np.float32), x[30:]])      # the middle row of an odd window
    assert all(np.array_equal(u, v) for u, v in zip(a, sampler.rank_ess(z, return_all=True)))
    c = x.copy()
    c[:, :, 0] = 2.5                                                                  # constant: every series without variance
    bulk, tail, e05, e95, last = sampler.rank_ess(c, return_all=True)
    assert np.isnan([bulk[0], tail[0], e05[0], e95[0]]).all() and np.all(last[0] == -1) and bulk[1] == a[0][1]
    _check(c)
    _check(x[:4])                                                                     # two rows a half: one pair
    with pytest.raises(ValueError):
        sampler.rank_ess(x[:3])


def test_ties_that_straddle_a_quantile():
    """Integer chains (a few dozen distinct values): the run of values equal to s_j holds the quantile's position, and every
    one of them is on the quantile's side (x <= q).  The indicator sums are integers: both sides agree to rounding."""
    x = ce.rhat_chain(5)[:301].transpose(0, 2, 1).astype(np.float32)
    for d in (0, 2, 3):
        v = emul.pooled(x)[:, :, d].reshape(-1)
        s = np.sort(v)
        for num in (1, 19):
            j = num * (len(v) - 1) // 20
            assert s[j - 1] == s[j] == s[j + 1], "no tie at the quantile"
    ref = _check(x)
    const = [i for i, p in enumerate(ce.RHAT_PARAMS) if p[0] == "const"]
    assert const and np.all(np.isnan(ref[const, :4])) and np.all(np.isfinite(np.delete(ref[:, :4], const, axis=0)))


@pytest.mark.parametrize("S1", [99, 1339, 101, 1301, 1305])
def test_quantile_positions_are_integers(S1):
    """The position arithmetic at its edges.  S = 2 n nw is even, so S - 1 is odd and neither S - 1 nor 19 (S - 1) is ever a
    multiple of 20: g = 0 cannot occur through this statistic, and the remainders are odd.  The edges that can: S - 1 = 19
    mod 20 (99, 1339: the remainders 19 and 1), S - 1 = 1 mod 20 (101, 1301: 1 and 19), and 1305 (5 and 15).  The values are
    the integers 0 .. S - 1 in a shuffled order: q lies strictly between j and j + 1 and I_p has exactly j + 1 ones."""
    S = S1 + 1
    v = np.random.RandomState(S).permutation(S).astype(np.float32)
    y = emul.series(v, S // 2, 1)
    for t, num in ((1, 1), (2, 19)):
        j, rem = divmod(num * S1, 20)
        assert rem % 2 == 1 and rem == {99: (19, 1), 1339: (19, 1), 101: (1, 19), 1301: (1, 19), 1305: (5, 15)}[S1][t - 1]
        assert int(y[t].sum()) == j + 1
    _check(v.reshape(S, 1, 1))


def test_the_entries_are_declared_guarded_and_bound():
    from linna_amd import _lib, sampler
    header = open(os.path.join(ROOT, "include", "linna_hip.h")).read()
    api = csrc_text.hip_sources()
    for name, nargs in (("linna_chain_rank_ess_scratch_bytes", 5), ("linna_chain_rank_ess", 12)):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert re.search(r"^(?:int|size_t) %s\(([^{;]*)\) try \{" % name, api, flags=re.M), name
        assert name in _lib.EXPORTED and len(_lib._SIGNATURES[name][1]) == nargs
    assert _lib.ABI_VERSION == 12 and re.search(r"#define\s+LINNA_ABI_VERSION\s+12\b", header)
    assert sampler.rank_ess is __import__("linna_amd.chainstats", fromlist=["rank_ess"]).rank_ess and "rank_ess" not in sampler.__all__


def test_refusals_need_no_gpu():
    """``ess_rank`` without ``criterion="rhat"`` raises before anything is built; the entry checks its arguments before anything
    touches the device (the pointers are never followed)."""
    from linna_amd import _lib, sampler, util
    with pytest.raises(ValueError, match="ess_rank"):
        sampler.HMCSampler._check(None, "hmc", 0, 10, False, False, 64, "tau", 1.01, 400, 0.0, False, True)
    with pytest.raises(ValueError, match="ess_rank"):
        sampler.HMCSampler(None, None, None, 2, 4).sample(None, 10, method="hmc", ess_rank=True)
    with pytest.raises(ValueError, match="ess_rank"):
        util.run_mcmc(None, ".", "hmc", 2, 4, None, None, ess_rank=True)
    lib = _lib.load()
    fake = 4096
    size = lib.linna_chain_rank_ess_scratch_bytes
    one = size(3, 65, 8, 3, 1)
    assert one > 16 * 8 * 65 and size(3, 65, 8, 3, 3) == 3 * one and size(3, 65, 8, 3, 7) == 3 * one
    assert size(3, 65, 7, 3, 1) == 0 and size(3, 65, 8, 3, 0) == 0 and size(3, 65, 8, 0, 1) == 0 and size(3, 65, 8, 4, 1) == 0
    assert size(3, 65, 2, 1, 1) == 0 and size(3, 4096, 1 << 20, 31, 1) == 0         # (n < 2; S >= 2^31)
    assert size(3, 65, 200, 31, 1) < size(3, 65, 200, 32, 1)                         # (lags come in blocks of 32)
    call = lambda nwp, nw, lo, hi, kuse, nbytes: lib.linna_chain_rank_ess(None, fake, 3, nwp, nw, lo, hi, kuse, fake, nbytes, fake, None)
    for args in ((128, 65, 5, 8, 1, one), (64, 65, 0, 8, 3, one), (128, 65, 0, 8, 0, one), (128, 65, 0, 8, 4, one)):
        assert call(*args) == _lib.ERR_INVALID and "chain_rank_ess" in lib.linna_last_error().decode(), args
    assert call(128, 65, 0, 8, 3, one - 1) == _lib.ERR_INVALID and "scratch" in lib.linna_last_error().decode()
    assert call(4096, 4096, 0, 1 << 20, 31, 1 << 40) == _lib.ERR_UNSUPPORTED and "2^31" in lib.linna_last_error().decode()
