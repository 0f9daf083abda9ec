"""CPU: ``sampler.rank_rhat`` (numpy float64: average ranks by argsort, Phi^-1 by Wichura's AS 241) against the restatement of
the definition with scipy's ``rankdata`` and ``ndtri`` (tests/rank_rhat_emul.py), the condition the GPU test of the stopping
rule rests on, and the C entries' declarations.

Tolerance 1e-12: both sides rank exactly; they differ in Phi^-1 (AS 241 against cephes, both good to a few 1e-16) and in the
order of float64 sums over at most a few thousand scores of magnitude <= 5."""
import os
import re

import numpy as np
import pytest

import chain_exact as ce
import csrc_text
import rank_rhat_emul as emul
import rhat_emul

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(x):
    from linna_amd import sampler
    ref, _ = emul.rank_rhat(x)
    got = np.stack(sampler.rank_rhat(x), axis=1)
    assert np.array_equal(np.isnan(got), np.isnan(ref[:, :3]))
    np.testing.assert_allclose(got, ref[:, :3], rtol=1e-12)
    return ref


@pytest.mark.parametrize("nw,nt", [(1, 40), (3, 101), (24, 300)])
def test_rank_rhat_equals_the_restatement_on_ar1_chains(nw, nt):
    x = rhat_emul.ar1(nt, nw, [0.5, 0.9, 0.97], seed=nw, mean=np.array([0.0, 30.0, -7.0]), scale=np.array([1.0, 1e-2, 3.0]))
    ref = _check(x.astype(np.float32))
    assert np.all(np.isfinite(ref))


@pytest.mark.parametrize("nw", [1, 65])
def test_rank_rhat_on_exact_integer_chains_with_ties_and_a_constant_parameter(nw):
    """The integer chains of chain_exact: values OFFSET + round(8 z), a few dozen distinct values among thousands (ties are
    the rule); the constant parameter gives NaN, the others do not."""
    x = ce.rhat_chain(nw)[:301].transpose(0, 2, 1).astype(np.float32)            # [rows][nw][nd]
    assert len(np.unique(x[:, :, 0])) < x[:, :, 0].size // 4
    ref = _check(x)
    const = [i for i, p in enumerate(ce.RHAT_PARAMS) if p[0] == "const"]
    assert const and np.all(np.isnan(ref[const, :3]))
    assert np.all(np.isfinite(np.delete(ref[:, :3], const, axis=0)))


def test_bulk_rhat_does_not_see_a_monotone_map():
    """x and 8 x + 0 have the same ranks (a power of two: no new ties in float32): the bulk R-hat is bit-equal."""
    from linna_amd import sampler
    x = rhat_emul.ar1(200, 16, [0.3, 0.8], seed=4).astype(np.float32)
    a, b = sampler.rank_rhat(x), sampler.rank_rhat(np.float32(8.0) * x + np.float32(0.0))
    assert np.array_equal(a[1], b[1]) and np.all(np.isfinite(a[1]))
    assert np.array_equal(a[2], b[2])                                             # (and so is the fold: |8 x - 8 med| = 8 |x - med|)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_chains_of_another_scale_pass_plain_rhat_and_fail_the_folded_one(seed):
    """64 chains of 400 rows N(0, 1), the first three 3 x too wide: plain split-R-hat < 1.005 (measured <= 0.9998), the tail
    R-hat > 1.03 (measured >= 1.0405); the same chains unscaled pass both."""
    from linna_amd import sampler
    x, y = emul.wide_chains(seed)
    plain = sampler.split_rhat(y.astype(np.float64))
    rhat, bulk, tail = sampler.rank_rhat(y)
    print("  seed %d: plain %.4f bulk %.4f tail %.4f" % (seed, plain[0], bulk[0], tail[0]))
    assert plain[0] < 1.005 and bulk[0] < 1.005 and tail[0] > 1.03 and rhat[0] == tail[0]
    ref, _ = emul.rank_rhat(y)
    np.testing.assert_allclose([rhat[0], bulk[0], tail[0]], ref[0, :3], rtol=1e-12)
    assert np.all(np.asarray(sampler.rank_rhat(x)) < 1.01)


def test_nan_and_short_windows():
    from linna_amd import sampler
    x = rhat_emul.ar1(60, 5, [0.3, 0.5], seed=9).astype(np.float32)
    y = x.copy()
    y[7, 2, 1] = np.inf
    a, b = sampler.rank_rhat(x), sampler.rank_rhat(y)
    assert np.all(np.isnan([v[1] for v in b])) and all(u[0] == v[0] for u, v in zip(a, b))
    z = np.concatenate([x[:30], np.full((1, 5, 2), np.nan, np.float32), x[30:]])      # the middle row of an odd window
    assert all(np.array_equal(u, v) for u, v in zip(a, sampler.rank_rhat(z)))
    with pytest.raises(ValueError):
        sampler.rank_rhat(x[:3])


def test_the_entries_are_declared_guarded_and_bound():
    from linna_amd import _lib
    header = open(os.path.join(ROOT, "include", "linna_hip.h")).read()
    api = csrc_text.hip_sources()
    for name, nargs in (("linna_chain_rank_rhat_scratch_bytes", 4), ("linna_chain_rank_rhat", 12)):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert re.search(r"^(?:int|size_t) %s\(([^{;]*)\) try \{" % name, api, flags=re.M), name
        assert name in _lib.EXPORTED and len(_lib._SIGNATURES[name][1]) == nargs
    assert _lib.ABI_VERSION == 12 and re.search(r"#define\s+LINNA_ABI_VERSION\s+12\b", header)
    assert "chain_rank.hip" in __import__("linna_amd._build", fromlist=["SOURCES"]).SOURCES


def test_refusals_need_no_gpu():
    """The entry checks its arguments before anything touches the device: two halves of at least 2 rows, walkers within the
    lanes, scratch for one parameter (LINNA_ERR_INVALID), fewer than 2^31 pooled values (LINNA_ERR_UNSUPPORTED, with a text
    that says so).  The pointers are never followed."""
    from linna_amd import _lib
    lib = _lib.load()
    fake = 4096
    one = lib.linna_chain_rank_rhat_scratch_bytes(3, 65, 8, 1)
    assert one > 16 * 8 * 65 and lib.linna_chain_rank_rhat_scratch_bytes(3, 65, 8, 3) == 3 * one
    assert lib.linna_chain_rank_rhat_scratch_bytes(3, 65, 8, 7) == 3 * one          # (never more rounds' worth than parameters)
    assert lib.linna_chain_rank_rhat_scratch_bytes(3, 65, 7, 1) == 0 and lib.linna_chain_rank_rhat_scratch_bytes(3, 65, 8, 0) == 0
    call = lambda nwp, nw, lo, hi, nbytes: lib.linna_chain_rank_rhat(None, fake, 3, nwp, nw, lo, hi, fake, nbytes, None, fake, None)
    assert call(128, 65, 5, 8, one) == _lib.ERR_INVALID
    assert call(64, 65, 0, 8, one) == _lib.ERR_INVALID
    assert call(128, 65, 0, 8, one - 1) == _lib.ERR_INVALID and "scratch" in lib.linna_last_error().decode()
    assert call(4096, 4096, 0, 1 << 20, 1 << 40) == _lib.ERR_UNSUPPORTED and "2^31" in lib.linna_last_error().decode()
