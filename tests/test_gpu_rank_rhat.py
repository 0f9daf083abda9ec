"""GPU: the rank-normalised, folded split-R-hat (csrc/chain_rank.hip through ``linna_chain_rank_rhat`` with ``rank2_out``)
against the restatement of the definition (tests/rank_rhat_emul.py: scipy's ``rankdata`` and ``ndtri``), then
``DeviceChain.rank_rhat`` and ``rhat_rank=True`` through the driver.

Ranks are integers and must agree EXACTLY (``rank2_out`` = 2 x the average rank, bulk and folded; padded lanes 0).  The R-hats
are held to ``chain_exact.BAR`` = 1e-9, the project's bar for chain statistics: with equal ranks the device and the
restatement differ only in Phi^-1 (Wichura's AS 241 by hand against cephes, both good to a few 1e-16) and in the order of
float64 sums of scores of magnitude <= 5.  Measured on MI355X: largest relative difference over all cases 5.6e-16.  The
median is the same two float64 operations on both sides: bit-equal.

Padded lanes and the rows outside the window hold -1e30: it would move every rank if it entered.  The sort's tile is 4096
elements (256 threads x 16 chunks): S = 4094, 4096, 4098 are the sizes around one tile (S is even), S = 130 000 takes 32
workgroups a pass."""
import contextlib
import ctypes
import io
import os

import numpy as np
import pytest

import chain_exact as ce
import rank_rhat_emul as emul
import rhat_emul
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = np.float32(-1e30)
TINY = np.finfo(np.float32).tiny
WORST = [0.0]


def _run(x, lo, hi, nwp=None, rows_after=2, npar=None, short=0):
    """x[N, nw, nd] float32 -> (rc, out[nd, 4], rank2[2, nd, 2 n, nwp]) of the window [lo, hi) of the image CT[lo + N + rows_after]
    [nd][nwp] whose rows [lo, lo + N) hold x and everything else the sentinel."""
    N, nw, nd = x.shape
    assert hi - lo == N
    nwp = (nw + 63) & ~63 if nwp is None else nwp
    ct = np.full((lo + N + rows_after, nd, nwp), SENTINEL, np.float32)
    ct[lo:hi, :, :min(nw, nwp)] = x.transpose(0, 2, 1)[:, :, :nwp]
    n = N // 2
    lib = _lib.load()
    need = int(lib.linna_chain_rank_rhat_scratch_bytes(nd, nw, 2 * n, nd if npar is None else npar)) if n >= 2 and nw <= nwp else 4096
    dct = torch.as_tensor(ct, device="cuda")
    scratch = torch.empty(max(need - short, 8), dtype=torch.uint8, device="cuda")
    r2 = torch.full((2, nd, max(2 * n, 1), nwp), -7, dtype=torch.int32, device="cuda")
    out = torch.full((nd, 4), -7.0, dtype=torch.float64, device="cuda")
    rc = lib.linna_chain_rank_rhat(_lib.ctx(), _lib.ptr(dct), nd, nwp, nw, lo, hi, _lib.ptr(scratch, torch.uint8), need - short,
                                   _lib.ptr(r2, torch.int32), _lib.ptr(out, torch.float64), _lib.stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), r2.cpu().numpy()


def _check(x, lo=0, odd_nan=False, **kw):
    """The window holding x (with ``odd_nan``: an odd window whose dropped middle row is NaN) against the restatement: ranks
    exactly, padded lanes 0, R-hats to 1e-9 with the same NaNs, the median bit for bit, a second call the same bits."""
    x = np.asarray(x, np.float32)
    if odd_nan:
        n = len(x) // 2
        x = np.concatenate([x[:n], np.full((1,) + x.shape[1:], np.nan, np.float32), x[len(x) - n:]])
    N, nw, nd = x.shape
    ref, (r2b, r2f) = emul.rank_rhat(x)
    for d in range(nd):                                       # the folded input as the definition forms it: no subnormal zeta
        zeta, _ = emul.fold(emul.pooled(x)[:, :, d])
        assert np.all((zeta == 0) | (zeta >= TINY) | ~np.isfinite(zeta))
    rc, out, r2 = _run(x, lo, lo + N, **kw)
    assert rc == 0, _lib.load().linna_last_error().decode()
    fin = np.all(np.isfinite(emul.pooled(x)), axis=(0, 1))
    for d in np.nonzero(fin)[0]:
        assert np.array_equal(r2[0, d, :, :nw], r2b[d]), ("bulk ranks", d)
        assert np.array_equal(r2[1, d, :, :nw], r2f[d]), ("folded ranks", d)
    assert np.all(r2[:, :, :, nw:] == 0)
    assert np.array_equal(np.isnan(out[:, :3]), np.isnan(ref[:, :3])), (out, ref)
    np.testing.assert_allclose(out[:, :3], ref[:, :3], rtol=ce.BAR)
    assert np.array_equal(out[fin, 3], ref[fin, 3])
    with np.errstate(invalid="ignore"):
        if np.any(np.isfinite(ref[:, :3])):
            WORST[0] = max(WORST[0], float(np.nanmax(np.abs(out[:, :3] / ref[:, :3] - 1.0))))
    rc2, out2, r22 = _run(x, lo, lo + N, **kw)
    assert rc2 == 0 and np.array_equal(out, out2, equal_nan=True) and np.array_equal(r2, r22)
    return out, ref


def _mixed(N, nw, seed):
    """Three parameters: AR(1) with a large offset; a chain in which 25 % of the rows repeat their predecessor bit for bit
    (rejected transitions); N(0, 1) with negatives, both zeros, float32 subnormals of both signs and a few exact ties."""
    rs = np.random.RandomState(seed)
    x = np.empty((N, nw, 3), np.float32)
    x[:, :, 0] = rhat_emul.ar1(N, nw, [0.9], seed=seed, mean=30.0, scale=1e-2)[:, :, 0]
    y = rs.standard_normal((N, nw)).astype(np.float32)
    for t in range(1, N):
        rep = rs.random_sample(nw) < 0.25
        y[t, rep] = y[t - 1, rep]
    x[:, :, 1] = y
    v = rs.standard_normal(N * nw).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1e-38, -1e-38, v[0], v[0], -v[0]], np.float32)
    k = min(len(special), max(1, (N * nw) // 4))
    v[rs.permutation(N * nw)[:k]] = special[:k]
    x[:, :, 2] = v.reshape(N, nw)
    return x


@pytest.mark.parametrize("nw", [1, 3, 64, 65, 130])
def test_ranks_and_rhat_on_mixed_values(nw):
    """Every lane count around the wavefront, lo > 0, an even window and an odd one whose dropped middle row is NaN."""
    x = _mixed(100, nw, seed=nw)
    _check(x, lo=7)
    _check(x, lo=3, odd_nan=True)
    print("  nw %d: largest relative difference so far %.3g" % (nw, WORST[0]))


@pytest.mark.parametrize("nw", [1, 65])
def test_two_rows_a_half(nw):
    _check(_mixed(4, nw, seed=40 + nw), lo=3)
    _check(_mixed(4, nw, seed=50 + nw), lo=0, odd_nan=True)


@pytest.mark.parametrize("nw,n", [(1, 2047), (1, 2048), (1, 2049), (64, 32)])
def test_around_one_sort_tile(nw, n):
    """S = 4094, 4096 (one chain and 64 chains), 4098: below one tile, exactly one, one pair more."""
    _check(_mixed(2 * n, nw, seed=n)[:, :, 1:], lo=1)


def test_one_key_repeated_and_all_keys_distinct():
    """Parameter 0: one value S times (every rank S + 1 over 2; NaN for the R-hats).  Parameter 1: a permutation of S distinct
    integers.  Parameter 2: constant within every split chain, different between them (W = 0: NaN)."""
    N, nw = 60, 65
    n = N // 2
    x = np.empty((N, nw, 3), np.float32)
    x[:, :, 0] = -2.5
    x[:, :, 1] = np.random.RandomState(1).permutation(N * nw).reshape(N, nw) - 1000.0
    x[:n, :, 2] = np.arange(nw)
    x[n:, :, 2] = -1.0 - np.arange(nw)
    out, ref = _check(x, lo=2)
    assert np.all(np.isnan(out[[0, 2], :3])) and np.all(np.isfinite(out[1, :3]))
    rc, _, r2 = _run(x, 2, 2 + N)
    assert rc == 0 and np.all(r2[:, 0, :, :nw] == N * nw + 1)


def test_exact_integer_chains():
    """The integer chains of chain_exact (a few dozen distinct values: ties are the rule; one constant parameter)."""
    x = ce.rhat_chain(65)[:301].transpose(0, 2, 1).astype(np.float32)
    out, _ = _check(x, lo=5)
    const = [i for i, p in enumerate(ce.RHAT_PARAMS) if p[0] == "const"]
    assert np.all(np.isnan(out[const, :3])) and np.all(np.isfinite(np.delete(out[:, :3], const, axis=0)))


def test_keys_that_agree_in_three_of_four_digits():
    """The degenerate pass, every element in one bin: parameter 0's keys differ in the lowest byte only, parameter 1's in the
    highest only (both signs)."""
    N, nw = 80, 70
    rs = np.random.RandomState(2)
    low = (np.uint32(0x3F800000) | rs.randint(0, 256, N * nw).astype(np.uint32)).view(np.float32)
    top = ((rs.randint(0x30, 0x50, N * nw).astype(np.uint32) << np.uint32(24)) | np.uint32(0x00123456) |
           (rs.randint(0, 2, N * nw).astype(np.uint32) << np.uint32(31))).view(np.float32)
    _check(np.stack([low.reshape(N, nw), top.reshape(N, nw)], axis=2), lo=1)


def test_many_workgroups_a_pass():
    """S = 130 000: 32 workgroups a pass, 130 chains of 1000 rows; AR(1) and the chain with repeated rows."""
    _check(_mixed(1000, 130, seed=11)[:, :, :2])
    print("  largest relative difference of an R-hat over all cases so far: %.3g" % WORST[0])


def test_a_value_that_is_not_finite_spoils_its_parameter_only():
    x = _mixed(100, 65, seed=21)
    rc, clean, _ = _run(x, 4, 104)
    for bad, row in ((np.nan, 13), (np.inf, 77), (-np.inf, 50)):
        y = x.copy()
        y[row, 9, 1] = bad
        out, _ = _check(y, lo=4)
        assert np.all(np.isnan(out[1, :3])) and np.array_equal(out[[0, 2]], clean[[0, 2]])


def test_parameter_rounds():
    """ndim = 5 with scratch for 1, 2 and 5 parameters a round: the same bits."""
    x = np.concatenate([_mixed(100, 65, seed=31), _mixed(100, 65, seed=32)[:, :, :2]], axis=2)
    got = [_run(x, 6, 106, npar=k) for k in (1, 2, 5)]
    assert all(g[0] == 0 for g in got)
    for g in got[1:]:
        assert np.array_equal(g[1], got[0][1], equal_nan=True) and np.array_equal(g[2], got[0][2])
    ref, (r2b, _) = emul.rank_rhat(x)
    np.testing.assert_allclose(got[0][1][:, :3], ref[:, :3], rtol=ce.BAR)
    assert np.array_equal(got[0][2][0, :, :, :65], r2b)


def test_refusals_launch_nothing():
    x = _mixed(8, 65, seed=3)
    lib = _lib.load()
    for kw, xx, lo, hi in ((dict(), x[:3], 5, 8), (dict(nwp=64), x, 0, 8), (dict(short=1, npar=1), x, 0, 8)):
        rc, out, r2 = _run(xx, lo, hi, **kw)
        assert rc == _lib.ERR_INVALID and "chain_rank_rhat" in lib.linna_last_error().decode(), (kw, rc)
        assert np.all(out == -7.0) and np.all(r2 == -7)
    rc, out, _ = _run(x[:4], 5, 9)
    assert rc == 0 and np.all(out[:, 3] != -7.0)


def test_device_chain_rank_rhat_sees_chains_of_another_scale():
    """64 chains of 400 rows, three of them 3 x too wide: plain R-hat and the ESS pass the rule at 1.01 / 400; the confirmation
    says "not converged".  The same chains unscaled pass both."""
    from linna_amd import sampler
    rule = sampler.HMCSampler.rhat_rule
    x, y = emul.wide_chains(0)
    for z, verdict in ((x, True), (y, False)):
        dc = sampler.DeviceChain()
        assert dc._rank_scratch is None
        dc.append(torch.as_tensor(z[:300], device="cuda"))
        dc.append(torch.as_tensor(z[300:], device="cuda"))
        assert rule(dc.rhat(), dc.ess(), 1.01, 400)
        rr = dc.rank_rhat()
        ref, _ = emul.rank_rhat(z)
        np.testing.assert_allclose(dc.last_rank_rhat[:, :3], ref[:, :3], rtol=ce.BAR)
        assert np.array_equal(dc.last_rank_rhat[:, 3], ref[:, 3]) and np.array_equal(rr, dc.last_rank_rhat[:, 0])
        assert bool(np.all(rr < 1.01)) is verdict
        if not verdict:
            assert dc.last_rank_rhat[0, 1] < 1.005 and dc.last_rank_rhat[0, 2] > 1.03
        ref2, _ = emul.rank_rhat(z[31:290])
        np.testing.assert_allclose(dc.rank_rhat(discard=31, upto=290), ref2[:, 0], rtol=ce.BAR)
        with pytest.raises(_lib.LinnaHipError):
            dc.rank_rhat(discard=10, upto=13)


def test_driver_confirms_with_rank_rhat(tmp_path, monkeypatch):
    """The Gaussian of test_driver_stops_on_rhat_and_ess, same seed, ``rhat_rank`` False and True.  False: the run stops at the
    first check the plain rule passes (by the restatement, as the parent) and never builds the sort's scratch.  True: it stops
    at the same row or later, the common prefix of the chains is bit-identical, and ``diagnostics`` holds the bulk and tail
    R-hat of the restatement on the rows read back from chhmc.h5."""
    from linna_amd import sampler, util
    from test_gpu_rhat import _problem
    t, x0, mass = _problem()
    made = []
    base = sampler.DeviceChain

    class Spy(base):
        def __init__(self, *a, **k):
            base.__init__(self, *a, **k)
            made.append(self)

    monkeypatch.setattr(sampler, "DeviceChain", Spy)
    runs = {}
    for flag in (False, True):
        out = os.path.join(str(tmp_path), str(flag))
        os.makedirs(out)
        np.random.seed(1)
        drv = sampler.HMCSampler(t["lp"], None, None, t["nd"], 64, x0=x0, m=mass, transform=util.Transform(t["priors"]), seed=5)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            drv.sample(None, 2000, samp_steps=4, samp_eps=0, Madapt=50, outdir=out, method="hmc", criterion="rhat", ncheck=50,
                       rhat_rank=flag)
        d = sampler.ChainStore.load(os.path.join(out, "chhmc.h5"))
        runs[flag] = (np.asarray(d["chain"], np.float64), drv.diagnostics, buf.getvalue())
    rule = sampler.HMCSampler.rhat_rule
    za, da, ta = runs[False]
    na = len(za)
    assert 50 < na < 2000 and na % 50 == 0 and da["n"] == na and "rhat_bulk" not in da and "max bulk rhat" not in ta
    assert rule(rhat_emul.split_rhat(za)[:, 0], rhat_emul.multichain_ess(za)[0], 1.01, 400)
    for earlier in range(50, na, 50):
        assert not rule(rhat_emul.split_rhat(za[:earlier])[:, 0], rhat_emul.multichain_ess(za[:earlier])[0], 1.01, 400), earlier
    assert ta.count("max rhat, min ess") == na // 50
    assert made[0]._rank_scratch is None and made[1]._rank_scratch is not None
    zb, db, tb = runs[True]
    nb = len(zb)
    print("  rhat_rank False: %d rows; True: %d rows, %d confirmations" % (na, nb, tb.count("max bulk rhat")))
    assert na <= nb < 2000 and np.array_equal(za, zb[:na])
    assert tb.count("max rhat, min ess") == nb // 50 and tb.count("max bulk rhat") >= 1
    ref, _ = emul.rank_rhat(zb)
    assert db["n"] == nb and np.all(ref[:, 0] < 1.01)
    np.testing.assert_allclose(db["rhat_bulk"], ref[:, 1], rtol=ce.BAR)
    np.testing.assert_allclose(db["rhat_tail"], ref[:, 2], rtol=ce.BAR)
    np.testing.assert_allclose(db["rhat_rank"], ref[:, 0], rtol=ce.BAR)
    for earlier in range(na, nb, 50):                          # every check between the two stops: the plain rule or the confirmation failed
        z = zb[:earlier]
        plain = rule(rhat_emul.split_rhat(z)[:, 0], rhat_emul.multichain_ess(z)[0], 1.01, 400)
        assert not (plain and np.all(emul.rank_rhat(z)[0][:, 0] < 1.01)), earlier
