"""GPU: the rank-normalised bulk-ESS and tail-ESS (csrc/chain_rank.hip through ``linna_chain_rank_ess``) against the
restatement of the definition (tests/rank_ess_emul.py: scipy's ``rankdata`` and ``ndtri``, lagged products as plain sums, its
own Geyer loop), then ``DeviceChain.rank_ess`` and ``ess_rank=True`` through the driver.

The four ESS values are held to ``chain_exact.BAR`` = 1e-9, the project's bar for chain statistics, with NaNs in the same
places; the last pairs and the status must be EQUAL, and a second call must give the same bits.  The discrete outputs are
decided by the sign of a pair P_t: every case is required to have the restatement's margin (the smallest |P_t| up to the pair
that ends the sequence) above 1e-6 for every series of every parameter -- the seeds were chosen on the CPU so that none is
left out, and ``_check`` asserts it.  Measured on MI355X: largest relative difference of an ESS over all cases 2.3e-14, of a
quantile's ESS on the integer chains 7.8e-16.

Padded lanes and the rows outside the window hold -1e30: it would move every rank and both quantiles if it entered."""
import contextlib
import io
import os

import numpy as np
import pytest

import chain_exact as ce
import rank_ess_emul as emul
import rhat_emul
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENTINEL = np.float32(-1e30)
WORST = [0.0]


def _run(x, lo, hi, kuse=None, nwp=None, rows_after=2, npar=None, short=0):
    """x[N, nw, nd] float32 -> (rc, out[nd, 8]) of the window [lo, hi) of the image CT[lo + N + rows_after][nd][nwp] whose rows
    [lo, lo + N) hold x and everything else the sentinel.  ``kuse`` None: n - 1, every lag."""
    N, nw, nd = x.shape
    assert hi - lo == N
    nwp = (nw + 63) & ~63 if nwp is None else nwp
    ct = np.full((lo + N + rows_after, nd, nwp), SENTINEL, np.float32)
    ct[lo:hi, :, :min(nw, nwp)] = x.transpose(0, 2, 1)[:, :, :nwp]
    n = N // 2
    kuse = n - 1 if kuse is None else kuse
    lib = _lib.load()
    need = int(lib.linna_chain_rank_ess_scratch_bytes(nd, nw, 2 * n, kuse, nd if npar is None else npar)) if n >= 2 else 0
    need = need or 4096                                       # (arguments the size function refuses: the entry refuses them too)
    dct = torch.as_tensor(ct, device="cuda")
    scratch = torch.empty(max(need - short, 8), dtype=torch.uint8, device="cuda")
    out = torch.full((nd, 8), -7.0, dtype=torch.float64, device="cuda")
    rc = lib.linna_chain_rank_ess(_lib.ctx(), _lib.ptr(dct), nd, nwp, nw, lo, hi, kuse, _lib.ptr(scratch, torch.uint8), need - short,
                                  _lib.ptr(out, torch.float64), _lib.stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def _compare(out, ref, margin):
    assert np.all(margin > emul.MARGIN), ("a series too close to the end of its sequence: another seed", margin)
    assert np.array_equal(np.isnan(out[:, :4]), np.isnan(ref[:, :4])), (out, ref)
    with np.errstate(invalid="ignore"):
        if np.any(np.isfinite(ref[:, :4])):
            worst = float(np.nanmax(np.abs(out[:, :4] / ref[:, :4] - 1.0)))
            WORST[0] = max(WORST[0], worst)
            print("  largest relative difference of an ESS: this case %.3g, so far %.3g" % (worst, WORST[0]))
    np.testing.assert_allclose(out[:, :4], ref[:, :4], rtol=ce.BAR)
    assert np.array_equal(out[:, 4:], ref[:, 4:]), (out[:, 4:], ref[:, 4:])


def _check(x, lo=0, odd_nan=False, kuse=None, **kw):
    """The window holding x (with ``odd_nan``: an odd window whose dropped middle row is NaN) against the restatement."""
    x = np.asarray(x, np.float32)
    if odd_nan:
        n = len(x) // 2
        x = np.concatenate([x[:n], np.full((1,) + x.shape[1:], np.nan, np.float32), x[len(x) - n:]])
    N = len(x)
    ref, margin = emul.rank_ess(x, kuse)
    rc, out = _run(x, lo, lo + N, kuse, **kw)
    assert rc == 0, _lib.load().linna_last_error().decode()
    _compare(out, ref, margin)
    rc2, out2 = _run(x, lo, lo + N, kuse, **kw)
    assert rc2 == 0 and np.array_equal(out, out2, equal_nan=True)
    return out, ref


def mixed(N, nw, seed):
    """Three parameters: AR(1) with a large offset; a chain in which 25 % of the rows repeat their predecessor bit for bit
    (rejected transitions); N(0, 1) with both zeros, float32 subnormals of both signs and a few exact ties."""
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


# the seeds of every case (chosen on the CPU: every series of every parameter has a margin above 1e-6)
LANE_SEEDS = {1: 1, 3: 3, 64: 64, 65: 65, 130: 130}
TWO_ROW_SEEDS = {1: (41, 51), 65: (105, 115)}
TILE_SEEDS = {2047: 2047, 2048: 12048, 2049: 2049}          # (seed 2048: a margin of 8e-6 -- above the bar, but thin)


@pytest.mark.parametrize("nw", [1, 3, 64, 65, 130])
def test_every_lane_count_around_the_wavefront(nw):
    """C = 2 ... 260 lanes of the image, lo > 0, an even window and an odd one whose dropped middle row is NaN."""
    x = mixed(100, nw, seed=LANE_SEEDS[nw])
    _check(x, lo=7)
    _check(x, lo=3, odd_nan=True)


@pytest.mark.parametrize("nw", [1, 65])
def test_two_rows_a_half(nw):
    """N = 4: one pair, kuse = 1 (N = 5 with the NaN row in the middle likewise)."""
    a, b = TWO_ROW_SEEDS[nw]
    _check(mixed(4, nw, seed=a), lo=3, kuse=1)
    _check(mixed(4, nw, seed=b), lo=0, odd_nan=True, kuse=1)


@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_around_one_sort_tile(n):
    """S = 4094, 4096, 4098: below one tile of the sort, exactly one, one pair more; 256 lags of 2047 and more."""
    _check(mixed(2 * n, 1, seed=TILE_SEEDS[n])[:, :, :2], lo=1, kuse=255)


def test_exact_integer_chains_with_ties_and_a_constant_parameter():
    """The integer chains of chain_exact (a few dozen distinct values: ties straddle both quantiles; one constant parameter:
    NaN for it only).  The indicators' lagged products and sums are small integers, exact in float64 whatever the order: what
    is left between the device and the restatement is the roundings of acov = S_k - m (2 T - tail - head) + (N - k) m^2 (six,
    with a cancellation of at most 20 where a chain starts on the rarer side of its quantile: 1.4e-14 of A_k), twice per pair,
    over at most a few dozen pairs, on a tau of order 1: 1e-12."""
    x = ce.rhat_chain(65)[:301].transpose(0, 2, 1).astype(np.float32)
    out, ref = _check(x, lo=5)
    const = [i for i, p in enumerate(ce.RHAT_PARAMS) if p[0] == "const"]
    live = np.delete(np.arange(x.shape[2]), const)
    assert np.all(np.isnan(out[const, :4])) and np.all(out[const, 4:7] == -1) and np.all(np.isfinite(out[live, :4]))
    print("  quantile ESS, largest relative difference: %.3g" % np.max(np.abs(out[live, 2:4] / ref[live, 2:4] - 1)))
    np.testing.assert_allclose(out[live, 2:4], ref[live, 2:4], rtol=1e-12)


def test_a_value_that_is_not_finite_spoils_its_parameter_only():
    x = mixed(100, 65, seed=21)
    rc, clean = _run(x, 4, 104)
    assert rc == 0
    for bad, row in ((np.inf, 77), (np.nan, 13), (-np.inf, 50)):
        y = x.copy()
        y[row, 9, 1] = bad
        out, _ = _check(y, lo=4)
        assert np.all(np.isnan(out[1, :4])) and np.all(out[1, 4:7] == -1) and out[1, 7] == 0
        assert np.array_equal(out[[0, 2]], clean[[0, 2]])


def test_parameter_rounds():
    """ndim = 5 with scratch for 1, 2 and 5 parameters a round: the same bits."""
    x = np.concatenate([mixed(100, 65, seed=31), mixed(100, 65, seed=32)[:, :, :2]], axis=2)
    got = [_run(x, 6, 106, npar=k) for k in (1, 2, 5)]
    assert all(g[0] == 0 for g in got)
    for g in got[1:]:
        assert np.array_equal(g[1], got[0][1], equal_nan=True)
    _compare(got[0][1], *emul.rank_ess(x))


def sticky(nw=8, seed=2):
    return emul.sticky_tail(seed, nt=400, nw=nw)


def test_more_lags_are_asked_for_while_a_sequence_has_not_ended():
    """A sticky upper tail (n = 200): the 95 % indicator's pairs are positive far beyond lag 31.  kuse = 31: status 1 and the
    restatement's values for those lags; kuse = n - 1: status 0 and the restatement's values."""
    x = sticky()
    out, ref = _check(x, lo=2, kuse=31)
    assert out[0, 7] == 1 and out[0, 6] == 15
    out, ref = _check(x, lo=2)
    assert out[0, 7] == 0 and out[0, 6] > 15


def test_refusals_launch_nothing():
    x = mixed(8, 65, seed=3)
    lib = _lib.load()
    for kw, xx, lo, hi in ((dict(short=1, npar=1), x, 0, 8), (dict(nwp=64), x, 0, 8), (dict(kuse=0), x, 0, 8), (dict(kuse=4), x, 0, 8),
                           (dict(kuse=1), x[:3], 5, 8)):
        rc, out = _run(xx, lo, hi, **kw)
        assert rc == _lib.ERR_INVALID and "chain_rank_ess" in lib.linna_last_error().decode(), (kw, rc)
        assert np.all(out == -7.0)
    assert lib.linna_chain_rank_ess_scratch_bytes(3, 4096, 1 << 20, 31, 1) == 0          # S = 2^32: refused by arithmetic alone
    rc, out = _run(x[:4], 5, 9, kuse=1)
    assert rc == 0 and np.all(out != -7.0)


def test_device_chain_rank_ess():
    """Two appended blocks, ``discard=`` / ``upto=``, the scratch only once a rank statistic is asked for, and the lag growth
    (x 4 from LAGS0 - 1 while status is 1, capped at n - 1) on the sticky chain."""
    from linna_amd import sampler
    x = mixed(400, 65, seed=7)
    dc = sampler.DeviceChain()
    dc.append(torch.as_tensor(x[:300], device="cuda"))
    dc.append(torch.as_tensor(x[300:], device="cuda"))
    dc.rhat(), dc.ess()
    assert dc._rank_scratch is None
    bulk, tail = dc.rank_ess()
    assert dc._rank_scratch is not None and dc.last_rank_ess.shape == (3, 8)
    _compare(dc.last_rank_ess, *emul.rank_ess(x))
    assert np.array_equal(bulk, dc.last_rank_ess[:, 0]) and np.array_equal(tail, dc.last_rank_ess[:, 1])
    dc.rank_ess(discard=31, upto=290)
    _compare(dc.last_rank_ess, *emul.rank_ess(x[31:290]))
    rr = dc.rank_rhat()                                           # (the shared scratch serves both)
    assert np.all(np.isfinite(rr))
    with pytest.raises(_lib.LinnaHipError):
        dc.rank_ess(discard=10, upto=13)
    y = sticky()
    dc = sampler.DeviceChain()
    dc.LAGS0 = 32
    dc.append(torch.as_tensor(y, device="cuda"))
    tok = dc.rank_ess_begin()
    assert tok["kuse"] == 31
    dc.rank_ess_end(tok)
    assert tok["kuse"] == 199                                     # 31 -> 127 -> 199 = n - 1
    _compare(dc.last_rank_ess, *emul.rank_ess(y))


def test_driver_confirms_with_rank_ess(tmp_path, monkeypatch):
    """The Gaussian of test_driver_stops_on_rhat_and_ess, same seed, ``ess_rank`` False and True.  False: the run stops at the
    first check the plain rule passes (by the restatement, as the parent), prints nothing new, keeps no ``ess_bulk`` and never
    builds the sort's scratch.  True: it stops at the same row or later, the common prefix of the chains is bit-identical,
    ``diagnostics`` holds the bulk-ESS and tail-ESS of the restatement on the rows read back from chhmc.h5, both at least
    ``ess_min``, and at every check between the two stops the plain rule or the confirmation failed by the restatement."""
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
                       **(dict(ess_rank=True) if flag else {}))
        d = sampler.ChainStore.load(os.path.join(out, "chhmc.h5"))
        runs[flag] = (np.asarray(d["chain"], np.float64), drv.diagnostics, buf.getvalue())
    rule = sampler.HMCSampler.rhat_rule
    plain = lambda z: rule(rhat_emul.split_rhat(z)[:, 0], rhat_emul.multichain_ess(z)[0], 1.01, 400)
    za, da, ta = runs[False]
    na = len(za)
    assert 50 < na < 2000 and na % 50 == 0 and da["n"] == na
    assert "ess_bulk" not in da and "ess_tail" not in da and "bulk ess" not in ta and "max bulk rhat" not in ta
    assert plain(za) and not any(plain(za[:earlier]) for earlier in range(50, na, 50))
    assert ta.count("max rhat, min ess") == na // 50
    assert made[0]._rank_scratch is None and made[1]._rank_scratch is not None
    zb, db, tb = runs[True]
    nb = len(zb)
    print("  ess_rank False: %d rows; True: %d rows, %d confirmations" % (na, nb, tb.count("min bulk ess, min tail ess")))
    assert na <= nb < 2000 and np.array_equal(za, zb[:na])
    assert tb.count("max rhat, min ess") == nb // 50 and tb.count("min bulk ess, min tail ess") >= 1 and "max bulk rhat" not in tb
    ref, margin = emul.rank_ess(zb)
    assert np.all(margin > emul.MARGIN), margin
    assert db["n"] == nb and np.all(ref[:, 0] >= 400) and np.all(ref[:, 1] >= 400)
    np.testing.assert_allclose(db["ess_bulk"], ref[:, 0], rtol=ce.BAR)
    np.testing.assert_allclose(db["ess_tail"], ref[:, 1], rtol=ce.BAR)
    for earlier in range(na, nb, 50):                          # every check between the two stops
        z = zb[:earlier]
        e = emul.rank_ess(z)[0]
        assert not (plain(z) and np.all(e[:, 0] >= 400) and np.all(e[:, 1] >= 400)), earlier
