"""GPU: the chain-statistics kernels of csrc/autocorr.hip, entry by entry through the C ABI (``_lib``, no DeviceChain),
against the integer references of tests/chain_exact.py on exact integer chains (tests/test_chain_exact_host.py pins the
chains' exactness, the references against the oracle and tests/rhat_emul.py, and the bound and margin of every case here).

Surfaces held with ``np.array_equal`` on the bits, no element, lag, lane or case left out: CT of linna_chain_append_t, Ssum and
Tsum of linna_acorr_update (every lag the call owns; every other lag and the guard lag block keep the sentinel), M of
linna_chain_block_moments, the window / status of linna_acorr_tau, the last pair / status of linna_acorr_ess.  Continuous
outputs (tau, ESS, R-hat, W, var+, the means and standard deviations) are held within the bound chain_exact derives for the
kernel's own formula from the reference's magnitudes: no tolerance in this file is a literal.

Conventions of tests/test_gpu_entries.py: every output buffer is one guard unit longer (a row of CT, a block of 32 lags, a
record of M, 8 outputs, 64 doubles of scratch) and pre-filled with a sentinel; input pads -- the columns of a chain block past
ndim, the lanes of CT no entry may read (past nwc for the running sums, past nw / nws for R-hat and the moments), the row
behind the chain, the records of M past nblocks -- hold NaN; torch.cuda.synchronize() before every read.

Shapes, the smallest at which each mechanism can go wrong: anchor counts around the tile of 16 rows (1, 15, 16, 17, 33); lag
ranges of one wave, one workgroup, a second partly empty workgroup and a range that starts at 32 (lag growth: Tsum must not
move); windows shorter than the lags; lo > 0; rows leaving at the front, fewer and more than there are lags, partners crossing
hi; nwc < nwp (the series -> parameter mapping) with 1, 2 and 3 parameters; a seeded interleaving of ragged appends, entering
rows, a moving discard and lag growth checked against sums from scratch at every step; kuse around the chunk of 32 lags and
the 256 threads of the window kernel (0, 31, 32, 33, 255, 256, 600, N - 1), nlive of 1, nwc - 1, nwc with DATA in the lanes
past nlive; the status-1 chain, the constant parameter, the chain whose first Geyer pair is negative, an unpaired last lag;
R-hat halves holding 0, 1 and 17 whole blocks (one more than the 16 wavefronts), N odd, n = 2, nblocks below what the window
spans, M against M = NULL (bit-identical here: every sum is exact), 1 / 64 / 65 walkers in 128 lanes.
Not reached: the argmin-0 rule of the window (all lags true at kuse = N - 1) -- the autocovariances of all N lags sum to acf_0 / 2,
so tau_{N-1} = 0 and lag N - 1 is always false for N >= 2.  Left out: the split of linna_chain_block_moments into launches of
32768 records, which needs a gigabyte of chain.

Wall time of the module on an MI355X, measured: 129 cases in 2.5 s (the slowest: the 384 appends of ndim = 1, 0.2 s, which
include the start of the device context; tau from 608 lags of 512 series with the integer check of those sums, 0.1 s; the 384
appends of ndim = 255, 0.1 s; the update sequence, 0.1 s).  Worst error in units of the derived bound, measured there
(``LINNA_CHAIN_MEASURE=1`` with ``-s`` prints every case's): tau 0.01, ESS 0.32 (the floored tau: one ulp of log10), mean / std
0.16, R-hat and its three companions 0.11 -- the bounds hold with room and none is vacuous.
"""
import os

import numpy as np
import pytest

import chain_exact as ce
import entries_ref as er
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
NAN = float("nan")
SENT = er.SENTINEL          # float32 buffers (CT)
SENT64 = er.SENTINEL + 0.25  # float64 buffers: no sum of integers equals it
INVALID = _lib.ERR_INVALID
MEASURE = os.environ.get("LINNA_CHAIN_MEASURE") == "1"       # print every case's worst error in units of its derived bound

_KEEP = []
_CACHE = {}


@pytest.fixture(autouse=True)
def _release_device_buffers():
    """Tensors stay referenced until the test ends: a pointer taken from a temporary would otherwise outlive its block."""
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def dev(a):
    _KEEP.append(torch.as_tensor(np.ascontiguousarray(a), device="cuda"))
    return _KEEP[-1]


def P(t):
    return None if t is None else _lib.ptr(t, t.dtype)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(got, want, what):
    """got equals the integer (or float) reference bit for bit, everywhere."""
    want = np.asarray(want).astype(got.dtype)
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: got %r, reference %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def untouched(a, what, sent=SENT64):
    assert np.all(np.asarray(a) == sent), "%s: the sentinel was overwritten" % what


def within(got, ref, bound, what):
    """|got - ref| <= bound where the reference is finite, NaN exactly where it is NaN."""
    got, ref, bound = np.asarray(got), np.asarray(ref), np.asarray(bound)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), "%s: NaN pattern %r, reference %r" % (what, got, ref)
    err = np.abs(got - ref)[~nan]
    if MEASURE and err.size:
        with np.errstate(invalid="ignore", divide="ignore"):
            print("MEASURE %s: worst error / bound %.3g" % (what, np.nanmax(np.where(err > 0, err / bound[~nan], 0.0))))
    assert np.all(err <= bound[~nan]), "%s: error %r exceeds the derived bound %r (got %r, reference %r)" % (what, err, bound[~nan], got, ref)


def lib():
    return _lib.load(), _lib.ctx(), _lib.stream()


# ----------------------------------------------------------------------------------------------- linna_chain_append_t
def _append(block, ldb, nsteps, nw, ndim, wstride, nwp, row0):
    L, ctx, st = lib()
    img = np.full((nsteps, nw, ldb), NAN, F)
    img[:, :, :ndim] = block
    ct = torch.full((row0 + nsteps + 1, ndim, nwp), SENT, dtype=torch.float32, device="cuda")
    _KEEP.append(ct)
    rc = L.linna_chain_append_t(ctx, P(dev(img)), ldb, nsteps, nw, ndim, wstride, P(ct), nwp, row0, st)
    return rc, ct


@pytest.mark.parametrize("ndim", [1, 3, 64, 255])
def test_append_is_the_lane_permutation_with_zero_pads(ndim):
    """CT rows [row0, row0 + nsteps) equal append_ref (lanes >= nw exactly zero), every other row keeps the sentinel; ndim = 255
    is the last value whose tile fits the 64 KiB of dynamic LDS."""
    ncase = 0
    for nw in (1, 63, 64, 65, 130):
        for nsteps, row0 in ((1, 0), (5, 0), (1, 7), (5, 7)):
            block = er.ints(("append", ndim, nw, nsteps), (nsteps, nw, ndim), amax=100)
            for ldb in (ndim, er.ld4(ndim) + 4):
                for wstride in sorted(set((1, 2, 3, nw, nw + 5))):
                    for nwp in ((nw + 63) // 64 * 64, (nw + 63) // 64 * 64 + 64):
                        rc, ct = _append(block, ldb, nsteps, nw, ndim, wstride, nwp, row0)
                        assert rc == 0, (nw, nsteps, row0, ldb, wstride, nwp, _lib.load().linna_last_error())
                        got = host(ct)
                        what = "append nw %d nsteps %d row0 %d ldb %d wstride %d nwp %d" % (nw, nsteps, row0, ldb, wstride, nwp)
                        same_bits(got[row0:row0 + nsteps], ce.append_ref(block, nw, ndim, wstride, nwp), what)
                        untouched(got[:row0], what + " (rows before row0)", SENT)
                        untouched(got[row0 + nsteps:], what + " (the row behind)", SENT)
                        ncase += 1
    assert ncase == (4 + 4 * 5) * 4 * 2 * 2                     # (nw = 1: wstride 1 and nw coincide)


def test_append_refuses_what_it_cannot_launch():
    block = er.ints("refuse", (1, 2, 256))
    rc, ct = _append(block, 256, 1, 2, 256, 1, 64, 0)
    assert rc == INVALID                                        # ndim = 256: the tile [64][257] is past 64 KiB of LDS
    untouched(host(ct), "refused append", SENT)
    L, ctx, st = lib()
    small = dev(np.zeros((4, 2, 3), F))
    ct = torch.full((4, 3, 64), SENT, dtype=torch.float32, device="cuda")
    _KEEP.append(ct)
    assert L.linna_chain_append_t(ctx, P(small), 3, 65536, 2, 3, 1, P(ct), 64, 0, st) == INVALID      # grid.y is the step count
    assert L.linna_chain_append_t(ctx, P(small), 2, 1, 2, 3, 1, P(ct), 64, 0, st) == INVALID          # ldb < ndim
    assert L.linna_chain_append_t(ctx, P(small), 3, 1, 65, 3, 1, P(ct), 64, 0, st) == INVALID         # more walkers than lanes
    untouched(host(ct), "refused append", SENT)


# ----------------------------------------------------------------------------------------------- linna_acorr_update
UPD_ROWS, UPD_K = 120, 160
UPD_LAYOUTS = ((1, 64, 64), (3, 192, 64), (2, 128, 128), (3, 192, 128))        # (ndim, nwp, nwc)
UPD_PARAMS = (("ar", 0.5), ("ar", 0.99), ("ar", 0.9))
LAG_RANGES = ((0, 32), (0, 128), (0, 160), (32, 96))


def _upd_chain(nd, nwc):
    return ce.cached_chain("upd", UPD_ROWS, nwc, UPD_PARAMS[:nd])


def _update(ct, nd, nwp, nwc, a0, a1, lo, hi, k0, k1, S0, T0, remove, ktot=UPD_K):
    """One call on sums S0[ktot][nd][nwc] (None entries: the sentinel) / T0; returns what S (with its guard lag block) and T
    (with its guard) hold afterwards."""
    L, ctx, st = lib()
    S = np.full((ktot + 32, nd, nwc), SENT64)
    S[:ktot] = S0
    T = None
    if T0 is not None:
        T = np.full(nd * nwc + 8, SENT64)
        T[:nd * nwc] = np.asarray(T0, np.float64).ravel()
    Sd, Td = dev(S), (None if T is None else dev(T))
    assert L.linna_acorr_update(ctx, P(ct), nd, nwp, nwc, a0, a1, lo, hi, k0, k1, P(Sd), P(Td), remove, st) == 0
    return host(Sd), (None if Td is None else host(Td))


def _check_update(x, got, k0, k1, lo, hi, T_want, what):
    S, T = got
    Sw, _ = ce.sums_ref(x, lo, hi, UPD_K)
    same_bits(S[k0:k1], Sw[k0:k1], what + ": Ssum")
    untouched(S[:k0], what + ": lags below k0")
    untouched(S[k1:], what + ": lags from k1 on and the guard block")
    if T is not None:
        nser = x.shape[1] * x.shape[2]
        same_bits(T[:nser], np.asarray(T_want).ravel(), what + ": Tsum")
        untouched(T[nser:], what + ": behind Tsum")


@pytest.mark.parametrize("layout", UPD_LAYOUTS, ids=lambda l: "nd%d_nwp%d_nwc%d" % l)
def test_update_sums_bit_for_bit(layout):
    nd, nwp, nwc = layout
    x = _upd_chain(nd, nwc)
    ct = dev(ce.ct_image(x, nwp, NAN, rows=UPD_ROWS + 1))
    sent = np.full((UPD_K, nd, nwc), SENT64)

    def start(Sb, k0, k1):
        S0 = sent.copy()
        S0[k0:k1] = Sb[k0:k1]
        return S0

    # ---- rows entering at the end of [lo, a0): every anchor count around the tile of 16 x every lag range
    for lo, a0 in ((0, 40), (37, 40)):                          # lo = 37: a0 - k < lo for all lags but three
        Sb, Tb = ce.sums_ref(x, lo, a0, UPD_K)
        for cnt in (1, 15, 16, 17, 33):
            a1 = a0 + cnt
            _, Ta = ce.sums_ref(x, lo, a1, 1)
            for k0, k1 in LAG_RANGES:
                what = "enter lo %d rows [%d, %d) lags [%d, %d)" % (lo, a0, a1, k0, k1)
                got = _update(ct, nd, nwp, nwc, a0, a1, lo, a1, k0, k1, start(Sb, k0, k1), Tb, 0)
                _check_update(x, got, k0, k1, lo, a1, Ta if k0 == 0 else Tb, what)
    # ---- from scratch: a window shorter than the lags; lag growth from the stored chain with and without Tsum
    zero = np.zeros((UPD_K, nd, nwc))
    _, T5 = ce.sums_ref(x, 10, 15, 1)
    got = _update(ct, nd, nwp, nwc, 10, 15, 10, 15, 0, 32, start(zero, 0, 32), np.zeros((nd, nwc)), 0)
    _check_update(x, got, 0, 32, 10, 15, T5, "N = 5 with 32 lags")
    _, T50 = ce.sums_ref(x, 3, 53, 1)
    got = _update(ct, nd, nwp, nwc, 3, 53, 3, 53, 32, 96, start(zero, 32, 96), T50, 0)
    _check_update(x, got, 32, 96, 3, 53, T50, "lag growth [32, 96), Tsum given")
    got = _update(ct, nd, nwp, nwc, 3, 53, 3, 53, 32, 96, start(zero, 32, 96), None, 0)
    _check_update(x, got, 32, 96, 3, 53, None, "lag growth [32, 96), Tsum = NULL")
    # ---- rows leaving at the front of [5, 55): fewer and more than there are lags, partners crossing hi
    Sb, Tb = ce.sums_ref(x, 5, 55, UPD_K)
    for r, (k0, k1) in ((7, (0, 32)), (45, (0, 32)), (33, (0, 128)), (17, (32, 96)), (49, (0, 160))):
        _, Ta = ce.sums_ref(x, 5 + r, 55, 1)
        what = "remove %d rows of [5, 55) lags [%d, %d)" % (r, k0, k1)
        got = _update(ct, nd, nwp, nwc, 5, 5 + r, 5, 55, k0, k1, start(Sb, k0, k1), Tb, 1)
        _check_update(x, got, k0, k1, 5 + r, 55, Ta if k0 == 0 else Tb, what)


def test_update_sequence_equals_sums_from_scratch_at_every_step():
    """A fixed, seeded interleaving of ragged appends (through linna_chain_append_t, every third walker first), entering rows,
    a moving discard and lag growth: after every step the running sums equal sums_ref from scratch on the window, bit for bit."""
    L, ctx, st = lib()
    nd, nw, wstride, nwp, nwc, rows, kmax = 2, 100, 3, 128, 64, 400, 160
    walkers = ce.cached_chain("seq", rows, nw, (("ar", 0.9), ("ar", 0.5)))          # [row][d][walker]
    x = np.ascontiguousarray(walkers[:, :, ce.lane_order(nw, wstride)][:, :, :nwc])
    blocks = np.ascontiguousarray(walkers.transpose(0, 2, 1)).astype(F)           # [row][walker][d]
    ct = torch.full((rows + 1, nd, nwp), NAN, dtype=torch.float32, device="cuda")
    S = torch.full((kmax + 32, nd, nwc), SENT64, dtype=torch.float64, device="cuda")
    S[:32] = 0
    T = torch.zeros(nd * nwc, dtype=torch.float64, device="cuda")
    _KEEP.extend([ct, S, T])
    rs = ce.rng("sequence")
    n = lo = hi = 0
    K = 32
    done = {"append": 0, "discard": 0, "grow": 0}
    for step in range(36):
        op = "append" if step == 0 else rs.choice(["append", "append", "discard", "grow"])
        if op == "append" and n < rows:
            r = int(min(rows - n, rs.randint(1, 41)))
            assert L.linna_chain_append_t(ctx, P(dev(blocks[n:n + r])), nd, r, nw, nd, wstride, P(ct), nwp, n, st) == 0
            n += r
            assert L.linna_acorr_update(ctx, P(ct), nd, nwp, nwc, hi, n, lo, n, 0, K, P(S), P(T), 0, st) == 0
            hi = n
        elif op == "discard" and hi - lo > 3:
            new = lo + int(rs.randint(1, min(hi - lo - 2, 50) + 1))
            assert L.linna_acorr_update(ctx, P(ct), nd, nwp, nwc, lo, new, lo, hi, 0, K, P(S), P(T), 1, st) == 0
            lo = new
        elif op == "grow" and K < kmax:
            S[K:K + 32] = 0
            assert L.linna_acorr_update(ctx, P(ct), nd, nwp, nwc, lo, hi, lo, hi, K, K + 32, P(S), None, 0, st) == 0
            K += 32
        else:
            continue
        done[op] += 1
        Sw, Tw = ce.sums_ref(x, lo, hi, K)
        what = "step %d (%s): window [%d, %d), %d lags" % (step, op, lo, hi, K)
        got = host(S)
        same_bits(got[:K], Sw, what + ": Ssum")
        untouched(got[K:], what + ": lags not yet kept")
        same_bits(host(T), Tw.ravel(), what + ": Tsum")
    assert min(done.values()) >= 3 and lo > 0 and K > 64, done
    same_bits(host(ct)[:n, :, :nwc], x[:n], "the appended chain")


# ----------------------------------------------------------------------------------------------- linna_chain_block_moments
@pytest.mark.parametrize("nd,nwp", [(1, 64), (3, 64), (1, 192), (3, 192)])
def test_block_moments_bit_for_bit(nd, nwp):
    L, ctx, st = lib()
    x = ce.cached_chain("moments", 5 * ce.RB + 3, nwp, UPD_PARAMS[:nd])
    ct = dev(ce.ct_image(x, nwp, NAN, rows=len(x) + 1))
    for b0 in (0, 2):
        for cnt in (1, 3):
            b1 = b0 + cnt
            M = torch.full((b1 + 1, 2, nd, nwp), SENT64, dtype=torch.float64, device="cuda")
            _KEEP.append(M)
            assert L.linna_chain_block_moments(ctx, P(ct), nd, nwp, b0, b1, P(M), st) == 0
            got = host(M)
            what = "records [%d, %d)" % (b0, b1)
            same_bits(got[b0:b1], ce.moments_ref(x, b0, b1), what)
            untouched(got[:b0], what + ": records before b0")
            untouched(got[b1:], what + ": the record behind")


# ----------------------------------------------------------------------------------------------- linna_acorr_tau / linna_acorr_ess
def _sums_on_device(case):
    """CT and the sums Ssum / Tsum of a case's window for K = kuse + 1 rounded up to 32 lags, produced by linna_acorr_update
    (never by the reference): the pair as the driver uses it."""
    _, params, rows, nwp, nwc, _, lo, hi, kuse = case
    K = (kuse + 32) // 32 * 32
    key = (params, rows, nwp, nwc, lo, hi, K)
    if key not in _CACHE:
        L, ctx, st = lib()
        x = ce.tau_case_chain(case)
        nd = x.shape[1]
        ct = torch.as_tensor(ce.ct_image(x, nwp, NAN, rows=rows + 1), device="cuda")
        S = torch.zeros((K, nd, nwc), dtype=torch.float64, device="cuda")
        T = torch.zeros((nd, nwc), dtype=torch.float64, device="cuda")
        assert L.linna_acorr_update(ctx, P(ct), nd, nwp, nwc, lo, hi, lo, hi, 0, K, P(S), P(T), 0, st) == 0
        Sw, Tw = ce.sums_ref(x, lo, hi, K)                     # (up to 640 lags: five workgroups of lag blocks)
        same_bits(host(S), Sw, "Ssum of %s for %d lags" % (case[0], K))
        same_bits(host(T), Tw, "Tsum of %s" % case[0])
        _CACHE[key] = (ct, S, T)
    return _CACHE[key]


def _finish(case, ess):
    L, ctx, st = lib()
    _, params, rows, nwp, nwc, nlive, lo, hi, kuse = case
    nd = len(params)
    ct, S, T = _sums_on_device(case)
    nbytes = int((L.linna_acorr_ess_scratch_bytes if ess else L.linna_acorr_scratch_bytes)(nd, nwc, kuse))
    assert nbytes > 0 and nbytes % 8 == 0
    scratch = torch.full((nbytes // 8 + 64,), SENT64, dtype=torch.float64, device="cuda")
    out = torch.full((3 * nd + 8,), SENT64, dtype=torch.float64, device="cuda")
    _KEEP.extend([scratch, out])
    if ess:
        rc = L.linna_acorr_ess(ctx, P(ct), nd, nwp, nwc, nlive, lo, hi, kuse, P(S), P(T), P(scratch), P(out), st)
    else:
        rc = L.linna_acorr_tau(ctx, P(ct), nd, nwp, nwc, nlive, lo, hi, kuse, P(S), P(T), 5.0, P(scratch), P(out), st)
    assert rc == 0
    o = host(out)
    untouched(o[3 * nd:], "behind the outputs")
    untouched(host(scratch)[nbytes // 8:], "behind the scratch")
    return o[:nd], o[nd:2 * nd], o[2 * nd:3 * nd]


@pytest.mark.parametrize("case", ce.TAU_CASES, ids=[c[0] for c in ce.TAU_CASES])
def test_tau_from_the_sums_of_the_update_entry(case):
    ref, _ = ce.tau_case_refs(case)
    tau, window, status = _finish(case, ess=False)
    assert np.array_equal(window, ref["window"]) and np.array_equal(status, ref["status"]), (window, status, ref)
    within(tau, ref["tau"], ref["bound"], "tau")


@pytest.mark.parametrize("case", ce.TAU_CASES, ids=[c[0] for c in ce.TAU_CASES])
def test_ess_from_the_sums_of_the_update_entry(case):
    _, ref = ce.tau_case_refs(case)
    ess, last, status = _finish(case, ess=True)
    assert np.array_equal(last, ref["last"]) and np.array_equal(status, ref["status"]), (last, status, ref)
    within(ess, ref["ess"], ref["bound"], "ESS")


# ----------------------------------------------------------------------------------------------- linna_chain_meanstd
@pytest.mark.parametrize("case", ce.MEANSTD_CASES, ids=lambda c: "%s" % (c,))
def test_meanstd_within_the_derived_bound(case):
    """include/linna_hip.h: an empty half gives NaN for both of its numbers, the other half is unaffected."""
    L, ctx, st = lib()
    (t0, tm, t1), nws = case
    x = ce.meanstd_chain()
    nd, nwp = x.shape[1], ce.MEANSTD_NWP
    ct = dev(ce.ct_image(x[:, :, :nws], nwp, NAN, rows=len(x) + 1))
    out = torch.full((nd * 4 + 8,), SENT64, dtype=torch.float64, device="cuda")
    _KEEP.append(out)
    assert L.linna_chain_meanstd(ctx, P(ct), nd, nwp, nws, t0, tm, t1, P(out), st) == 0
    got = host(out)
    untouched(got[nd * 4:], "behind the outputs")
    ref, bound = ce.meanstd_ref(x, nws, t0, tm, t1)
    assert np.isnan(ref[:, 0]).all() == (tm == t0) and np.isnan(ref[:, 1]).all() == (t1 == tm)
    within(got[:nd * 4].reshape(nd, 2, 2), ref, bound, "mean / std")


# ----------------------------------------------------------------------------------------------- linna_chain_rhat
NBLOCKS = ce.RHAT_ROWS // ce.RB


def _rhat_image(nw, nanrow):
    """CT (lanes >= nw NaN) and the records M of every complete block, from linna_chain_block_moments."""
    key = ("rhat", nw, nanrow)
    if key not in _CACHE:
        L, ctx, st = lib()
        nd, nwp = len(ce.RHAT_PARAMS), ce.RHAT_NWP
        img = ce.ct_image(ce.rhat_chain(nw), nwp, NAN, rows=ce.RHAT_ROWS + 1)
        if nanrow is not None:
            img = ce.with_nan_row(img, nanrow, 3)
        ct = torch.as_tensor(img, device="cuda")
        M = torch.full((NBLOCKS + 1, 2, nd, nwp), SENT64, dtype=torch.float64, device="cuda")
        assert L.linna_chain_block_moments(ctx, P(ct), nd, nwp, 0, NBLOCKS, P(M), st) == 0
        torch.cuda.synchronize()
        _CACHE[key] = (ct, M)
    return _CACHE[key]


@pytest.mark.parametrize("win", ce.RHAT_WINDOWS, ids=[w[0] for w in ce.RHAT_WINDOWS])
@pytest.mark.parametrize("nw", ce.RHAT_NW)
def test_rhat_within_the_derived_bound(win, nw):
    L, ctx, st = lib()
    _, lo, hi, nblocks, nanrow = win
    nd, nwp = len(ce.RHAT_PARAMS), ce.RHAT_NWP
    ct, M = _rhat_image(nw, nanrow)
    nb = NBLOCKS if nblocks is None else nblocks
    Mn = M.clone()
    Mn[nb:] = NAN                                               # records past nblocks must not be read
    _KEEP.append(Mn)
    ref, bound, _ = ce.rhat_ref(ce.rhat_image(nw, nanrow), lo, hi, nwp)

    def run(Mp):
        out = torch.full((nd * 4 + 8,), SENT64, dtype=torch.float64, device="cuda")
        _KEEP.append(out)
        assert L.linna_chain_rhat(ctx, P(ct), nd, nwp, nw, lo, hi, P(Mp), nb, P(out), st) == 0
        got = host(out)
        untouched(got[nd * 4:], "behind the outputs")
        return got[:nd * 4].reshape(nd, 4)

    with_m, again, without = run(Mn), run(Mn), run(None)
    assert np.array_equal(bits(with_m), bits(again)), "two calls differ"
    for name, got in (("M given", with_m), ("M = NULL", without)):
        for d in range(nd):
            if np.isnan(ref[d]).all():                          # a NaN row in the halves: the header promises the NaN R-hat
                assert np.isnan(got[d, 0]), (name, d, got[d])
            else:
                within(got[d], ref[d], bound[d], "%s, parameter %d" % (name, d))
    fin = ~np.isnan(ref).all(axis=1)
    assert np.array_equal(with_m[fin], without[fin], equal_nan=True), "block records and chain rows give different results on exact sums"


def test_rhat_refuses_halves_of_one_row():
    L, ctx, st = lib()
    ct, M = _rhat_image(64, None)
    nd, nwp = len(ce.RHAT_PARAMS), ce.RHAT_NWP
    out = torch.full((nd * 4 + 8,), SENT64, dtype=torch.float64, device="cuda")
    _KEEP.append(out)
    assert L.linna_chain_rhat(ctx, P(ct), nd, nwp, 64, 5, 8, P(M), NBLOCKS, P(out), st) == INVALID      # (hi - lo) / 2 = 1
    assert L.linna_chain_rhat(ctx, P(ct), nd, nwp, 64, 5, 9, P(M), NBLOCKS, P(out), st) == 0
    assert L.linna_chain_rhat(ctx, P(ct), nd, nwp, 129, 5, 9, P(M), NBLOCKS, P(out), st) == INVALID     # more walkers than lanes
    untouched(host(out)[nd * 4:], "behind the outputs")
