"""GPU: the stand-alone entries of the C ABI (include/linna_hip.h) -- the small kernels of csrc/pointwise.hip and the thin
GEMM wrappers at the top of csrc/api.hip -- called directly through ``_lib`` against the float64 references of
tests/entries_ref.py (pinned on the CPU by tests/test_entries_host.py).  No TrainEngine, no Log_prob.

Two devices throughout:
 * exact tables (small integers, power-of-two scales): the result equals the float64 reference BIT FOR BIT, so no tolerance
   hides a dropped row, a doubled tail element or a wrong stride;
 * pads and guards: every input matrix has a leading dimension larger than its width with NaN in the pad columns (zeros
   where the header makes them the caller's duty: packed weights, Cinv rows), every output buffer is allocated 8 elements
   (or 2 rows) longer and pre-filled with a sentinel.  ``both`` runs every call twice, NaN pads and zero pads, and requires
   bit-identical outputs; ``Out.check`` requires the guard and the output pad columns to hold what the header says.

Tolerances that are not bit equality: either derived (docstring) or set by the measured-bound rule -- four times the worst
error measured on an MI355X against the float64 reference, rounded up to one significant digit, both numbers in the
docstring.  The metric of those is |got - ref| <= tol * (|ref| + scale) with the scale named in the test
(np.testing.assert_allclose with atol = tol * scale, so LINNA_PARITY_REPORT records it; tests/parity.py widens every
assert_allclose of a GPU test by its BOX_MARGIN on top).  ``LINNA_ENTRIES_MEASURE=1`` prints each measured worst error.
"""
import ctypes as C
import os

import numpy as np
import pytest

import entries_ref as R
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
NAN = float("nan")
SENT = R.SENTINEL
MEASURE = os.environ.get("LINNA_ENTRIES_MEASURE") == "1"


# ----------------------------------------------------------------------------------------------- buffers
_KEEP = []


@pytest.fixture(autouse=True)
def _release_device_buffers():
    """Input tensors stay referenced until the test ends: a pointer taken from a temporary would otherwise outlive its block."""
    yield
    del _KEEP[:]


def dmat(a, ld=None, fill=NAN, off=0):
    """[rows][ld] device image of the 2-D float32 array ``a`` (pad columns = fill), as a flat tensor whose first element
    sits ``off`` floats behind a 16-byte aligned allocation."""
    a = np.asarray(a, F)
    rows, w = a.shape
    ld = w if ld is None else ld
    host = np.full(rows * ld + off, fill, F)
    host[off:].reshape(rows, ld)[:, :w] = a
    _KEEP.append(torch.as_tensor(host, device="cuda"))
    return _KEEP[-1][off:]


def dvec(a, dtype=F, off=0):
    if a is None:
        return None
    host = np.zeros(len(a) + off, dtype)
    host[off:] = a
    _KEEP.append(torch.as_tensor(host, device="cuda"))
    return _KEEP[-1][off:]


def ptr(t):
    return None if t is None else _lib.ptr(t, t.dtype)


class Out(object):
    """An output matrix [rows][ld] of which ``w`` columns are written, allocated ``guard`` elements (vectors: 8; matrices: two
    rows) longer, all sentinel."""

    def __init__(self, rows, w, ld=None, guard=8):
        self.rows, self.w, self.ld, self.guard = rows, w, (w if ld is None else ld), guard
        self.t = torch.full((self.rows * self.ld + guard,), SENT, device="cuda")

    @property
    def p(self):
        return _lib.ptr(self.t)

    def read(self):
        torch.cuda.synchronize()
        self.host = self.t.cpu().numpy()
        return self.host[: self.rows * self.ld].reshape(self.rows, self.ld)[:, : self.w].copy()

    def check(self, pads):
        """The guard holds the sentinel; the pad columns hold ``pads`` (0 or the sentinel)."""
        assert np.all(self.host[self.rows * self.ld:] == SENT), "wrote past the end of an output"
        body = self.host[: self.rows * self.ld].reshape(self.rows, self.ld)
        assert np.all(body[:, self.w:] == pads), "output pad columns: expected %r" % (pads,)

    def untouched(self):
        torch.cuda.synchronize()
        assert bool(torch.all(self.t == SENT))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def bit1(values):
    return [int(b) for b in bits(np.asarray(values, F))]


def biteq(got, ref64, what=""):
    """got (float32) equals the float64 reference rounded once, bit for bit."""
    ref = R.round_once(ref64)
    bad = bits(got) != bits(ref)
    assert not bad.any(), "%s: %d of %d elements differ, first at %s: got %r, reference %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), np.asarray(got)[bad][0], ref[bad][0])


def both(run):
    """``run(fill)`` with NaN pads and with zero pads: bit-identical outputs.  Returns the NaN-pad outputs."""
    a, b = run(NAN), run(0.0)
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(bits(x), bits(y)), "the result depends on the pad columns"
    return a if len(a) > 1 else a[0]


class Worst(object):
    """Measured-bound rule: collects max |got - ref| / (|ref| + scale) over a test's cases, then asserts every case with
    np.testing.assert_allclose(rtol = tol, atol = tol * scale)."""

    def __init__(self, name, tol, scale):
        self.name, self.tol, self.scale, self.worst, self.cases = name, tol, scale, 0.0, []

    def add(self, got, ref64):
        got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
        fin = np.isfinite(ref64) & np.isfinite(got)
        with np.errstate(invalid="ignore"):
            if fin.any():
                self.worst = max(self.worst, float(np.max(np.abs(got - ref64)[fin] / (np.abs(ref64)[fin] + self.scale))))
        self.cases.append((got, ref64))

    def check(self, *others):
        """Every figure is printed before anything is asserted."""
        for w in (self,) + others:
            if MEASURE:
                print("MEASURED %s worst %.3e  (tol %.1e, scale %g; 64 ulp = %.1e)" % (w.name, w.worst, w.tol, w.scale, 64 * 2.0 ** -24))
        for w in (self,) + others:
            for got, ref64 in w.cases:
                np.testing.assert_allclose(got, ref64, rtol=w.tol, atol=w.tol * w.scale, err_msg=w.name)


def env():
    return _lib.ctx(), _lib.stream()


def rc_of(name, *args):
    return getattr(_lib.load(), name)(*args)


# ----------------------------------------------------------------------------------------------- linna_val_metrics
def run_val_metrics(loss, frac, last):
    ctx, st = env()
    dl, df, dlast, out = dvec(loss), dvec(frac), (None if last is None else dvec([last])), Out(1, 4)
    _lib.call("linna_val_metrics", ctx, ptr(dl), ptr(df), len(loss), ptr(dlast), out.p, st)
    got = out.read()[0]
    out.check(SENT)
    return got


@pytest.mark.parametrize("n", R.VAL_NS)
def test_val_metrics_selection(n):
    """Lower medians and the maximum by rank counting over tiles of 256: one block, a full block, several blocks, even and odd
    counts, ties (the index tie-break), infinities, and the NaN rule -- value equality with lower_median / max."""
    for k, name in enumerate(R.val_table_names(n)):
        loss, frac = R.val_table(n, name)
        last = None if k % 2 else F(0.75 + k)
        got, ref = run_val_metrics(loss, frac, last), R.val_metrics_ref(loss, frac, last)
        same = (got == ref) | (np.isnan(got) & np.isnan(ref))
        assert same.all(), "n %d table %s: got %r, reference %r" % (n, name, got, ref)


def test_val_metrics_refuses_bad_arguments():
    """n = 65537, n = 0 and a null pointer are refused on the host (api.hip: before any launch), ``out`` untouched."""
    ctx, st = env()
    big = dvec(np.zeros(65537, F))
    out = Out(1, 4)
    for args in ((ptr(big), ptr(big), 65537, None, out.p), (ptr(big), ptr(big), 0, None, out.p), (None, ptr(big), 5, None, out.p),
                 (ptr(big), None, 5, None, out.p)):
        assert rc_of("linna_val_metrics", ctx, *args, st) == _lib.ERR_INVALID
    assert rc_of("linna_val_metrics", ctx, ptr(big), ptr(big), 5, None, None, st) == _lib.ERR_INVALID
    out.untouched()


# ----------------------------------------------------------------------------------------------- colsum_kernel
@pytest.mark.parametrize("N", R.COLSUM_N)
def test_colsum_through_linear_bwd(N):
    """db = scale * column sums of dY (16 waves x 4 accumulators, a `b + 48 < B` main loop and a tail loop): every B around the
    16 / 48 / 64 row boundaries, aligned and odd leading dimension, exact table, bit for bit."""
    ctx, st = env()
    for B in R.COLSUM_B:
        dY = R.colsum_table(B, N)
        for lddy in (R.ld4(N) + 4, N + 3):
            for scale in (1.0, 0.5):
                def run(fill):
                    d, db = dmat(dY, lddy, fill), Out(1, N)
                    _lib.call("linna_linear_bwd", ctx, ptr(d), lddy, None, 0, None, 0, None, 0, None, 0, None, 0, db.p, B, 1, N, scale, st)
                    got = db.read()[0]
                    db.check(SENT)
                    return got
                biteq(both(run), R.linear_bwd_ref(dY, np.zeros((B, 1)), np.zeros((N, 1)), None, scale)[2], "db B %d N %d ld %d" % (B, N, lddy))


# ----------------------------------------------------------------------------------------------- layers
def in_ld(w, k):
    """Leading dimension of an input matrix, larger than its width: 16-byte rows for even case numbers, odd rows otherwise."""
    return R.ld4(w) + 4 if k % 2 == 0 else w + 1


def run_linear_fwd(t, B, K, N, k, bias, relu, res, alpha):
    ctx, st = env()
    ldx, ldw, ldr, ldy = in_ld(K, k), in_ld(K, k // 2), in_ld(N, k), R.ld4(N) + 4

    def run(fill):
        X, W, Rm, Y = dmat(t["X"], ldx, fill), dmat(t["W"], ldw, fill), (dmat(t["R"], ldr, fill) if res else None), Out(B, N, ldy, 2 * ldy)
        _lib.call("linna_linear_fwd", ctx, ptr(X), ldx, ptr(W), ldw, ptr(dvec(t["b"]) if bias else None), Y.p, ldy, B, K, N, relu, alpha,
                  ptr(Rm), ldr if res else 0, st)
        got = Y.read()
        Y.check(SENT)
        return got
    return both(run)


@pytest.mark.parametrize("B,K,N", R.LAYER_SHAPES)
def test_linear_fwd_exact(B, K, N):
    """Y = act(alpha (X W^T + b) + R) on the exact table, with and without bias, relu and R, alpha 1 and 0.5: bit for bit."""
    t = R.linear_exact_table(B, K, N)
    for k, (bias, relu, res, alpha) in enumerate([(1, 1, 1, 1.0), (0, 0, 0, 1.0), (1, 0, 1, 0.5), (0, 1, 0, 0.5), (1, 1, 0, 0.5), (0, 0, 1, 1.0)]):
        got = run_linear_fwd(t, B, K, N, k, bias, relu, res, alpha)
        biteq(got, R.linear_fwd_ref(t["X"], t["W"], t["b"] if bias else None, alpha, t["R"] if res else None, relu), "linear_fwd case %d" % k)


@pytest.mark.parametrize("B,K,N", R.LAYER_SHAPES)
def test_linear_fwd_random(B, K, N):
    """A random table with alpha = 0.1, held to the bound tools/fuzz_gemm.py asserts (entries_ref.gemm_bound)."""
    t = R.linear_random_table(B, K, N)
    got = run_linear_fwd(t, B, K, N, 0, 1, 1, 1, 0.1)
    ref = R.linear_fwd_ref(t["X"], t["W"], t["b"], 0.1, t["R"], 1)
    tol, scale = R.gemm_bound(ref, K)
    assert np.abs(got - ref).max() / scale < tol


def packed(W, fill=0.0):
    """A weight matrix in the packed convention of linna_layer_t: row stride LINNA_LD(K), pad entries zero."""
    return dmat(W, R.ld4(W.shape[1]), fill)


@pytest.mark.parametrize("B,K,C_,N,ws", R.RESBLOCK_SHAPES)
def test_resblock_fwd(B, K, C_, N, ws):
    """T = relu(X W1^T + b1), Y = relu(0.1 (T W2^T + b2) + skip), identity skip and Ws; a random table (the fixed 0.1 is not
    exact) held to the bound of tools/fuzz_gemm.py with K_total = C + K."""
    ctx, st = env()
    t = R.resblock_table(B, K, C_, N, ws)
    ldx, ldt, ldy = R.ld4(K) + 4, R.ld4(C_) + 4, R.ld4(N) + 4

    def run(fill):
        X, T, Y = dmat(t["X"], ldx, fill), Out(B, C_, ldt, 2 * ldt), Out(B, N, ldy, 2 * ldy)
        Ws = packed(t["Ws"]) if ws else None
        _lib.call("linna_resblock_fwd", ctx, ptr(X), ldx, ptr(packed(t["W1"])), ptr(dvec(t["b1"])), ptr(packed(t["W2"])), ptr(dvec(t["b2"])),
                  ptr(Ws), T.p, ldt, Y.p, ldy, B, K, C_, N, st)
        gt, gy = T.read(), Y.read()
        T.check(SENT)
        Y.check(SENT)
        return gt, gy
    gt, gy = both(run)
    rt, ry = R.resblock_fwd_ref(t["X"], t["W1"], t["b1"], t["W2"], t["b2"], t["Ws"])
    for got, ref, ktot in ((gt, rt, K), (gy, ry, C_ + K)):
        tol, scale = R.gemm_bound(ref, ktot)
        assert np.abs(got - ref).max() / scale < tol


def test_resblock_fwd_identity_skip_needs_square():
    """Ws == NULL with K != N: LINNA_ERR_INVALID on the host (api.hip: the first statement of the entry), nothing written."""
    ctx, st = env()
    t = R.resblock_table(17, 3, 33, 130, True)
    X, T, Y = dmat(t["X"], 4, 0.0), Out(17, 33, 36), Out(17, 130, 132)
    rc = rc_of("linna_resblock_fwd", ctx, ptr(X), 4, ptr(packed(t["W1"])), ptr(dvec(t["b1"])), ptr(packed(t["W2"])), ptr(dvec(t["b2"])), None,
               T.p, 36, Y.p, 132, 17, 3, 33, 130, st)
    assert rc == _lib.ERR_INVALID
    T.untouched()
    Y.untouched()


@pytest.mark.parametrize("B,K,N", R.LAYER_SHAPES)
def test_linear_bwd_exact(B, K, N):
    """dX = scale (dY W) * (Xmask > 0), dW = scale dY^T X, db = scale colsum dY; each output NULL in turn, with and without the
    mask (zeros, negatives, positives), scale 1 and 0.5; exact table, bit for bit."""
    ctx, st = env()
    t = R.linear_bwd_table(B, K, N)
    for k, (wx, ww, wb, mask, scale) in enumerate([(1, 1, 1, 1, 0.5), (0, 1, 1, 0, 1.0), (1, 0, 1, 0, 0.5), (1, 1, 0, 1, 1.0)]):
        lddy, ldx, ldw, ldm = in_ld(N, k), in_ld(K, k), in_ld(K, k // 2), in_ld(K, k + 1)
        lddx, lddw = R.ld4(K) + 4, R.ld4(K) + 4

        def run(fill):
            dY, X, W, M = dmat(t["dY"], lddy, fill), dmat(t["X"], ldx, fill), dmat(t["W"], ldw, fill), (dmat(t["Xmask"], ldm, fill) if mask else None)
            dX, dW, db = Out(B, K, lddx, 2 * lddx) if wx else None, Out(N, K, lddw, 2 * lddw) if ww else None, Out(1, N) if wb else None
            _lib.call("linna_linear_bwd", ctx, ptr(dY), lddy, ptr(X), ldx, ptr(W), ldw, dX.p if wx else None, lddx, ptr(M), ldm if mask else 0,
                      dW.p if ww else None, lddw, db.p if wb else None, B, K, N, scale, st)
            res = []
            for o in (dX, dW, db):
                res.append(None if o is None else o.read())
                if o is not None:
                    o.check(SENT)
            return tuple(res)
        gx, gw, gb = both(run)
        rx, rw, rb = R.linear_bwd_ref(t["dY"], t["X"], t["W"], t["Xmask"] if mask else None, scale)
        if wx:
            biteq(gx, rx, "dX case %d" % k)
        if ww:
            biteq(gw, rw, "dW case %d" % k)
        if wb:
            biteq(gb[0], rb, "db case %d" % k)


# ----------------------------------------------------------------------------------------------- linna_gemm_f32: the rest
def gemm_desc(A, lda, Bm, ldb, M, N, K):
    g = _lib.Gemm()
    g.npairs, g.M, g.N, g.alpha0 = 1, M, N, 1.0
    g.p[0].A, g.p[0].lda, g.p[0].alay, g.p[0].B, g.p[0].ldb, g.p[0].blay, g.p[0].K = A.data_ptr(), lda, 0, Bm.data_ptr(), ldb, 0, K
    return g


@pytest.mark.parametrize("M,N,K", R.GEMM_EXTRA_SHAPES)
def test_gemm_exp_epilogue(M, N, K):
    """v = v cscale + cshift; v = exp(v) cpost + cshift2 with each of the four NULL or given (the `ypositive` output map);
    the argument of exp stays inside [-4, 4].  Measured-bound rule, scale 1: worst measured 1.9e-07 (M = N = 65, K = 5),
    asserted 8e-07."""
    ctx, st = env()
    t = R.gemm_exp_table(M, N, K)
    w = Worst("gemm exp epilogue M %d N %d K %d" % (M, N, K), TOL["gemm_exp"], 1.0)
    lda, ldb, ldc = R.ld4(K) + 4, R.ld4(K) + 4, R.ld4(N) + 4
    for combo in range(16):
        use = {n: (t[n] if combo >> i & 1 else None) for i, n in enumerate(("cscale", "cshift", "cpost", "cshift2"))}

        def run(fill):
            A, Bm, out = dmat(t["A"], lda, fill), dmat(t["B"], ldb, fill), Out(M, N, ldc, 2 * ldc)
            keep = {n: dvec(v) for n, v in use.items()}
            g = gemm_desc(A, lda, Bm, ldb, M, N, K)
            g.C, g.ldc, g.cexp = out.t.data_ptr(), ldc, 1
            for n, v in keep.items():
                setattr(g, n, None if v is None else v.data_ptr())
            _lib.call("linna_gemm_f32", ctx, C.byref(g), st)
            got = out.read()
            out.check(SENT)
            return got
        ref, arg = R.gemm_epilogue_ref(t["A"], t["B"], None, use["cscale"], use["cshift"], 1, use["cpost"], use["cshift2"])
        assert np.abs(arg).max() <= 4.0
        w.add(both(run), ref)
    w.check()


@pytest.mark.parametrize("M,N,K", R.GEMM_EXTRA_SHAPES)
def test_gemm_row_dots(M, N, K):
    """The row-dot partial sums: with `dotwith`, with LINNA_GEMM_DOT_SELF (sum_n C[m][n]^2; dotwith only says "on"), each with
    and without a C store.  Exact table; the slots summed in float64 equal the reference exactly, C bit for bit."""
    ctx, st = env()
    t = R.gemm_dot_table(M, N, K)
    c64 = R.gemm_epilogue_ref(t["A"], t["B"], t["bias"], None, None, 0, None, None)[0]
    slots = _lib.load().linna_gemm_dot_slots(M, N)
    lda, ldb, ldc, ldd = R.ld4(K) + 4, K + 1, R.ld4(N) + 4, N + 1
    for self_, store in ((0, 1), (0, 0), (1, 1), (1, 0)):
        def run(fill):
            A, Bm, dw, bias = dmat(t["A"], lda, fill), dmat(t["B"], ldb, fill), dmat(t["dw"], ldd, fill), dvec(t["bias"])
            out, part = Out(M, N, ldc, 2 * ldc), Out(M, slots)
            g = gemm_desc(A, lda, Bm, ldb, M, N, K)
            g.bias0, g.dotwith, g.lddot, g.dot_partial, g.dot_slots = bias.data_ptr(), dw.data_ptr(), ldd, part.t.data_ptr(), slots
            if store:
                g.C, g.ldc = out.t.data_ptr(), ldc
            g.flags = 0x100 if self_ else 0             # LINNA_GEMM_DOT_SELF
            _lib.call("linna_gemm_f32", ctx, C.byref(g), st)
            gp, gc = part.read(), out.read()
            part.check(SENT)
            if store:
                out.check(SENT)
            else:
                out.untouched()
            return gp, gc
        gp, gc = both(run)
        ref = (c64 * c64).sum(-1) if self_ else (c64 * R.f64(t["dw"])).sum(-1)
        assert np.array_equal(gp.astype(np.float64).sum(-1), ref), "row-dot self %d store %d" % (self_, store)
        if store:
            biteq(gc, c64, "C")


# ----------------------------------------------------------------------------------------------- linna_gauss_loglike_diag
DIAG_LAYOUTS = ("aligned", "odd_ld", "offset")


def run_loglike_diag(D, w, Z, T, layout):
    ctx, st = env()
    B, nout = D.shape
    nin = Z.shape[1]
    ldd, ldz, off = (R.ld4(nout) + 4, R.ld4(nin) + 4, 0) if layout == "aligned" else (nout + 1, nin + 1, 0) if layout == "odd_ld" else (R.ld4(nout) + 4, R.ld4(nin) + 4, 1)

    def run(fill):
        dD, dw, dZ, out = dmat(D, ldd, fill, off), dvec(w, F, off), dmat(Z, ldz, fill, off), Out(1, B)
        _lib.call("linna_gauss_loglike_diag", ctx, ptr(dD), ldd, B, nout, ptr(dw), ptr(dZ), ldz, nin, T, out.p, st)
        got = out.read()[0]
        out.check(SENT)
        return got
    return both(run)


@pytest.mark.parametrize("nout,nin", R.DIAG_SHAPES)
def test_loglike_diag_exact(nout, nin):
    """Every lanes-per-row instantiation on both sides of its switch (max(nout, nin) = 16/17, 32/33, 64/65, 128/129), the
    16-byte and the scalar load path (leading dimension width + 1; base pointers one float off an aligned allocation), row
    counts around the 16 / 64 rows of a wavefront / block.  Exact table, T = 2: bit for bit.  A row with a NaN in D and another
    with a NaN in Z give -inf; the other rows are bit-identical to the clean table's."""
    for B in R.DIAG_B:
        D, w, Z = R.diag_exact_table(nout, nin, B)
        ref = R.loglike_diag_ref(D, w, Z, R.T_EXACT)
        Dn, Zn = D.copy(), Z.copy()
        Dn[0, nout - 1] = np.nan
        Zn[B - 1, nin // 2] = np.nan
        refn = R.loglike_diag_ref(Dn, w, Zn, R.T_EXACT)
        assert np.isneginf(refn[0]) and np.isneginf(refn[B - 1])
        for layout in DIAG_LAYOUTS:
            biteq(run_loglike_diag(D, w, Z, R.T_EXACT, layout), ref, "diag nout %d nin %d B %d %s" % (nout, nin, B, layout))
            biteq(run_loglike_diag(Dn, w, Zn, R.T_EXACT, layout), refn, "diag + NaN rows nout %d nin %d B %d %s" % (nout, nin, B, layout))


@pytest.mark.parametrize("nout,nin", R.DIAG_RANDOM)
def test_loglike_diag_random(nout, nin):
    """One random table per lanes-per-row value against float64, row-wise within the DERIVED bound
    |err| <= (nout + nin + 4) 2^-24 (sum_j |d_j^2 w_j| / (2T) + sum z^2 / 2)  (entries_ref.loglike_diag_bound)."""
    r = R.rng("diagrand", nout, nin)
    B = 257
    D, w, Z = r.standard_normal((B, nout)).astype(F), r.uniform(0.5, 2, nout).astype(F), r.standard_normal((B, nin)).astype(F)
    ref, bound = R.loglike_diag_ref(D, w, Z, 1.5), R.loglike_diag_bound(D, w, Z, 1.5)
    for layout in DIAG_LAYOUTS:
        got = run_loglike_diag(D, w, Z, 1.5, layout)
        assert np.all(np.abs(got - ref) <= bound), "worst %.2f of the bound" % float(np.max(np.abs(got - ref) / bound))


# ----------------------------------------------------------------------------------------------- linna_gauss_loglike_dense
@pytest.mark.parametrize("nout", R.DENSE_NOUT)
def test_loglike_dense_exact(nout):
    """MFMA GEMM D.S fused with the row-dot, then the finishing reduction over the slots; exact table, T = 2, bit for bit; a
    NaN row gives -inf and leaves the others alone; scratch of B * linna_gemm_dot_slots(B, nout) floats plus a guard."""
    ctx, st = env()
    nin = 5
    for B in R.DENSE_B:
        D, S, Z = R.dense_exact_table(nout, nin, B)
        Dn = D.copy()
        Dn[B // 2, 0] = np.nan
        slots = _lib.load().linna_gemm_dot_slots(B, nout)
        ldd, lds, ldz = R.ld4(nout) + 4, R.ld4(nout) + 4, nin + 1
        for Dm in (D, Dn):
            def run(fill):
                dD, dS, dZ, scratch, out = dmat(Dm, ldd, fill), dmat(S, lds, fill), dmat(Z, ldz, fill), Out(B, slots), Out(1, B)
                _lib.call("linna_gauss_loglike_dense", ctx, ptr(dD), ldd, B, nout, ptr(dS), lds, ptr(dZ), ldz, nin, R.T_EXACT, scratch.p, out.p, st)
                got = out.read()[0]
                out.check(SENT)
                scratch.read()
                scratch.check(SENT)
                return got
            ref = R.loglike_dense_ref(Dm, S, Z, R.T_EXACT)
            biteq(both(run), ref, "dense nout %d B %d" % (nout, B))
        assert np.isneginf(ref[B // 2]) and np.isfinite(np.delete(ref, B // 2)).all()


# ----------------------------------------------------------------------------------------------- prior map
def prior_args(t):
    return [dvec(t["is_flat"], np.int32), dvec(t["a1"]), dvec(t["a2"]), dvec(t["lg"], np.int32)]


@pytest.mark.parametrize("nin", R.PRIOR_NIN)
def test_prior_map_fwd(nin):
    """Flat and Gaussian priors, log10 flags on columns of each kind, z over the fixed grid (erf saturated at +-6, +-9), THETA
    NULL and given.  Gaussian non-log columns are algebra only: bit-equal to the float32 restatement (= the float64 reference
    rounded once; the library is built with -ffp-contract=off, no FMA contraction to allow for).  A log10 column with
    theta <= 0 gives NaN, never an infinity.  Columns through erff / log10f: measured-bound rule, scale 1: X worst measured 2.4e-07,
    asserted 1e-06; THETA worst measured 1.1e-07, asserted 5e-07."""
    ctx, st = env()
    wx, wt = Worst("prior_map_fwd X nin %d" % nin, TOL["prior_fwd"], 1.0), Worst("prior_map_fwd THETA nin %d" % nin, TOL["prior_theta"], 1.0)
    for B in R.PRIOR_B:
        t = R.prior_table(nin, B)
        ldz, ldx, ldt = nin + 1, R.ld4(nin) + 4, nin + 3
        x64, th64 = R.prior_fwd_ref(t)
        for theta in (0, 1):
            def run(fill):
                Z, X, TH = dmat(t["Z"], ldz, fill), Out(B, nin, ldx, 2 * ldx), Out(B, nin, ldt, 2 * ldt)
                a = prior_args(t)
                _lib.call("linna_prior_map_fwd", ctx, ptr(Z), ldz, B, nin, ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(dvec(t["xmean"])),
                          ptr(dvec(t["xstd"])), X.p, ldx, TH.p if theta else None, ldt, st)
                gx = X.read()
                X.check(0.0)
                if not theta:
                    TH.untouched()
                    return gx, None
                gt = TH.read()
                TH.check(SENT)
                return gx, gt
            gx, gt = both(run)
            alg = t["algebra"]
            biteq(gx[:, alg], x64[:, alg], "X of the Gaussian non-log columns")
            assert not np.isinf(gx).any() and np.array_equal(np.isnan(gx), np.isnan(x64))
            wx.add(gx[:, ~alg], x64[:, ~alg])
            if theta:
                biteq(gt[:, alg], th64[:, alg], "THETA of the Gaussian non-log columns")
                wt.add(gt[:, ~alg], th64[:, ~alg])
    wx.check(wt)


def test_prior_map_fwd_refuses_short_rows():
    """ldx < nin (and ldz < nin): LINNA_ERR_INVALID on the host, nothing written."""
    ctx, st = env()
    t = R.prior_table(5, 3)
    Z, X, a = dmat(t["Z"], 8, 0.0), Out(3, 8), prior_args(t)
    for ldz, ldx in ((8, 4), (4, 8)):
        rc = rc_of("linna_prior_map_fwd", ctx, ptr(Z), ldz, 3, 5, ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(dvec(t["xmean"])),
                   ptr(dvec(t["xstd"])), X.p, ldx, None, 0, st)
        assert rc == _lib.ERR_INVALID
    X.untouched()


@pytest.mark.parametrize("nin", R.PRIOR_NIN)
def test_prior_map_bwd(nin):
    """dz = dx / xstd * [1 / (theta ln 10)] * dtheta/dz - z against oracle.likelihood.prior_map_grad chained by hand in float64.
    Gaussian non-log columns: bit-equal to the float32 restatement.  dZ is written in its nin columns only (pad columns keep
    the sentinel).  Columns through erff / expf: measured-bound rule, scale 8 = the largest |dx / xstd| of the tables (the
    gradient entering the chain): worst measured 6.3e-08, asserted 3e-07."""
    ctx, st = env()
    w = Worst("prior_map_bwd nin %d" % nin, TOL["prior_bwd"], 8.0)
    for B in R.PRIOR_B:
        t = R.prior_table(nin, B)
        ldz, lddx, lddz = nin + 1, R.ld4(nin) + 4, nin + 3
        ref = R.prior_bwd_ref(t)
        assert np.abs(R.f64(t["dX"]) / R.f64(t["xstd"])[None, :]).max() <= 8.0

        def run(fill):
            Z, dX, dZ, a = dmat(t["Z"], ldz, fill), dmat(t["dX"], lddx, fill), Out(B, nin, lddz, 2 * lddz), prior_args(t)
            _lib.call("linna_prior_map_bwd", ctx, ptr(Z), ldz, B, nin, ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), ptr(dvec(t["xstd"])),
                      ptr(dX), lddx, dZ.p, lddz, st)
            g = dZ.read()
            dZ.check(SENT)
            return g
        got = both(run)
        alg = t["algebra"]
        biteq(got[:, alg], ref[:, alg], "dZ of the Gaussian non-log columns")
        biteq(got[:, alg], R.prior_bwd_f32(t)[:, alg], "dZ against the float32 restatement")
        assert np.array_equal(np.isfinite(got), np.isfinite(ref))
        w.add(got[:, ~alg], ref[:, ~alg])
    w.check()


# ----------------------------------------------------------------------------------------------- gather + transforms
@pytest.mark.parametrize("nin", R.XFORM_W)
def test_gather_xform(nin):
    """XB[i] = (X[rows[i]] (log10 on flagged columns) - mean) / std: ROWS NULL, a permutation, repeats ending in the last row
    of the set.  Plain columns bit-equal; XB pad columns zero.  log10 columns: measured-bound rule, scale 1:
    worst measured 7.7e-08, asserted 4e-07."""
    ctx, st = env()
    w = Worst("gather_xform nin %d" % nin, TOL["gather_log"], 1.0)
    for B in R.XFORM_B:
        t = R.gather_table(B, nin)
        ldx, ldxb = nin + 1, R.ld4(nin) + 4
        for name, rows in R.rows_tables(B, t["ntot"]).items():
            def run(fill):
                X, XB = dmat(t["X"], ldx, fill), Out(B, nin, ldxb, 2 * ldxb)
                _lib.call("linna_gather_xform", ctx, ptr(X), ldx, ptr(dvec(rows, np.int32)), B, nin, ptr(dvec(t["lg"], np.int32)),
                          ptr(dvec(t["xmean"])), ptr(dvec(t["xstd"])), XB.p, ldxb, st)
                g = XB.read()
                XB.check(0.0)
                return g
            got, ref = both(run), R.gather_xform_ref(t, rows)
            plain = t["lg"] == 0
            biteq(got[:, plain], ref[:, plain], "plain columns, rows %s" % name)
            w.add(got[:, ~plain], ref[:, ~plain])
    w.check()


def loss_desc(c, ylog=0, keep=None):
    """linna_loss_desc_t over device copies of the constants; Cinv rows zero-padded to ldc (the caller's duty)."""
    ldc = R.ld4(c["nout"]) + 4
    dev = dict(sigma=dvec(c["sigma"]), ymean=dvec(c["ymean"]), ystd=dvec(c["ystd"]), dn=dvec(c["dn"]), Cinv=dmat(c["Cinv"], ldc, 0.0))
    d = _lib.LossDesc()
    d.nout, d.ldc, d.ylog = c["nout"], ldc, ylog
    d.sigma, d.ymean, d.ystd, d.data_norm, d.Cinv = (dev[k].data_ptr() for k in ("sigma", "ymean", "ystd", "dn", "Cinv"))
    d._keep = dev
    return d


@pytest.mark.parametrize("nout", R.XFORM_W)
def test_loss_targets(nout):
    """YN = ((y / sigma) - ymean) / ystd, NaN where the element is masked (both sentinels 1e10, 1e-30 and a masked data_norm
    column), pad columns zero.  ylog = 0 on the exact constants: bit-equal.  ylog = 1 (log(y / sigma)): measured-bound rule,
    scale 1: worst measured 1.0e-07, asserted 4e-07."""
    ctx, st = env()
    w = Worst("loss_targets ylog nout %d" % nout, TOL["targets_log"], 1.0)
    for B in R.XFORM_B:
        n = B + 3
        for ylog in (0, 1):
            c = R.loss_consts(nout, "random" if ylog else "exact")
            Y = R.loss_Y(("targets", B, nout), n, nout)
            if ylog:
                Y = np.where((Y == F(1e10)) | (Y == F(1e-30)), Y, (np.abs(Y) + 1) * F(1.25)).astype(F)
            ldy, ldyn = nout + 1, R.ld4(nout) + 4
            d = loss_desc(c, ylog)

            def run(fill):
                dY, YN = dmat(Y, ldy, fill), Out(n, nout, ldyn, 2 * ldyn)
                _lib.call("linna_loss_targets", ctx, C.byref(d), ptr(dY), ldy, n, YN.p, ldyn, st)
                g = YN.read()
                YN.check(0.0)
                return g
            got, ref = both(run), R.loss_targets_ref(c, Y, ylog)
            assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(got[1, 0]) and np.isnan(got[2, nout - 1])
            assert nout < 2 or np.isnan(got[:, 1]).all()
            if ylog:
                w.add(got, ref)
            else:
                biteq(got, ref, "YN")
    w.check()


# ----------------------------------------------------------------------------------------------- chi2-ratio loss
LOSS_NOUT = (1, 3, 63, 64, 65, 130)
LOSS_B = (1, 4, 5, 257)


def scratch_for(B, nout):
    return Out(1, _lib.load().linna_loss_scratch_bytes(B, nout) // 4)


def run_chi2_md(c, Y):
    ctx, st = env()
    n, nout = Y.shape
    ldy = nout + 1
    d = loss_desc(c)

    def run(fill):
        dY, scratch, den = dmat(Y, ldy, fill), scratch_for(n, nout), Out(1, n)
        _lib.call("linna_chi2_md", ctx, C.byref(d), ptr(dY), ldy, n, scratch.p, den.p, st)
        g = den.read()[0]
        den.check(SENT)
        scratch.read()
        scratch.check(SENT)
        return g
    return both(run)


@pytest.mark.parametrize("nout", LOSS_NOUT)
def test_chi2_md(nout):
    """den = max(chisqMd, nout / 2).  With Cinv = I / 2: rows whose chi2 lies below (0 and (nout - 1) / 2), at (nout / 2) and
    above (2 nout) the floor -- below it the result is exactly the floor.  With the full exact Cinv and the sentinels in Y and in
    data_norm: bit for bit against oracle.training.aux."""
    c = R.loss_consts(nout, "exact", "diag")
    assert run_chi2_md(c, R.floor_Y(c).astype(F)).tolist() == [0.5 * nout, 0.5 * nout, 2.0 * nout, 0.5 * nout]
    c = R.loss_consts(nout, "exact")
    for B in LOSS_B:
        Y = R.loss_Y(("md", B, nout), B, nout)
        biteq(run_chi2_md(c, Y), R.chi2_md_ref(c, Y), "den nout %d B %d" % (nout, B))


def rel_max(got, ref):
    """The metric tools/fuzz_moves_loss.py asserts below 2e-4: max|got - ref| / (max|ref| + 1e-12)."""
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (np.abs(ref).max() + 1e-12))


@pytest.mark.parametrize("nout", LOSS_NOUT)
def test_val_rows(nout):
    """Per-row loss and |chisq_nnd / chisq_Md - 1| against oracle.training.aux (the rows behind val_metric).  Exact table: both
    chi2 sums are exact, so loss = chi2 / den is the float64 quotient rounded once (bit for bit; division double-rounds
    innocuously from 53 to 24 bits) and frac equals its float32 restatement |chi2 / den - 1| on the exact chi2.  Random
    table: the 2e-4 relative bound tools/fuzz_moves_loss.py asserts."""
    ctx, st = env()
    for kind in ("exact", "random"):
        c = R.loss_consts(nout, kind)
        d = loss_desc(c)
        for B in LOSS_B:
            Y = R.loss_Y(("valrows", B, nout, kind), B, nout, kind)
            pred = R.ints(("valpred", B, nout), (B, nout), 2) if kind == "exact" else R.rng("valpred", B, nout).standard_normal((B, nout)).astype(F)
            den = R.round_once(R.chi2_md_ref(c, Y))
            ldp, ldy = R.ld4(nout) + 4, nout + 1

            def run(fill):
                P, dY, scratch, lr, fr = dmat(pred, ldp, fill), dmat(Y, ldy, fill), scratch_for(B, nout), Out(1, B), Out(1, B)
                _lib.call("linna_val_rows", ctx, C.byref(d), ptr(P), ldp, ptr(dY), ldy, ptr(dvec(den)), B, scratch.p, lr.p, fr.p, st)
                gl, gf = lr.read()[0], fr.read()[0]
                lr.check(SENT)
                fr.check(SENT)
                scratch.read()
                scratch.check(SENT)
                return gl, gf
            gl, gf = both(run)
            rl, rf = R.val_rows_ref(c, pred, Y)
            if kind == "exact":
                biteq(gl, rl, "loss rows nout %d B %d" % (nout, B))
                cnnd = R.round_once(R.loss_aux(c, pred, Y)[2])
                assert np.array_equal(bits(gf), bits(np.abs(cnnd / den - F(1))))
            assert rel_max(gl, rl) < 2e-4 and rel_max(gf, rf) < 2e-4


@pytest.mark.parametrize("nout", LOSS_NOUT)
def test_chi2_ratio_loss_fwd_bwd(nout):
    """loss_b = chi2 / den[r], L = inv_batch sum_b loss_b, dPRED = -2 (delta Cinv) inv_batch / den[r] against
    oracle.training.aux / loss / loss_grad, on both sides of the 64 / 65 switch between the one-launch and the five-launch
    form, ROWS NULL / a permutation / repeats, loss_mean and dPRED each NULL or given.  Exact table: loss rows bit for bit,
    dPRED bit-equal to the float32 restatement (-2 U) inv_batch / den on the exact U, a masked element exactly 0, pad columns
    zero.  The batch mean, and everything on the random table: the 2e-4 relative bound of tools/fuzz_moves_loss.py.
    (lddp = LINNA_LD(nout) + 4 is 68 for nout = 63, 64 -- past the 64 lanes of the one-launch kernel's wave, which left those pad
    columns unwritten until this test: loss_fused_small_kernel now zeroes them like loss_grad_kernel.)"""
    ctx, st = env()
    for kind in ("exact", "random"):
        c = R.loss_consts(nout, kind)
        d = loss_desc(c)
        for B in LOSS_B:
            ntot = B + 3
            Y = R.loss_Y(("loss", B, nout, kind), ntot, nout, kind)
            pred = R.ints(("losspred", B, nout), (B, nout), 2) if kind == "exact" else R.rng("losspred", B, nout).standard_normal((B, nout)).astype(F)
            den = R.round_once(R.chi2_md_ref(c, Y))
            inv_b = F(1.0 / B)
            ldp, ldy, lddp = R.ld4(nout) + 4, nout + 1, R.ld4(nout) + 4
            for k, (name, rows) in enumerate(R.rows_tables(B, ntot).items()):
                want_mean, want_grad = k != 1, k != 2
                Yb = Y[:B] if rows is None else Y[rows]
                denb = den[:B] if rows is None else den[rows]

                def run(fill):
                    P, dY, scratch = dmat(pred, ldp, fill), dmat(Y, ldy, fill), scratch_for(B, nout)
                    lr, lm, dP = Out(1, B), Out(1, 1), Out(B, nout, lddp, 2 * lddp)
                    _lib.call("linna_chi2_ratio_loss_fwd_bwd", ctx, C.byref(d), ptr(P), ldp, ptr(dY), ldy, ptr(dvec(den)), ptr(dvec(rows, np.int32)),
                              B, scratch.p, lr.p, lm.p if want_mean else None, dP.p if want_grad else None, lddp, float(inv_b), st)
                    gl, gm, gp = lr.read()[0], lm.read()[0, 0], dP.read()
                    lr.check(SENT)
                    lm.check(SENT)
                    scratch.read()
                    scratch.check(SENT)
                    if want_grad:
                        dP.check(0.0)
                    else:
                        assert np.all(gp == SENT)
                    assert want_mean or gm == SENT
                    return gl, np.asarray([gm], F), gp
                gl, gm, gp = both(run)
                l64, _, _, delta, notmask = R.loss_aux(c, pred, Yb)
                _, g64 = R.loss_grad_ref(c, pred, Yb)
                if kind == "exact":
                    biteq(gl, l64, "loss rows nout %d B %d rows %s" % (nout, B, name))
                    if want_grad:
                        U = R.round_once(delta @ R.f64(c["Cinv"]))
                        f32 = np.where(notmask, (F(-2) * U) * inv_b / denb[:, None], F(0)).astype(F)
                        assert np.array_equal(bits(gp), bits(f32)), "dPRED nout %d B %d rows %s" % (nout, B, name)
                assert rel_max(gl, l64) < 2e-4
                if want_mean:
                    assert rel_max(gm, np.array([l64.mean()])) < 2e-4
                if want_grad:
                    assert rel_max(gp, g64) < 2e-4 and np.all(gp[~notmask] == 0)


# ----------------------------------------------------------------------------------------------- AdamW
def run_adamw(p, g, m, v, lr, wd, step, prepared, hyper23=(0.0, 0.0)):
    ctx, st = env()
    n = len(p)
    P, M, V = Out(1, n), Out(1, n), Out(1, n)
    for o, a in ((P, p), (M, m), (V, v)):
        o.t[:n] = torch.as_tensor(np.asarray(a, F), device="cuda")
    hyper = Out(1, 4)
    hyper.t[:4] = torch.as_tensor(np.array([lr, wd, hyper23[0], hyper23[1]], F), device="cuda")
    sd = torch.as_tensor(np.array([step, 12345], np.int32), device="cuda")
    _lib.call("linna_adamw_step", ctx, P.p, ptr(dvec(g)), M.p, V.p, n, hyper.p, ptr(sd), float(R.BETA1), float(R.BETA2), float(R.EPS), prepared, st)
    res = [o.read()[0] for o in (P, M, V, hyper)]
    for o in (P, M, V, hyper):
        o.check(SENT)
    sdh = sd.cpu().numpy()
    assert sdh[1] == 12345
    return res + [int(sdh[0])]


@pytest.mark.parametrize("n", R.ADAMW_N)
def test_adamw_step(n):
    """torch.optim.AdamW against oracle.training.adamw_step in float64 (on the float32 beta1 / beta2 / eps / lr the device gets):
    three consecutive steps from a zero state, weight_decay 0 and 1e-4, one step with step_dev preset to 9999, and prepared = 1
    (neither step_dev nor hyper[2..3] advance).  hyper[2], hyper[3] = float32(1 - b1^t), float32(sqrt(1 - b2^t)) computed in
    float64: BIT FOR BIT (not 1 ulp: the device's double-precision pow and sqrt round to the same float32 at t = 1, 2, 3 and
    10000).  m and v (two and three fp32 operations): within 4 ulp of the result (measured 1.5 and 1.6 ulp).  An element with
    g = m = v = 0 moves by the decay alone.  p, measured-bound rule, scale = lr (the size of one update): worst measured
    1.3e-07, asserted 6e-07."""
    p0, g = R.adamw_table(n)
    w = Worst("adamw p n %d" % n, TOL["adamw_p"], float(R.LR))
    for wd in (0.0, 1e-4):
        p, m, v = p0.copy(), np.zeros(n, F), np.zeros(n, F)
        for step in (1, 2, 3):
            rp, rm, rv = R.adamw_ref(p, g[step - 1], m, v, step, R.LR, wd)
            p, m, v, hyper, sd = run_adamw(p, g[step - 1], m, v, R.LR, wd, step - 1, 0)
            assert sd == step and hyper[0] == R.LR and hyper[1] == F(wd)
            assert bit1(hyper[2:4]) == bit1(R.adamw_bc(step))
            assert R.ulps(m, rm).max() <= 4 and R.ulps(v, rv).max() <= 4, (R.ulps(m, rm).max(), R.ulps(v, rv).max())
            if MEASURE:
                print("MEASURED adamw n %d step %d: m %.2f ulp, v %.2f ulp" % (n, step, R.ulps(m, rm).max(), R.ulps(v, rv).max()))
            w.add(p, rp)
            assert m[0] == 0 and v[0] == 0
        decay = F(1) - R.LR * F(wd)
        assert bit1([p[0]]) == bit1([((p0[0] * decay) * decay) * decay])
    # a late step: the bias corrections at t = 10000
    rp, rm, rv = R.adamw_ref(p0, g[1], np.zeros(n, F), np.zeros(n, F), 10000, R.LR, 1e-4)
    p, m, v, hyper, sd = run_adamw(p0, g[1], np.zeros(n, F), np.zeros(n, F), R.LR, 1e-4, 9999, 0)
    assert sd == 10000 and bit1(hyper[2:4]) == bit1(R.adamw_bc(10000))
    assert R.ulps(m, rm).max() <= 4 and R.ulps(v, rv).max() <= 4
    w.add(p, rp)
    # prepared = 1: the caller's step counter and bias corrections are used as they are
    bc = R.adamw_bc(2)
    rp, rm, rv = R.adamw_ref(p0, g[0], np.zeros(n, F), np.zeros(n, F), 2, R.LR, 1e-4)
    p, m, v, hyper, sd = run_adamw(p0, g[0], np.zeros(n, F), np.zeros(n, F), R.LR, 1e-4, 2, 1, bc)
    assert sd == 2 and bit1(hyper[2:4]) == bit1(bc)
    assert R.ulps(m, rm).max() <= 4 and R.ulps(v, rv).max() <= 4
    w.add(p, rp)
    w.check()


def test_adamw_step_refuses_null_pointers():
    """A null pointer: LINNA_ERR_INVALID on the host (api.hip: the first statement of the entry), nothing written."""
    ctx, st = env()
    bufs = [Out(1, 5) for _ in range(5)]
    sd = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k in range(6):
        a = [b.p for b in bufs] + [ptr(sd)]
        a[k] = None
        assert rc_of("linna_adamw_step", ctx, a[0], a[1], a[2], a[3], 5, a[4], a[5], 0.9, 0.999, 1e-8, 0, st) == _lib.ERR_INVALID
    for b in bufs:
        b.untouched()
    assert int(sd.cpu()[0]) == 0


# The measured-bound rule's tolerances: 4 x the worst error measured on an MI355X against the float64 reference (the figures
# in the docstrings), rounded up to one significant digit.  All of them sit below 64 ulp (3.8e-06) of their scale.
TOL = {
    "gemm_exp": 8e-7,
    "prior_fwd": 1e-6,
    "prior_theta": 5e-7,
    "prior_bwd": 3e-7,
    "gather_log": 4e-7,
    "targets_log": 4e-7,
    "adamw_p": 6e-7,
}
