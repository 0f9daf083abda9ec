"""GPU: the whole-network kernel (csrc/net_stream.hip, net_stream_body.inc, the planner net_program.hip and the weight
re-layout ns_pack_kernel) BIT FOR BIT against the integer references of tests/net_exact.py, on exact integer tables
(tests/test_net_exact_host.py pins the tables' conditions, the references against the oracle and every shape's planner edge
on the CPU).  No tolerance anywhere: ``np.array_equal`` on every surface, no row, column or table left out -- zero is exact
here, so there is no ReLU-kink exemption -- and every table's lnP meets the exactness condition (no derived-bound fallback).

Surfaces:
 * the training forward (STORE instantiation): the output and every stored activation of the workspace;
 * the one-launch dX chain (down to op 1 and down to the input): dX, every d/d(input) and d/dh of the backward workspace, and
   every parameter gradient computed from them;
 * serving: lnP and THETA on the engines of 4, 8 and 16 rows and the automatic choice, the plain instantiation on and off, a
   diagonal likelihood, a dense one in the factored form under linna_dense_tri 0 / 1 / 2 and in the direct form;
 * the one-launch gradient (the fused MLP form and the any-network form) and the fused leapfrog: lnP, G, P, Q;
 * cross-engine equality: a failure there points at an engine without needing the reference.
Conventions of tests/test_gpu_entries.py: outputs pre-filled with the sentinel and one guard row longer, row strides padded,
input pads NaN, every launch repeated with zero pads.

Shapes (net_exact.NETS): the smallest at which each mechanism of ns_shape / ns_lower can go wrong -- K tails and first-layer
padding (1, 15, 16, 17, 64, 65, 256 inputs; hidden K of 16, 17, 1000), column groups (N of 1 ... 257, 512, 513, 1024), the
SPLIT / WIDE choice, SIDE segments of kc 4 / 2 / 1 with one and two steps and one past, residual blocks (ChtoModelv2,
ChtoModelsimple, custom C of 1, 16, 17, 64, the identity skip K == N that no model class reaches), dense likelihoods of 16 ...
1024 columns, the gradient gates of 257 / 513 wide hidden layers; batches of 1, 3, 5, 9, 17, 33 and 20 rows.
Left to its existing tolerance test: the input-skip network (ChtoModelv2_linear, its 1e-3 fold), the layer-by-layer paths.
The bf16 engines and the merged training step's loss: tests/test_gpu_net_exact_bf16.py, the same technique.

Wall time of the module on an MI355X, measured: 153 cases in 19.4 s, the ten networks on the bf16 planner's edges among them,
which run here in fp32 too (the slowest: ChtoModelv2(33, 33) through serving, 1.2 s, and ChtoModelv2(26, 457) through the
training forward and the dX chain, 1.1 s).
"""
import numpy as np
import pytest

import entries_ref as er
import net_exact as ne
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
NAN = float("nan")
SENT = er.SENTINEL
FILLS = (NAN, 0.0)


@pytest.fixture(autouse=True)
def _restore_switches():
    """engine_rows, serve_plain and dense_tri are process wide: put back what the test found."""
    lib = _lib.load()
    rows, plain, tri = _lib.engine_rows(0), _lib.serve_plain(1), lib.linna_dense_tri(-1)
    _lib.engine_rows(rows)
    _lib.serve_plain(plain)
    yield
    _lib.engine_rows(rows)
    _lib.serve_plain(plain)
    lib.linna_dense_tri(tri)


def f32(ref64):
    """The float64 reference as float32; it is exact (asserted on the CPU), so this rounds nothing."""
    a = np.asarray(ref64, np.float64).astype(F)
    assert np.array_equal(a.astype(np.float64), ref64)
    return a


def padded(a, fill):
    """[rows][ld4(w) + 4] device buffer holding ``a`` with ``fill`` in the pad columns, and its [rows, w] view."""
    a = np.asarray(a, F)
    host = np.full((a.shape[0], _lib.ld4(a.shape[1]) + 4), fill, F)
    host[:, :a.shape[1]] = a
    buf = torch.as_tensor(host, device="cuda")
    return buf, buf[:, :a.shape[1]]


class Out(object):
    """An output matrix [rows][ld4(w) + 4] with one guard row, all sentinel."""

    def __init__(self, rows, w):
        self.rows, self.w = rows, w
        self.t = torch.full((rows + 1, _lib.ld4(w) + 4), SENT, device="cuda")

    def read(self):
        """The [rows, w] block; the guard row and the columns from ld4(w) on must hold the sentinel."""
        host = self.t.cpu().numpy()
        assert np.all(host[self.rows] == SENT), "wrote past the last row of an output"
        assert np.all(host[:, _lib.ld4(self.w):] == SENT), "wrote past the row of an output"
        return host[:self.rows, :self.w].copy()


def same(got, ref64, what):
    ref = f32(ref64)
    if not np.array_equal(got, ref):
        bad = np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, expected %r" % (what, len(bad), ref.size, i, got[i], ref[i]))


def load(model, P):
    model.load_state_dict({k: torch.as_tensor(v) for k, v in P.items()})


# ----------------------------------------------------------------------------------------------- training forward + dX chain
def run_training_table(model, name, dense, B, tag):
    t = ne.table(name, dense, B)
    ops, nout = t["ops"], model.out_size
    lay_f, tot_f = ne.fwd_layout(ops, B)
    lay_b, tot_b = ne.bwd_layout(ops, B)
    for fill in FILLS:
        xbuf, _ = padded(t["x"], fill)
        out = Out(B, nout)
        ws = model.workspace(B)
        ws.fill_(SENT)
        model.forward_buffer(xbuf, B, out=out.t)
        same(out.read(), t["fwd"][-1]["y"], tag + " forward output")
        w = ws.cpu().numpy()
        for (i, what, off, ld, cols) in lay_f:
            same(w[off:off + B * ld].reshape(B, ld)[:, :cols], t["fwd"][i][what], "%s stored %s of op %d" % (tag, what, i))
        assert np.all(w[tot_f:] == SENT), tag + ": wrote past the forward workspace"
        assert model.stream_state()[0] == 1, tag + ": the forward did not run as one launch"
        dbuf, dview = padded(t["dY"], fill)
        for need_dx in (True, False):
            bws = model.workspace(B, "bwd")
            bws.fill_(SENT)
            model.flat_grads().fill_(SENT)
            dx = model.backward(dview, param_grads=True, need_dx=need_dx)
            state = model.stream_state()
            assert state[2 if need_dx else 1] == 1, "%s: the dX chain (need_dx=%s) did not run as one launch: %r" % (tag, need_dx, state)
            if need_dx:
                same(dx.cpu().numpy(), t["dX"], tag + " dX")
            w = bws.cpu().numpy()
            for (i, what, off, ld, cols) in lay_b:
                same(w[off:off + B * ld].reshape(B, ld)[:, :cols], t["bufs"][i][what], "%s %s of op %d (need_dx=%s)" % (tag, what, i, need_dx))
            assert np.all(w[tot_b:] == SENT), tag + ": wrote past the backward workspace"
            for k, g in model.grad_dict().items():
                same(g.cpu().numpy(), t["G"][k], "%s gradient of %s (need_dx=%s)" % (tag, k, need_dx))


@pytest.mark.parametrize("name", list(ne.NETS))
def test_training_forward_and_dx_chain(name):
    """model.forward (STORE) and model.backward (the one-launch dX chain + the parameter gradients it feeds): every dense map
    on the engine the batch selects, the first and the last dense map at every batch size on each engine."""
    model = ne.fresh_model(name).to("cuda")
    n = ne.n_maps(name)
    for dense in range(n):
        load(model, ne.weights(name, dense))
        _lib.engine_rows(0)
        run_training_table(model, name, dense, ne.ROWS, "%s dense map %d rows %d" % (name, dense, ne.ROWS))
        if dense in (0, n - 1):
            for rows in ne.ENGINES:
                _lib.engine_rows(rows)
                for B in ne.BATCH_ROWS:
                    run_training_table(model, name, dense, B, "%s dense map %d rows %d engine %d" % (name, dense, B, rows))


# ----------------------------------------------------------------------------------------------- serving
def build_logprob(name, kind="diag"):
    from linna_amd import predictor_gpu, util
    c = ne.serving_consts(name, kind)
    t = lambda a: torch.as_tensor(np.asarray(a, F))
    Xt = util.X_transform_class(t(c["X_mean"]), t(c["X_std"]), "cpu", None)
    Yt = util.Y_transform_class(t(c["y_mean"]), t(c["y_std"]), "cpu", ypositive=False)
    pred = predictor_gpu.Predictor(c["nin"], c["nout"], model=ne.fresh_model(name), X_transform=Xt, y_transform=Yt, device="cuda")
    yinv = util.Y_invtransform_data(np.asarray(c["sigma"], F), "cpu")
    lp = util.Log_prob(t(c["data"]), t(c["invcov"]), pred, yinv, util.Transform(c["priors"]), c["T"], util.gaussianlogliklihood, nograd=True)
    lp._ensure()
    return lp, pred.model


def serve(lp, z, fill, theta):
    """(lnP[B], THETA[B, nin] or None) of one evaluate call on padded, guarded buffers."""
    B, nin = z.shape
    _, zview = padded(z, fill)
    lnp = torch.full((B + 8,), SENT, device="cuda")
    th = Out(B, nin) if theta else None
    lp.evaluate(zview, out=lnp[:B], theta=th.t if theta else None)
    host = lnp.cpu().numpy()
    assert np.all(host[B:] == SENT), "wrote past the end of lnP"
    return host[:B].copy(), (th.read() if theta else None)


def run_serving_table(lp, s, tag, plain_net):
    ref, z = s["ref"], s["z"]
    first = None
    for rows in (0,) + ne.ENGINES:
        _lib.engine_rows(rows)
        for fill in FILLS:
            lnp, th = serve(lp, z, fill, True)
            same(th, ref["theta"], "%s engine %d THETA" % (tag, rows))
            same(lnp, ref["lnP"], "%s engine %d lnP (with THETA)" % (tag, rows))
            for plain in (1, 0):
                _lib.serve_plain(plain)
                if rows == 16:
                    assert lp.serves_plain(len(z)) is bool(plain and plain_net), tag
                lnp, _ = serve(lp, z, fill, False)
                same(lnp, ref["lnP"], "%s engine %d plain %d lnP" % (tag, rows, plain))
                if first is None:
                    first = lnp
                assert np.array_equal(lnp, first), "%s: engine %d plain %d differs from the first engine" % (tag, rows, plain)
            _lib.serve_plain(1)


@pytest.mark.parametrize("name", [n for n in ne.NETS if n not in ne.DENSE_NETS])
def test_serving_diagonal(name):
    """Log_prob.evaluate, lnP and THETA, diagonal likelihood: every dense map at ROWS rows and the first and last one at every
    batch size, on each engine and the automatic choice, the plain instantiation on and off."""
    lp, model = build_logprob(name)
    for dense, B in ne.sweep_tables(name):
        s = ne.serving_table(name, dense, B, grad=name in ne.GRAD_NETS)
        load(model, s["P"])
        run_serving_table(lp, s, "%s dense map %d rows %d" % (name, dense, B), name in ne.PLAIN_NETS)


@pytest.mark.parametrize("name", ne.DENSE_NETS)
def test_serving_dense(name, monkeypatch):
    """A dense inverse covariance S = L L^T as the program's last segment: the factored form (chi^2 = |d L|^2) under
    linna_dense_tri 0, 1 and 2 and, for the widths whose double sum stays exact, the direct form (chi^2 = d S d^T).  The
    switches are read when the object is created."""
    lib = _lib.load()
    forms = [("tri%d" % m, m) for m in (0, 1, 2)] + ([("direct", None)] if name in ne.DIRECT_NETS else [])
    base = {}
    for form, mode in forms:
        if mode is None:
            monkeypatch.setenv("LINNA_DENSE_FACTORED", "0")
        else:
            lib.linna_dense_tri(mode)
        lp, model = build_logprob(name, "dense")
        assert ("Sfac" in lp._plan["keep"]) is (mode is not None)
        for dense, B in ne.dense_sweep(name):
            s = ne.serving_table(name, dense, B, kind="dense")
            load(model, s["P"])
            for rows in (0,) + ne.ENGINES:
                _lib.engine_rows(rows)
                for fill in FILLS:
                    tag = "%s %s dense map %d rows %d engine %d" % (name, form, dense, B, rows)
                    lnp, th = serve(lp, s["z"], fill, True)
                    same(th, s["ref"]["theta"], tag + " THETA")
                    same(lnp, s["ref"]["lnP"], tag + " lnP")
                    assert np.array_equal(lnp, base.setdefault((dense, B), lnp)), tag + ": differs from the first form / engine"
        if mode is None:
            monkeypatch.delenv("LINNA_DENSE_FACTORED")


# ----------------------------------------------------------------------------------------------- one-launch gradient, leapfrog
@pytest.mark.parametrize("name", ne.GRAD_NETS)
def test_gradient_and_leapfrog(name):
    """evaluate_with_grad (lnP, G) and linna_logprob_grad_leapfrog (P, Q) in one launch: the fused MLP gradient where the
    hidden layers are WIDE (grad257, grad513, n512_513, n1000_1024), the any-network form elsewhere
    (tests/test_net_exact_host.py pins which); each engine."""
    lp, model = build_logprob(name)
    nin = model.in_size
    mass = torch.as_tensor(ne.MASS(nin).astype(F), device="cuda")
    for dense, B in ne.sweep_tables(name):
        s = ne.serving_table(name, dense, B, grad=True)
        ref, z = s["ref"], s["z"]
        load(model, s["P"])
        P0 = ne.momenta(name, dense, B)
        Pn, Qn = ne.leapfrog_ref(ref["G"], z, P0, ne.MASS(nin), ne.EPS, ne.EPS)
        first = None
        for rows in ((0,) + ne.ENGINES if B == ne.ROWS else ne.ENGINES):
            _lib.engine_rows(rows)
            for fill in FILLS:
                tag = "%s dense map %d rows %d engine %d" % (name, dense, B, rows)
                _, zview = padded(z, fill)
                lnp, G = torch.full((B + 8,), SENT, device="cuda"), Out(B, nin)
                lp.evaluate_with_grad(zview, out=lnp[:B], grad=G.t)
                g = G.read()
                same(g, ref["G"], tag + " G")
                host = lnp.cpu().numpy()
                assert np.all(host[B:] == SENT)
                same(host[:B], ref["lnP"], tag + " lnP")
                first = g if first is None else first
                assert np.array_equal(g, first), tag + ": G differs from the first engine"
                # the leapfrog: Q and P are updated in place
                qbuf, qview = padded(z, fill)
                pbuf, pview = padded(P0, fill)
                lnp, G = torch.full((B + 8,), SENT, device="cuda"), Out(B, nin)
                p = lp._ensure()
                _lib.call("linna_logprob_grad_leapfrog", p["handle"], _lib.ptr(qbuf), qbuf.stride(0), B, _lib.ptr(lp._workspace(B, True)),
                          _lib.ptr(lnp), _lib.ptr(G.t), G.t.stride(0), _lib.ptr(pbuf), pbuf.stride(0), _lib.ptr(mass), ne.EPS, ne.EPS,
                          _lib.stream())
                same(G.read(), ref["G"], tag + " leapfrog G")
                same(lnp.cpu().numpy()[:B], ref["lnP"], tag + " leapfrog lnP")
                same(pview.cpu().numpy(), Pn, tag + " leapfrog P")
                same(qview.cpu().numpy(), Qn, tag + " leapfrog Q")
                pads = qbuf.cpu().numpy()[:, nin:]
                assert np.all(np.isnan(pads)) if fill != fill else np.all(pads == fill), tag + ": the leapfrog wrote the pads of Q"
