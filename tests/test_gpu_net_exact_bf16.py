"""GPU: the three bf16 forms of the whole-network kernel -- serving (linna_logprob_set_precision), the one-launch gradient
and leapfrog (linna_logprob_set_grad_precision), the merged training step (linna_net_set_train_precision) -- and the merged
training step's loss in fp32, BIT FOR BIT against the rounding references of tests/net_exact.py on exact integer tables.

The technique of tests/test_gpu_net_exact.py carried to bf16: the integer tables make every fp32 partial sum exact, so every
value a bf16 engine rounds is known exactly, round-to-nearest-even of it is deterministic, and a float64 reference that rounds
where include/linna_hip.h says the engine rounds (net_exact.Bf16Hook in forward_ref / backward_ref / serving_ref) equals the GPU
with ``np.array_equal`` -- no tolerance, no rms, no row, column or table left out.  tests/test_net_exact_host.py pins on the
CPU that every table meets the exactness condition on its ROUNDED operands, that the serving tables round nothing (so lnP and
THETA are the fp32 integer reference's), that gradient and training tables do round, ties among them, and every new shape's
planner edge.  What the statistical tests (test_gpu_bf16*.py) cannot see and this module does: a wrong slot at the K tail of
a 32-k step or a column group off by one, on every table; a delta rounded at the wrong place, truncation on a tie, a gate from
the unrounded forward, on the tables whose deltas round -- the training step's loss tables on every network it runs, the
gradient tables of the sixteen networks the host test's GRAD_ROUNDS names (the others' backward operands are bf16 numbers).

Surfaces:
 * serving on a bf16 object: lnP and THETA on the engines of 4, 8 and 16 rows and the automatic choice, linna_logprob_eval_if
   (a launch gated off leaves its rows' sentinel), linna_logprob_eval_slice_points with integer directions and weights that
   form the table's z in the prologue; the object's precision is read back (a silent fp32 fallback would pass every equality);
 * the bf16 one-launch gradient: lnP, G, and P, Q of linna_logprob_grad_leapfrog and linna_logprob_grad_leapfrog_eps (a
   power-of-two step size per row); the refusal of a network without such a program;
 * the merged training step (linna_net_train_step, linna_net_train_step_update) in fp32 and in bf16: loss rows, batch mean,
   PRED, the gathered batch, d loss / d pred, every stored activation and delta of both workspaces, every parameter gradient;
   parameters and moments after the update entry's AdamW against linna_adamw_step on the same gradients.
Conventions of tests/test_gpu_net_exact.py: outputs pre-filled with the sentinel and one guard row longer, row strides padded,
input pads NaN, every launch repeated with zero pads, process-wide switches restored by a fixture.

Shapes: every non-dense network of net_exact.NETS, ten of them added for the bf16 planner's own edges (32 k per step: hidden
K of 31 and 63, [x ; h] of a residual block at 63 / 64 / 65 k, 64 / 32 / 16 columns behind K = 256 / 257 / 512 / 513 / 1024, SPLIT
against WIDE at 4 and 3 steps); the gradient on the 41 networks of up to 64 inputs and outputs, the training step on 20.
The launch owns the whole row stride of the gathered batch and of d loss / d pred (zeros behind the columns: the parameter-
gradient launch reads padded matrices); those two are checked as that, every other output with untouched pads.

Wall time of the module on an MI355X, measured: 128 cases in 21.3 s (44 serving, 41 gradient, 3 refusal and 40
training-step cases; the slowest, ChtoModelv2(26, 457) through bf16 serving, 1.6 s).
"""
import ctypes as C

import numpy as np
import pytest

import net_exact as ne
from linna_amd import _lib
from test_gpu_net_exact import FILLS, SENT, Out, load, padded, same, serve

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
SERVE_NETS = [n for n in ne.NETS if n not in ne.DENSE_NETS]


@pytest.fixture(autouse=True)
def _restore_switches():
    """engine_rows is process wide: put back what the test found."""
    rows = _lib.engine_rows(0)
    _lib.engine_rows(rows)
    yield
    _lib.engine_rows(rows)


def build_logprob(name, grad_precision="fp32"):
    from linna_amd import predictor_gpu, util
    c = ne.serving_consts(name)
    t = lambda a: torch.as_tensor(np.asarray(a, F))
    Xt = util.X_transform_class(t(c["X_mean"]), t(c["X_std"]), "cpu", None)
    Yt = util.Y_transform_class(t(c["y_mean"]), t(c["y_std"]), "cpu", ypositive=False)
    pred = predictor_gpu.Predictor(c["nin"], c["nout"], model=ne.fresh_model(name), X_transform=Xt, y_transform=Yt, device="cuda")
    yinv = util.Y_invtransform_data(np.asarray(c["sigma"], F), "cpu")
    lp = util.Log_prob(t(c["data"]), t(c["invcov"]), pred, yinv, util.Transform(c["priors"]), c["T"], util.gaussianlogliklihood, nograd=True,
                       precision="bf16", grad_precision=grad_precision)
    lp._ensure()
    return lp, pred.model


def precisions(lp):
    """(serving, gradient) precision codes of the handle."""
    h = lp._ensure()["handle"]
    a, b = C.c_int(-7), C.c_int(-7)
    _lib.call("linna_logprob_precision", h, C.byref(a))
    _lib.call("linna_logprob_grad_precision", h, C.byref(b))
    return a.value, b.value


# ----------------------------------------------------------------------------------------------- serving
def eval_if_halves(lp, z, fill):
    """lnP of two linna_logprob_eval_if launches over the halves of ``z``: the first gate open, the second shut."""
    B = len(z)
    h = (B + 1) // 2
    zbuf, _ = padded(z, fill)
    lnp = torch.full((B + 8,), SENT, device="cuda")
    gates = torch.tensor([1, 0], dtype=torch.int32, device="cuda")
    hd = lp._ensure()["handle"]
    for k, (lo, hi) in enumerate(((0, h), (h, B))):
        if hi > lo:
            _lib.call("linna_logprob_eval_if", hd, _lib.ptr(zbuf[lo:]), zbuf.stride(0), hi - lo, _lib.ptr(lp._workspace(hi - lo, False)),
                      _lib.ptr(lnp[lo:]), None, 0, _lib.iptr(gates[k:]), _lib.stream())
    return lnp.cpu().numpy(), h


def slice_points(lp, z, fill):
    """(rc, lnP [2 B]) of linna_logprob_eval_slice_points whose trial points coords[S[k]] + w[j B + k] DIR[k] ARE the rows of z:
    integer directions from {-1, 0, 1}, integer weights from {1, 2} (the same for both repetitions), coords = z - w DIR exactly."""
    B, nd = z.shape
    ld, nw = _lib.ld4(nd) + 4, 2 * B
    r = ne.rng("slice", B, nd)
    DIR = r.randint(-1, 2, (B, nd)).astype(F)
    w = r.randint(1, 3, B).astype(F)
    S = r.permutation(nw)[:B]
    coords = np.full((nw, ld), fill, F)
    coords[:, :nd] = 7.0                                   # (walkers outside S: never read)
    coords[S, :nd] = z - w[:, None] * DIR
    assert np.array_equal(coords[S, :nd] + w[:, None] * DIR, z)
    Db = np.full((B, ld), fill, F)
    Db[:, :nd] = DIR
    dev = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")
    cd, Dd, Sd, wd = dev(coords), dev(Db), dev(S, torch.int32), dev(np.concatenate([w, w]))
    lnp = torch.full((2 * B + 8,), SENT, device="cuda")
    rc = _lib.load().linna_logprob_eval_slice_points(lp._ensure()["handle"], _lib.ptr(cd), ld, nd, _lib.iptr(Sd), B, _lib.ptr(Dd), ld,
                                                     _lib.ptr(wd), 2, _lib.ptr(lnp), None, _lib.stream())
    torch.cuda.synchronize()
    return rc, lnp.cpu().numpy()


@pytest.mark.parametrize("name", SERVE_NETS)
def test_bf16_serving(name):
    """Log_prob(precision="bf16").evaluate, linna_logprob_eval_if and linna_logprob_eval_slice_points: every dense map at ROWS
    rows and the first and last one at every batch size, on each engine and the automatic choice."""
    lp, model = build_logprob(name)
    assert precisions(lp) == (1, 0), "the object is not served in bf16"
    nin = model.in_size
    for dense, B in ne.sweep_tables(name):
        s = ne.bf16_serving_table(name, dense, B, grad=name in ne.GRAD_NETS)
        ref, z = s["ref"], s["z"]
        load(model, s["P"])
        first = None
        for rows in (0,) + ne.ENGINES:
            _lib.engine_rows(rows)
            for fill in FILLS:
                tag = "%s dense map %d rows %d engine %d" % (name, dense, B, rows)
                lnp, th = serve(lp, z, fill, True)
                same(th, ref["theta"], tag + " THETA")
                same(lnp, ref["lnP"], tag + " lnP (with THETA)")
                lnp, _ = serve(lp, z, fill, False)
                same(lnp, ref["lnP"], tag + " lnP")
                first = lnp if first is None else first
                assert np.array_equal(lnp, first), tag + ": differs from the first engine"
                got, h = eval_if_halves(lp, z, fill)
                same(got[:h], ref["lnP"][:h], tag + " eval_if, gate open")
                assert np.all(got[h:] == SENT), tag + ": a launch gated off wrote lnP"
                rc, got = slice_points(lp, z, fill)
                if nin <= 64:
                    assert rc == 0, "%s: linna_logprob_eval_slice_points: %d %r" % (tag, rc, _lib.load().linna_last_error().decode())
                    same(got[:B], ref["lnP"], tag + " slice points, repetition 0")
                    same(got[B:2 * B], ref["lnP"], tag + " slice points, repetition 1")
                    assert np.all(got[2 * B:] == SENT), tag + ": wrote past the end of lnP"
                else:
                    assert rc == _lib.ERR_UNSUPPORTED and np.all(got == SENT), (tag, rc)
    assert precisions(lp) == (1, 0)


# ----------------------------------------------------------------------------------------------- gradient, leapfrog
def eps_rows(B):
    """A power-of-two step size per row."""
    return (2.0 ** -(1 + np.arange(B) % 3)).astype(F)


@pytest.mark.parametrize("name", ne.BF16_GRAD_NETS)
def test_bf16_gradient_and_leapfrog(name):
    """evaluate_with_grad (lnP, G), linna_logprob_grad_leapfrog and linna_logprob_grad_leapfrog_eps (P, Q) on the bf16 one-launch
    gradient, each engine, against the rounding reference."""
    lp, model = build_logprob(name, "bf16")
    assert precisions(lp) == (1, 1), "the gradient is not a bf16 one"
    nin = model.in_size
    m64 = ne.MASS(nin)
    mass = torch.as_tensor(m64.astype(F), device="cuda")
    hd = lp._ensure()["handle"]
    for dense, B in ne.sweep_tables(name):
        s = ne.bf16_serving_table(name, dense, B, grad=True)
        ref, z = s["ref"], s["z"]
        load(model, s["P"])
        P0 = ne.momenta(name, dense, B)
        Pn, Qn = ne.leapfrog_ref(ref["G"], z, P0, m64, ne.EPS, ne.EPS)
        eps = eps_rows(B)
        Pe, Qe = ne.leapfrog_ref(ref["G"], z, P0, m64, eps[:, None].astype(np.float64), 0.5 * eps[:, None].astype(np.float64))
        epsd = torch.as_tensor(eps, device="cuda")
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
                for form, (Pr, Qr) in (("", (Pn, Qn)), ("_eps", (Pe, Qe))):
                    qbuf, qview = padded(z, fill)
                    pbuf, pview = padded(P0, fill)
                    lnp, G = torch.full((B + 8,), SENT, device="cuda"), Out(B, nin)
                    head = (hd, _lib.ptr(qbuf), qbuf.stride(0), B, _lib.ptr(lp._workspace(B, True)), _lib.ptr(lnp), _lib.ptr(G.t), G.t.stride(0),
                            _lib.ptr(pbuf), pbuf.stride(0), _lib.ptr(mass))
                    if form:
                        _lib.call("linna_logprob_grad_leapfrog_eps", *(head + (_lib.ptr(epsd), 1.0, 0.5, _lib.stream())))
                    else:
                        _lib.call("linna_logprob_grad_leapfrog", *(head + (ne.EPS, ne.EPS, _lib.stream())))
                    same(G.read(), ref["G"], "%s leapfrog%s G" % (tag, form))
                    host = lnp.cpu().numpy()
                    assert np.all(host[B:] == SENT)
                    same(host[:B], ref["lnP"], "%s leapfrog%s lnP" % (tag, form))
                    same(pview.cpu().numpy(), Pr, "%s leapfrog%s P" % (tag, form))
                    same(qview.cpu().numpy(), Qr, "%s leapfrog%s Q" % (tag, form))
                    pads = qbuf.cpu().numpy()[:, nin:]
                    assert np.all(np.isnan(pads)) if fill != fill else np.all(pads == fill), tag + ": the leapfrog wrote the pads of Q"
    assert precisions(lp) == (1, 1)


@pytest.mark.parametrize("name", ne.BF16_GRAD_REFUSED)
def test_bf16_gradient_refusal(name):
    """A network with more than 64 inputs or outputs has no bf16 gradient program: LINNA_ERR_UNSUPPORTED with the reason from
    the setter and from the gradient entry of the bf16 object, and never a result."""
    lp, model = build_logprob(name)
    lib, hd = _lib.load(), lp._ensure()["handle"]
    rc = lib.linna_logprob_set_grad_precision(hd, 1)
    msg = lib.linna_last_error().decode()
    assert rc == _lib.ERR_UNSUPPORTED and "64" in msg, (rc, msg)
    assert precisions(lp) == (1, 0)
    B, nin = 5, model.in_size
    s = ne.bf16_serving_table(name, 0, B)
    load(model, s["P"])
    zbuf, _ = padded(s["z"], 0.0)
    lnp, G = torch.full((B + 8,), SENT, device="cuda"), Out(B, nin)
    rc = lib.linna_logprob_grad(hd, _lib.ptr(zbuf), zbuf.stride(0), B, _lib.ptr(lp._workspace(B, True)), _lib.ptr(lnp), _lib.ptr(G.t),
                                G.t.stride(0), _lib.stream())
    assert rc == _lib.ERR_UNSUPPORTED and "bf16" in lib.linna_last_error().decode()
    torch.cuda.synchronize()
    assert np.all(lnp.cpu().numpy() == SENT) and np.all(G.t.cpu().numpy() == SENT)


# ----------------------------------------------------------------------------------------------- the merged training step
class TrainRig(object):
    """One network on the GPU with a loss descriptor over net_exact.loss_cinv, driven through the C entries."""

    def __init__(self, name, precision):
        from linna_amd.predictor_gpu import _AdamWState
        self.name, self.model = name, ne.fresh_model(name).to("cuda")
        m = self.model
        self.nin, self.nout = m.in_size, m.out_size
        m.flat_grads()
        m.set_train_precision(precision)
        ldc = _lib.ld4(self.nout)
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, F), device="cuda")
        cinv = np.zeros((self.nout, ldc), F)
        cinv[:, :self.nout] = ne.loss_cinv(self.nout)
        self.keep = dict(one=dev(np.ones(self.nout)), zero=dev(np.zeros(self.nout)), cinv=dev(cinv), xmean=dev(np.zeros(self.nin)),
                         xstd=dev(np.ones(self.nin)))
        d = _lib.LossDesc()
        d.nout = self.nout
        d.sigma, d.ymean, d.ystd, d.data_norm = (_lib.ptr(self.keep[k]) for k in ("one", "zero", "one", "zero"))
        d.Cinv, d.ldc, d.ylog = _lib.ptr(self.keep["cinv"]), ldc, 0
        self.desc = d
        h = m.net_handle(with_grads=True)
        _lib.call("linna_net_prepare", h, 1, 0)
        _lib.call("linna_net_prepare_loss", h, C.byref(d))
        got = C.c_int(-7)
        _lib.call("linna_net_train_precision", h, C.byref(got))
        assert got.value == _lib.PRECISION[precision], "the handle does not train in %s" % precision
        self.opt = _AdamWState(m, 1e-3)

    def step(self, t, B, fill, update):
        """One call of linna_net_train_step (``update`` False; AdamW's step constants riding in it) or of
        linna_net_train_step_update on table ``t``: (rc, everything the call wrote)."""
        m, k, opt = self.model, self.keep, self.opt
        h = m.net_handle(with_grads=True)
        assert _lib.load().linna_net_train_launches(h, B) == 2, "not the merged training step"
        X, _ = padded(t["x"], fill)
        YN, _ = padded(t["YN"], fill)
        den = torch.as_tensor(t["den"], device="cuda")
        rows = torch.arange(B, dtype=torch.int32, device="cuda")
        xb, pred, dpred = Out(B, self.nin), Out(B, self.nout), Out(B, self.nout)
        loss_rows, mean = torch.full((B + 8,), SENT, device="cuda"), torch.full((4,), SENT, device="cuda")
        ws, bws = m.workspace(B), m.workspace(B, "bwd")
        ws.fill_(SENT); bws.fill_(SENT); m.flat_grads().fill_(SENT)
        head = (h, C.byref(self.desc), _lib.ptr(X), X.stride(0), _lib.iptr(rows), B, None, _lib.ptr(k["xmean"]), _lib.ptr(k["xstd"]), _lib.ptr(xb.t),
                xb.t.stride(0), _lib.ptr(ws), _lib.ptr(pred.t), pred.t.stride(0), _lib.ptr(YN), YN.stride(0), _lib.ptr(den), ne.INV_BATCH,
                _lib.ptr(loss_rows), _lib.ptr(mean), _lib.ptr(dpred.t), dpred.t.stride(0), _lib.ptr(bws))
        if update:
            rc = _lib.load().linna_net_train_step_update(*(head + (_lib.ptr(m._flat), _lib.ptr(opt.m), _lib.ptr(opt.v), m._flat.numel(), _lib.ptr(opt.hyper),
                                                                   _lib.iptr(opt.step_dev), opt.betas[0], opt.betas[1], opt.eps, _lib.stream())))
        else:
            rc = _lib.load().linna_net_train_step(*(head + (_lib.ptr(opt.hyper), _lib.iptr(opt.step_dev), opt.betas[0], opt.betas[1], _lib.stream())))
        torch.cuda.synchronize()
        return rc, dict(xb=xb, pred=pred, dpred=dpred, loss_rows=loss_rows.cpu().numpy(), mean=mean.cpu().numpy(), ws=ws.cpu().numpy(),
                        bws=bws.cpu().numpy(), G={kk: g.cpu().numpy().copy() for kk, g in m.grad_dict().items()})


def check_step(t, B, out, tag):
    ops = t["ops"]
    # (the launch owns the whole row stride of XB and dPRED -- the parameter-gradient launch reads them as padded matrices --
    #  and fills it with zeros behind the columns; the guard row stays)
    for what, ref64, key in ((" gathered batch", t["x"], "xb"), (" d loss / d pred", t["dpred"], "dpred")):
        full = out[key].t.cpu().numpy()
        same(full[:B, :ref64.shape[1]], ref64, tag + what)
        assert np.all(full[:B, ref64.shape[1]:] == 0) and np.all(full[B] == SENT), tag + what + ": its pads, or the row behind it"
    same(out["pred"].read(), t["fwd"][-1]["y"], tag + " PRED")
    same(out["loss_rows"][:B], t["rows"], tag + " loss rows")
    assert np.all(out["loss_rows"][B:] == SENT), tag + ": wrote past the loss rows"
    same(out["mean"][:1], np.array([t["mean"]]), tag + " batch mean")
    assert np.all(out["mean"][1:] == SENT)
    lay_f, tot_f = ne.fwd_layout(ops, B)
    for (i, what, off, ld, cols) in lay_f:
        same(out["ws"][off:off + B * ld].reshape(B, ld)[:, :cols], t["fwd"][i][what], "%s stored %s of op %d" % (tag, what, i))
    assert np.all(out["ws"][tot_f:] == SENT), tag + ": wrote past the forward workspace"
    lay_b, tot_b = ne.bwd_layout(ops, B)
    for (i, what, off, ld, cols) in lay_b:
        same(out["bws"][off:off + B * ld].reshape(B, ld)[:, :cols], t["bufs"][i][what], "%s %s of op %d" % (tag, what, i))
    assert np.all(out["bws"][tot_b:] == SENT), tag + ": wrote past the backward workspace"
    for k, g in out["G"].items():
        same(g, t["G"][k], "%s gradient of %s" % (tag, k))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ne.TRAIN_STEP_NETS)
def test_merged_training_step(name, precision):
    """linna_net_train_step and linna_net_train_step_update on the 4-row engine, exact loss tables: every dense map at 20 rows,
    the first and the last one at 1, 3, 4, 5 and 9 rows.  The update entry's parameters and moments against linna_adamw_step
    on the gradients of the step entry (AdamW itself is not exact: a cross-route check, bit for bit)."""
    bf = precision == "bf16"
    n = ne.n_maps(name)
    a, b = TrainRig(name, precision), TrainRig(name, precision)
    ran = False
    for dense in range(n):
        for B in (ne.LOSS_ROWS if dense in (0, n - 1) else (ne.ROWS,)):
            t = ne.loss_table(name, dense, B, bf)
            for fill in FILLS:
                tag = "%s %s dense map %d rows %d" % (name, precision, dense, B)
                for rig in (a, b):
                    load(rig.model, t["P"])
                    rig.opt.m.zero_(); rig.opt.v.zero_(); rig.opt.step_dev.zero_(); rig.opt.push_hyper()
                rc, out = a.step(t, B, fill, False)
                assert rc == 0, "%s: linna_net_train_step: %d %r" % (tag, rc, _lib.load().linna_last_error().decode())
                check_step(t, B, out, tag + " train_step")
                g = a.model.flat_grads()                   # (the sentinel out of the row pads: the parameters' pads stay zero)
                clean = torch.zeros_like(g)
                for k in a.model._index:
                    a.model._view(clean, k).copy_(a.model._view(g, k))
                g.copy_(clean)
                _lib.call("linna_adamw_step", _lib.ctx(0), _lib.ptr(a.model._flat), _lib.ptr(a.model.flat_grads()), _lib.ptr(a.opt.m), _lib.ptr(a.opt.v),
                          C.c_size_t(a.model._flat.numel()), _lib.ptr(a.opt.hyper), _lib.iptr(a.opt.step_dev), a.opt.betas[0], a.opt.betas[1],
                          a.opt.eps, 1, _lib.stream())
                rc, out = b.step(t, B, fill, True)
                assert rc == 0, "%s: linna_net_train_step_update: %d %r" % (tag, rc, _lib.load().linna_last_error().decode())
                check_step(t, B, out, tag + " train_step_update")
                torch.cuda.synchronize()
                # (tensor by tensor: the flat buffers' row pads hold the sentinel gradient in one route and nothing in the other)
                for what, x, y in (("parameters", a.model._flat, b.model._flat), ("first moments", a.opt.m, b.opt.m), ("second moments", a.opt.v, b.opt.v)):
                    for k in a.model._index:
                        assert torch.equal(a.model._view(x, k), b.model._view(y, k)), "%s: %s of %s after the update entry differ from linna_adamw_step's" % (tag, what, k)
                assert torch.equal(a.opt.hyper, b.opt.hyper) and torch.equal(a.opt.step_dev, b.opt.step_dev), tag + ": step constants"
                assert int(b.opt.step_dev.item()) == 1, tag + ": the step counter"
                ran = ran or float(b.opt.v.abs().max()) > 0
    assert ran, name + ": no update moved a moment"
