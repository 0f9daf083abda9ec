"""GPU: the opt-in bf16 training step (linna_net_set_train_precision; Predictor.train / train_NN / ml_sampler_core with
precision="bf16").

* one step against a float64 emulation that rounds exactly where the kernel does (tests/bf16_train_emul.py): the GPU's
  distance from it is at most 0.2 x the rounding's own effect (the serving test's rule), for the loss rows, d loss / d pred
  and every parameter gradient;
* the loss segment stays fp32 inside the bf16 launch: at condition 1e6 the launch's loss equals the layered fp32 loss on
  the launch's own predictions;
* the stream the AdamW writers leave equals a fresh pack, the update forms agree, graph replay equals direct launches, fp32
  training is untouched by a bf16 run in the same process, refusals come before anything runs;
* training quality (300 epochs) and the README problem end to end with a bf16-trained emulator.
"""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import synth
import readme33
import bf16_train_emul

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _engine(kind, nin, nout, seed, B, precision, cond=1e2, kw=None, weights=None, nbatch=3, half_residuals=False):
    """A TrainEngine over nbatch batches of B rows of a synthetic problem, its loss covariance dense of condition `cond`."""
    from linna_amd import nn, util, predictor_gpu, trainer
    kw = kw or {}
    rs = np.random.RandomState(seed + 31)
    if cond > 1e3:
        cov, _, half = synth.cond_problem(nin, nout, seed, cond)
        data = rs.uniform(size=nout)
    else:
        data, cov, _ = synth.gaussian_problem(nin, nout, seed, dense=True, cond=cond)
        half = None
    sigma = np.sqrt(np.diag(cov))
    X_mean, X_std, y_mean, y_std = synth.transform_constants(nin, nout, seed)
    X = (X_mean[None, :] + X_std[None, :] * rs.standard_normal((nbatch * B, nin))).astype(np.float32)
    if half is not None:       # residuals the covariance calls likely (chi^2 of order nout)
        Y = (data[None, :] + rs.standard_normal((nbatch * B, nout)) @ half).astype(np.float32)
    else:
        Y = (data[None, :] + 3 * sigma[None, :] * rs.standard_normal((nbatch * B, nout))).astype(np.float32)
    cls = {"ChtoModelv2": nn.ChtoModelv2, "MLP": nn.MLP, "ChtoModelv2_linear": nn.ChtoModelv2_linear}[kind]
    model = cls(nin, nout, None, **kw)
    model.load_state_dict(weights if weights is not None else synth.weights(kind, nin, nout, seed, **kw))
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    pred = predictor_gpu.Predictor(nin, nout, model=model, device="cuda",
                                   X_transform=util.X_transform_class(t(X_mean), t(X_std), "cpu", None),
                                   y_transform=util.Y_transform_class(t(y_mean), t(y_std), "cpu"))
    lf = util.Loss_fn(t(data), torch.tensor(cov, dtype=torch.float64), torch.tensor(np.linalg.inv(cov), dtype=torch.float64),
                      util.Y_transform_data(sigma, "cpu"), util.Y_invtransform_class(t(y_mean), t(y_std), t(data), "cpu"), "cpu")
    loader = predictor_gpu.BatchLoader(util.ArrayDataset(X, Y), B, shuffle=False, drop_last=True)
    eng = trainer.TrainEngine(pred, loader, lf, None, use_graph=False, precision=precision)
    return model, eng


PROBLEMS = {      # name: (kind, nin, nout, seed, B, kw)
    "train_v2_33_33": ("ChtoModelv2", 33, 33, 203, 100, {}),
    "train_v2_26_457": ("ChtoModelv2", 26, 457, 205, 64, {}),
    "mlp_4x512_33_33": ("MLP", 33, 33, 207, 100, {}),
}


def _rows(s, B):
    return torch.arange((s % 3) * B, (s % 3 + 1) * B, dtype=torch.int32, device="cuda")


def _rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64))))) if np.size(a) else 0.0


def _stored(model, eng, kind, nin, nout, B, kw):
    """What the launch stored, per op (net_bufs' order in api.hip): (input, hidden t, output) of the forward; d loss /
    d (op input) (dys[i], i >= 1) and d loss / d t (dts[i]) of the backward."""
    from oracle import emulator
    from linna_amd import _lib
    ops = emulator.topology(kind, nin, nout, **kw)
    fw = model.workspace(B).cpu().numpy()
    bw = model.workspace(B, "bwd").cpu().numpy()
    take = lambda buf, off, n: (buf[off:off + B * _lib.ld4(n)].reshape(B, _lib.ld4(n))[:, :n], off + B * _lib.ld4(n))
    acts, off, h = [], 0, eng.xb[:, :nin].cpu().numpy()
    for i, op in enumerate(ops):
        t = None
        if op[0] == "resblock":
            t, off = take(fw, off, op[3])
        N = op[3] if op[0] == "linear" else op[4]
        if i + 1 < len(ops):
            y, off = take(fw, off, N)
        else:
            y = eng.predb[:, :N].cpu().numpy()
        acts.append((h, t, y))
        h = y
    dys, dts, off = {}, {}, 0
    for i in range(len(ops) - 1, -1, -1):
        op = ops[i]
        if i > 0:
            dys[i], off = take(bw, off, op[2])
        if op[0] == "resblock":
            dts[i], off = take(bw, off, op[3])
    return acts, dys, dts


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_one_step_matches_the_emulation(name, capsys):
    kind, nin, nout, seed, B, kw = PROBLEMS[name]
    model, eng = _engine(kind, nin, nout, seed, B, "bf16", kw=kw)
    params = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    rows = _rows(1, B)
    eng._forward_loss_backward(rows, torch.zeros(1, device="cuda"), None, update=False)     # linna_net_train_step: gradients stay readable
    torch.cuda.synchronize()
    assert eng.one_launch is True
    x = eng.xb[:, :nin].cpu().numpy()
    YN = eng.YN[rows.long()][:, :nout].cpu().numpy()
    den = eng.den[rows.long()].cpu().numpy()
    cinv = eng._keep["cinv"][:, :nout].cpu().numpy()
    got_loss = eng.loss_rows.cpu().numpy()
    got_dp = eng.dpred[:, :nout].cpu().numpy()
    got_g = {k: v.detach().cpu().numpy() for k, v in model.grad_dict().items()}
    r = bf16_train_emul.train_step(params, x, kind, nin, nout, YN, den, eng.inv_batch, cinv, rounded=True, **kw)
    e = bf16_train_emul.train_step(params, x, kind, nin, nout, YN, den, eng.inv_batch, cinv, rounded=False, **kw)
    # the loss rows, d loss / d pred and the last layer's gradients against the free-running emulation of the whole step;
    # every other parameter gradient one rounding stage at a time from the launch's own stored tensors
    # (bf16_train_emul.stage_grads: over a deep chain, fp32 noise that moves an operand across a bf16 rounding boundary
    # compounds -- the free-running distance grows by about 0.01 per stage of ChtoModelv2(26,457))
    acts, dys, dts = _stored(model, eng, kind, nin, nout, B, kw)
    rs = bf16_train_emul.stage_grads(params, kind, nin, nout, acts, dys, dts, got_dp, rounded=True, **kw)
    es = bf16_train_emul.stage_grads(params, kind, nin, nout, acts, dys, dts, got_dp, rounded=False, **kw)
    checks = [("loss rows", got_loss, r[0], e[0]), ("dPRED", got_dp, r[1], e[1])]
    checks += [(k, got_g[k], r[2][k], e[2][k]) for k in r[2] if k not in rs]
    checks += [(k + " (stage)", got_g[k], rs[k], es[k]) for k in rs]
    assert len(checks) == 2 + len(r[2])
    with capsys.disabled():
        for what, g, rr, ee in checks:
            gap, eff = _rms(g - rr), _rms(rr - ee)
            print("%s %-26s |gpu - emul| %.3e   |emul - exact| %.3e   ratio %.3f" % (name, what, gap, eff, gap / max(eff, 1e-30)))
    for what, g, rr, ee in checks:
        assert np.all(np.isfinite(g)), what
        assert _rms(g - rr) <= 0.2 * _rms(rr - ee), (what, _rms(g - rr), _rms(rr - ee))


def test_loss_segment_stays_fp32_at_condition_1e6():
    """(26,457) with a loss covariance of condition 1e6: the launch's loss rows and d loss / d pred against
    linna_chi2_ratio_loss_fwd_bwd on the launch's own predictions -- bf16 rounding of Cinv or delta would move chi^2 by
    about 2^-9 cond; the fp32 suite's bound for the one-launch loss (2e-4 of the largest value) holds."""
    from linna_amd import _lib
    model, eng = _engine("ChtoModelv2", 26, 457, 211, 64, "bf16", cond=1e6)
    rows = _rows(0, 64)
    eng._forward_loss_backward(rows, torch.zeros(1, device="cuda"), None, update=False)
    torch.cuda.synchronize()
    lr_a, dp_a = eng.loss_rows.clone(), eng.dpred.clone()
    pred = eng.predb.clone()
    lr_b, lm = torch.zeros_like(lr_a), torch.zeros(1, device="cuda")
    dp_b = torch.full_like(dp_a, 7.0)
    _lib.call("linna_chi2_ratio_loss_fwd_bwd", eng.ctx, C.byref(eng.desc), _lib.ptr(pred), pred.stride(0), _lib.ptr(eng.Y),
              eng.Y.stride(0), _lib.ptr(eng.den), _lib.iptr(rows), 64, _lib.ptr(eng.scratch), _lib.ptr(lr_b), _lib.ptr(lm),
              _lib.ptr(dp_b), dp_b.stride(0), eng.inv_batch, _lib.stream())
    torch.cuda.synchronize()
    a, b = lr_a.cpu().numpy(), lr_b.cpu().numpy()
    da, db = dp_a[:, :457].cpu().numpy(), dp_b[:, :457].cpu().numpy()
    e_rows = np.abs(a - b).max() / np.abs(b).max()
    e_dp = np.abs(da - db).max() / np.abs(db).max()
    print("condition 1e6: loss rows %.2e, dPRED %.2e of the largest value" % (e_rows, e_dp))
    assert np.all(np.isfinite(a)) and e_rows < 2e-4 and e_dp < 2e-4, (e_rows, e_dp)


def _state(model, opt):
    return [model._flat.clone(), opt.m.clone(), opt.v.clone(), opt.step_dev.clone(), opt.hyper.clone()]


def _restore(model, opt, st):
    for dst, src in zip([model._flat, opt.m, opt.v, opt.step_dev, opt.hyper], st):
        dst.copy_(src)


def _step4_live_and_fresh(model, eng, opt, B):
    """Step 4 twice from the state after step 3: on the stream the AdamW writers left, and after linna_weights_changed
    (a fresh pack)."""
    from linna_amd import _lib
    st = _state(model, opt)
    out = []
    for fresh in (False, True):
        if fresh:
            _restore(model, opt, st)
            torch.cuda.synchronize()
            _lib.call("linna_weights_changed", eng.ctx)
        loss = torch.zeros(1, device="cuda")
        eng.step(opt, _rows(3, B), loss_out=loss)
        torch.cuda.synchronize()
        out.append([t.cpu().numpy().copy() for t in (model._flat, opt.m, opt.v, loss, eng.loss_rows, eng.dpred)])
    return out


@pytest.mark.parametrize("name", ["train_v2_33_33", "train_v2_26_457", "mlp_4x512_33_33"])
@pytest.mark.parametrize("form", ["update", "step+adamw"])
def test_written_stream_equals_a_fresh_pack(name, form):
    from linna_amd.predictor_gpu import _AdamWState
    kind, nin, nout, seed, B, kw = PROBLEMS[name]
    model, eng = _engine(kind, nin, nout, seed, B, "bf16", kw=kw)
    opt = _AdamWState(model, 2e-3)
    if form != "update":
        eng.one_update = False
    for s in range(3):
        eng.step(opt, _rows(s, B))
    live, fresh = _step4_live_and_fresh(model, eng, opt, B)
    assert eng.one_launch is True
    assert (eng.one_update is True) if form == "update" else (opt._streams is True and eng.one_update is False)
    assert np.all(np.isfinite(live[3]))
    for a, b in zip(live, fresh):
        np.testing.assert_array_equal(a, b)


def test_update_forms_agree():
    from linna_amd.predictor_gpu import _AdamWState
    kind, nin, nout, seed, B, kw = PROBLEMS["train_v2_26_457"]
    res = []
    for form in ("update", "step+adamw"):
        model, eng = _engine(kind, nin, nout, seed, B, "bf16", kw=kw)
        opt = _AdamWState(model, 1e-3)
        if form != "update":
            eng.one_update = False
        losses = []
        for s in range(3):
            out = torch.zeros(1, device="cuda")
            eng.step(opt, _rows(s, B), loss_out=out)
            losses.append(out)
        torch.cuda.synchronize()
        res.append([model._flat.cpu().numpy().copy(), opt.m.cpu().numpy().copy(), opt.v.cpu().numpy().copy(), torch.cat(losses).cpu().numpy()])
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


def test_graph_replay_equals_direct_launches():
    from linna_amd.predictor_gpu import _AdamWState
    kind, nin, nout, seed, B, kw = PROBLEMS["train_v2_33_33"]
    res = []
    for use_graph in (False, True):
        model, eng = _engine(kind, nin, nout, seed, B, "bf16", kw=kw)
        eng.use_graph = use_graph
        opt = _AdamWState(model, 1e-3)
        if use_graph:
            eng.prepare_graph(opt)
        for s in range(3):
            eng.step(opt, _rows(s, B))
        torch.cuda.synchronize()
        res.append(model.flat_params().cpu().numpy().copy())
    assert np.all(np.isfinite(res[0]))
    np.testing.assert_array_equal(res[0], res[1])


def _train_NN(tmp, kind, nin, nout, tx, ty, vx, vy, cov, data, epochs, precision, w0=None, B=500, lr=1e-3):
    from linna_amd import util, nn
    os.makedirs(tmp, exist_ok=True)
    np.savetxt(tmp + "train_samples_x.txt", tx); np.save(tmp + "train_samples_y.npy", ty)
    np.savetxt(tmp + "val_samples_x.txt", vx); np.save(tmp + "val_samples_y.npy", vy)
    np.save(tmp + "lr.npy", lr)
    cls = {"MLP": nn.MLP, "ChtoModelv2": nn.ChtoModelv2}[kind]

    def factory(in_size, out_size, linearmodel, docpu=False):
        m = cls(in_size, out_size, linearmodel, docpu=docpu)
        if w0 is not None:
            m.load_state_dict(w0)
        return m

    torch.manual_seed(readme33.SEED)
    model = util.train_NN(None, cov, np.linalg.inv(cov), np.sqrt(np.diag(cov)), tmp, [tmp], data, None, False, True, 2, 1.0,
                          False, None, 1, factory, {"num_epochs": epochs, "batch_size": B}, False, precision=precision)
    return model


def _readme33_set():
    prob = readme33.problem()
    tx, vx = readme33.design(10000, prob["ndim"]), readme33.design(500, prob["ndim"])
    return prob, tx, tx.copy(), vx, vx.copy()


def test_fp32_training_is_untouched_by_a_bf16_run(tmp_path):
    prob, tx, ty, vx, vy = _readme33_set()
    w0 = synth.weights("MLP", 33, 33, 17)
    runs = []
    for k, prec in enumerate(("fp32", "bf16", "fp32")):
        m = _train_NN(str(tmp_path) + "/r%d/" % k, "MLP", 33, 33, tx[:2000], ty[:2000], vx, vy, prob["cov"], prob["means"], 3, prec, w0)
        runs.append((m.model._flat.cpu().numpy().copy(), np.asarray(m.train_history[0]), np.asarray(m.train_history[1])))
    for a, b in zip(runs[0], runs[2]):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(runs[0][0], runs[1][0])          # (the bf16 run did run in bf16)


def test_refusals_leave_the_weights_untouched():
    from linna_amd import _lib, nn
    # a 2048-row batch: the 8-row engine
    model, eng = _engine("ChtoModelv2", 33, 33, 203, 100, "fp32")
    before = model._flat.clone()
    with pytest.raises(ValueError, match="4-row engine"):
        _engine("ChtoModelv2", 33, 33, 203, 2048, "bf16", weights={k: v.cpu().numpy() for k, v in model.state_dict().items()}, nbatch=1)
    # the C entries on a bf16 handle at that batch: UNSUPPORTED with "bf16"
    model2, eng2 = _engine("ChtoModelv2", 33, 33, 203, 100, "bf16")
    h = model2.net_handle(with_grads=True)
    flat = model2._flat
    z = torch.zeros(flat.numel(), device="cuda")
    hyper, step = torch.tensor([1e-3, 1e-4, 1.0, 1.0], device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    prev = flat.clone()
    rc = _lib.load().linna_net_adamw_step(h, 2048, _lib.ptr(flat), _lib.ptr(z), _lib.ptr(z), _lib.ptr(z), flat.numel(), _lib.ptr(hyper),
                                          _lib.iptr(step), 0.9, 0.999, 1e-8, 1, _lib.stream())
    assert rc == _lib.ERR_UNSUPPORTED and "bf16" in _lib.load().linna_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(prev, flat)
    # a 1100-wide network and an input-skip network: refused when training starts
    with pytest.raises(ValueError, match="1024"):
        _engine("ChtoModelv2", 12, 1100, 213, 64, "bf16", nbatch=1)
    with pytest.raises(ValueError, match="input-skip"):
        _engine("ChtoModelv2_linear", 5, 3, 206, 40, "bf16", nbatch=1)
    torch.cuda.synchronize()
    assert torch.equal(before, model._flat)


def _linear457_set(n, seed):
    rs = np.random.RandomState(seed)
    A = rs.standard_normal((26, 457)) / np.sqrt(26)
    c = rs.uniform(size=457)
    x = rs.uniform(-1, 1, (n, 26))
    return x, x @ A + c


def test_training_quality(tmp_path, capsys):
    """300 epochs, same seed, fp32 and bf16: the best validation metric of the bf16 run is within 1.1 x the fp32 one, on the
    README problem with the 4 x 512 MLP and on a linear 26 -> 457 theory with ChtoModelv2(26,457) and a dense covariance."""
    from linna_amd import _lib
    res = {}
    prob, tx, ty, vx, vy = _readme33_set()
    x4, y4 = _linear457_set(10500, 3)
    _, cov457, _ = synth.gaussian_problem(26, 457, 5, dense=True, cond=1e2)
    sets = {"readme33 MLP 4x512": ("MLP", 33, 33, tx, ty, vx, vy, prob["cov"], prob["means"]),
            "linear457 ChtoModelv2(26,457)": ("ChtoModelv2", 26, 457, x4[:10000], y4[:10000], x4[10000:], y4[10000:], cov457, y4.mean(0))}
    for name, (kind, nin, nout, a, b, c, d, cov, data) in sets.items():
        for prec in ("fp32", "bf16"):
            m = _train_NN(str(tmp_path) + "/%s_%s/" % (kind, prec), kind, nin, nout, a, b, c, d, cov, data, 300, prec)
            res[(name, prec)] = float(np.min(np.asarray(m.train_history[1])[:, 0]))
            if prec == "bf16":
                st = np.zeros(1, np.int32)
                _lib.call("linna_net_train_precision", m.model.net_handle(with_grads=True), st.ctypes.data_as(C.c_void_p))
                assert int(st[0]) == _lib.PRECISION["bf16"]
        with capsys.disabled():
            print("%s: best validation metric fp32 %.5g, bf16 %.5g" % (name, res[(name, "fp32")], res[(name, "bf16")]))
    for name in sets:
        assert res[(name, "bf16")] <= 1.1 * res[(name, "fp32")], (name, res[(name, "bf16")], res[(name, "fp32")])


def test_ml_sampler_core_with_a_bf16_trained_emulator(tmp_path):
    from linna_amd.main import ml_sampler_core
    from linna_amd import nn
    prob = readme33.problem()
    means, cov, ndim = prob["means"], prob["cov"], prob["ndim"]
    sig = np.sqrt(np.diag(cov))
    out = str(tmp_path) + "/g33/"
    np.random.seed(0)
    torch.manual_seed(readme33.SEED)
    params = {"trainingoption": 1, "num_epochs": 600, "batch_size": 500}
    chain, logp = ml_sampler_core([10000] * 4, [500] * 4, [2, 2, 5, 4], [5, 5, 10, 15], [0.03, 0.03, 0.02, 0.01], [0.2] * 4,
                                  [0.15] * 4, out, readme33.theory, prob["priors"], means, cov, prob["init"], None, 4096, "cuda",
                                  None, False, [4.0, 2.0, 1.0, 1.0], None, False, 1, None, nn.MLP4x512, params, "emcee",
                                  train_precision="bf16")
    assert chain.ndim == 2 and chain.shape[1] == ndim and np.all(np.isfinite(chain))
    bias = np.abs(chain.mean(0) - means) / sig
    print("bf16-trained emulator: max |mean bias| %.3f sigma, max |std/sigma - 1| %.3f" % (bias.max(), np.abs(chain.std(0) / sig - 1).max()))
    assert bias.max() < 0.05, bias
    np.testing.assert_allclose(chain.std(0), sig, rtol=0.05)
    corr = np.corrcoef(chain.T)
    assert np.abs(corr - np.eye(ndim)).max() < 0.05
    import shutil
    shutil.rmtree(out, ignore_errors=True)
