"""GPU: the opt-in bf16 serving engine of the whole-network kernel (linna_logprob_set_precision, util.Log_prob(precision=)).

Bounds are plain asserts with the bound in the message (no tolerance wrappers: tests/parity.py widens those in test_gpu_*
files).  Every golden serving network is used with a DIAGONAL inverse covariance (the diagonal of its own): bf16 refuses a
dense one."""
import ctypes as C

import numpy as np
import pytest

import bf16_emul
import cases
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from test_gpu_serving import build_logprob, _custom_problem  # noqa: E402
from test_gpu_sampling import identity_emulator_logprob, _gaussian_33  # noqa: E402

NAMES = [c[0] for c in cases.SERVING]


def diag_problem(name):
    prob = cases.serving_problem(name)
    w = np.diagonal(np.asarray(prob["invcov"], np.float64)).copy()
    return dict(prob, invcov=np.diag(w)), w


def as_bf16(lp):
    """A bf16 Log_prob on the same emulator, data and priors as `lp`."""
    from linna_amd import util
    return util.Log_prob(lp.data_new, lp.invcov_new, lp.model, lp.y_invtransform_data, lp.transform, lp.T,
                         lp.loglikelihoodfunc, nograd=True, precision="bf16")


def rows_of(z, rows, lp):
    prev = _lib.engine_rows(rows)
    try:
        return lp(z, returntorch=False).astype(np.float64)
    finally:
        _lib.engine_rows(prev)


def sensitivity(prob, w, z, T):
    """S [B]: the first-order bound of |lnP(bf16) - lnP(exact)| per unit of c 2^-8 (test_error_bound_against_the_exact_network)."""
    from oracle import likelihood
    z64 = np.asarray(z, np.float64)
    theta = likelihood.prior_map(z64, prob["priors"])
    x = likelihood.x_transform(theta, np.asarray(prob["X_mean"], np.float64), np.asarray(prob["X_std"], np.float64), prob["dolog10"])
    h = bf16_emul.network(prob["weights"], x.astype(np.float32), prob["kind"], prob["nin"], prob["nout"], rounded=False, **prob["kw"])
    A = bf16_emul.abs_network(prob["weights"], x.astype(np.float32), prob["kind"], prob["nin"], prob["nout"], **prob["kw"])
    return h, A


@pytest.mark.parametrize("name", NAMES)
def test_rounds_exactly_where_it_says(name):
    """GPU against tests/bf16_emul.py (weights rounded after folding, A operands rounded, input as hi + lo): over walkers,
    rms(GPU - emulation) <= 0.2 rms(emulation - unrounded network), for every engine, temperature and batch size (the
    64-row batch as 32 launches of 64 rows, so that the rms is over 2048 walkers).  The GPU sums in fp32, the emulation in
    float64: an operand that lies within that difference of a bf16 rounding boundary rounds the other way (measured: the
    median |GPU - emulation| is ~1e-5 at |lnP| ~ 200, but a few walkers in a thousand move by up to a whole one-operand
    rounding of a narrow layer) -- per walker |GPU - emulation| <= 2^-6 S + 1e-5 (1 + |lnP|), S the first-order bound of
    ONE stage's rounding (_lnp_sensitivity): a few one-ulp flips (2^-7 each), never the L + 1 stages of the whole effect.
    A kernel that truncates, rounds before folding 0.1, or drops x_lo fails the rms ratio (its rms is ~ the whole effect)."""
    prob, w = diag_problem(name)
    for T in (1.0, 2.0, 4.0):
        lp32 = build_logprob(None, T, prob)[0]
        lp = as_bf16(lp32)
        for B, nb in ((4096, 1), (64, 32)):
            z = (0.5 * np.random.RandomState(B + int(T)).standard_normal((B * nb, prob["nin"]))).astype(np.float32)
            emu = bf16_emul.log_prob(z, prob, w, T)
            exact = bf16_emul.log_prob(z, prob, w, T, rounded=False)
            ref_rms = np.sqrt(np.mean((emu - exact) ** 2))
            S = _lnp_sensitivity(prob, w, z, T)
            for rows in (16, 8, 4):
                got = np.concatenate([rows_of(z[i * B:(i + 1) * B], rows, lp) for i in range(nb)])
                assert np.all(np.isfinite(got)), (name, T, B, rows)
                rms = np.sqrt(np.mean((got - emu) ** 2))
                assert rms <= 0.2 * ref_rms, "%s T=%g B=%d rows=%d: rms(GPU-emu) %.3e > 0.2 * rms(emu-exact) %.3e" % (
                    name, T, B, rows, rms, 0.2 * ref_rms)
                bound = 2.0 ** -6 * S + 1e-5 * (1 + np.abs(emu))
                worst = np.max(np.abs(got - emu) / bound)
                assert worst <= 1.0, "%s T=%g B=%d rows=%d: |GPU-emu| reaches %.3g of its bound 2^-6 S + 1e-5(1+|lnP|)" % (
                    name, T, B, rows, worst)


def _lnp_sensitivity(prob, w, z, T):
    """S = sum_j w_j (|d_j| e_j + e_j^2 / 2) / T with e_j the bound of |delta d_j| for ONE unit (2^-8) of relative error on the
    raw output's absolute network A_j (see test_error_bound_against_the_exact_network)."""
    h, A = sensitivity(prob, w, z, T)
    return _lnp_bound(prob, w, h, A, T, 1.0)


def _lnp_bound(prob, w, h, A, T, c):
    ys, ym = np.asarray(prob["y_std"], np.float64), np.asarray(prob["y_mean"], np.float64)
    sig, data = np.asarray(prob["sigma"], np.float64), np.asarray(prob["data"], np.float64)
    Er = c * 2.0 ** -8 * A                                   # bound on |delta raw output|
    if prob["ypositive"]:
        v = h * ys + ym
        d = np.exp(v) * sig - data
        with np.errstate(over="ignore"):                     # (a first-order bound this loose may be infinite: vacuous, still true)
            e = np.abs(sig) * np.exp(v) * np.expm1(np.abs(ys) * Er)
    else:
        d = (h * ys + ym) * sig - data
        e = np.abs(ys * sig) * Er
    with np.errstate(over="ignore", invalid="ignore"):
        return (w[None, :] * (np.abs(d) * e + 0.5 * e * e)).sum(-1) / T


@pytest.mark.parametrize("name", NAMES)
def test_error_bound_against_the_exact_network(name, capsys):
    """|lnP(bf16 GPU) - lnP(float64 oracle)| against a bound derived from where the engine rounds.

    Each of the network's L matrix products (a residual block counts two: h = W1 x, then [Ws | 0.1 W2] [x ; h]) multiplies
    operands that were each rounded to bf16 by at most a relative u = 2^-9 (the input's hi + lo split is exact to 2^-17):
    |fl(a) fl(w) - a w| <= (2u + u^2) |a||w|, i.e. at most 2^-8 (1 + 2^-9) sum_k |a_k||w_k| per output of that stage.
    ReLU is 1-Lipschitz and every later stage maps an error through |W| (0.1 |W2| in a residual block), so the error of a
    raw output is at most (1 + 2^-8)^L L 2^-8 A_j <= (L + 1) 2^-8 A_j for L <= 16, A the absolute-value network
    (A_0 = |x|, each op with |W| and |b|; tests/bf16_emul.abs_network).  With e_j the image of that bound through the output
    map (|ystd sigma| per unit, or sigma exp(v) expm1(ystd .) for the exp map) and d_j the exact residual:
        |delta lnP| <= sum_j w_j (|d_j| e_j + e_j^2 / 2) / T          (c = L + 1, the form c 2^-8 sum |terms|)
    plus the fp32 arithmetic of the rest, well inside 1e-5 (1 + |lnP|).  The distribution is printed."""
    from oracle import likelihood
    prob, w = diag_problem(name)
    T = 1.0
    lp = as_bf16(build_logprob(None, T, prob)[0])
    z = (0.5 * np.random.RandomState(11).standard_normal((4096, prob["nin"]))).astype(np.float32)
    got = lp(z, returntorch=False).astype(np.float64)
    ref = likelihood.log_prob(z, cases.oracle_emulator(prob), prob["priors"], prob["data"], prob["invcov"], T, dtype=np.float64)
    L = bf16_emul.stages(prob["kind"], prob["nin"], prob["nout"], **prob["kw"])
    h, A = sensitivity(prob, w, z, T)
    bound = _lnp_bound(prob, w, h, A, T, L + 1) + 1e-5 * (1 + np.abs(ref))
    err = np.abs(got - ref)
    q = np.percentile(err, [50, 90, 99, 100])
    with capsys.disabled(), np.errstate(over="ignore"):
        print("\n  bf16 %-16s |dlnP| p50 %.2e p90 %.2e p99 %.2e max %.2e   (|lnP| median %.2e, bound/err min %.1f)" % (
            name, q[0], q[1], q[2], q[3], np.median(np.abs(ref)), np.min(bound / np.maximum(err, 1e-30))))
    assert np.all(err <= bound), "%s: |dlnP| exceeds (L+1) 2^-8 sum|terms| in %d walkers (worst %.3g of the bound)" % (
        name, int(np.sum(err > bound)), np.max(err / bound))
    assert q[3] > 0, "bf16 equal to the fp64 oracle everywhere: not rounding?"


def _posterior_gate(th, means, cov, what):
    sig = np.sqrt(np.diag(cov))
    dm = np.max(np.abs(th.mean(0) - means) / sig)
    ds = np.max(np.abs(th.std(0) / sig - 1))
    assert dm < 0.05, "%s: posterior mean off by %.3f sigma (gate 0.05)" % (what, dm)
    assert ds < 0.06, "%s: posterior std off by %.3f (gate 6 %%)" % (what, ds)


def test_posterior_33d_gaussian_emcee_and_slice():
    """test_ensemble_posterior_33d_gaussian's set-up through a bf16 Log_prob: emcee at 2048 walkers (the fused bf16 stretch
    launches) and the slice driver (bf16 has no slice move: the driver falls back to linna_slice_points + a bf16
    linna_logprob_eval_if)."""
    from linna_amd import sampler, util
    ndim, means, cov, priors = _gaussian_33()
    lp = as_bf16(identity_emulator_logprob(ndim, means, cov, priors))
    nw = 2048
    ens = sampler.EnsembleSampler(nw, ndim, lp, seed=3)
    z0 = util.invTransform(priors)(means)[None, :] + 0.01 * np.random.RandomState(1).standard_normal((nw, ndim))
    ens.set_state(z0)
    ens.run(1500, store=False)
    c, _ = ens.run(600)
    assert ens.fused is not False, "the bf16 stretch move must run fused"
    _posterior_gate(ens.theta_of(c).cpu().numpy().reshape(-1, ndim), means, cov, "emcee bf16")

    nw = 512
    sl = sampler.SliceEnsembleSampler(nw, ndim, lp, seed=5)
    z0 = util.invTransform(priors)(means)[None, :] + 0.001 * np.random.RandomState(1).standard_normal((nw, ndim))
    sl.set_state(z0)
    sl.run(300, store=False)
    c, l = sl.run(500)
    _posterior_gate(sl.theta_of(c).cpu().numpy().reshape(-1, ndim), means, cov, "slice bf16")
    # the stored log-probabilities are the bf16 log-probabilities of the stored positions (another engine may sum in
    # another order: fp32-level differences only, the operands are rounded the same way)
    again = lp.evaluate(torch.nn.functional.pad(c[-1], (0, sl.ld - ndim))).cpu().numpy().astype(np.float64)
    stored = l[-1].cpu().numpy().astype(np.float64)
    worst = np.max(np.abs(again - stored) / (1e-4 * (1 + np.abs(stored))))
    assert worst <= 1.0, "slice chain lnP are not the bf16 lnP of the stored positions: %.3g of 1e-4 (1 + |lnP|)" % worst


@pytest.mark.parametrize("name,nw", [("mlp_33_33", 200), ("v2_33_33", 64), ("custom_7_5", 34)])
def test_fused_stretch_is_bit_identical_to_propose_eval_accept(name, nw):
    """In bf16 as in fp32: linna_stretch_half_step against propose / bf16 linna_logprob_eval / accept on the same Philox draws."""
    from linna_amd import sampler
    custom = _custom_problem(7, 5, 31, 48, 3) if name == "custom_7_5" else None
    prob = custom if custom is not None else diag_problem(name)[0]
    if custom is not None:
        prob = dict(prob, invcov=np.diag(np.diagonal(prob["invcov"])))
    lp = as_bf16(build_logprob(None, 2.0, prob)[0])
    nd = prob["nin"]
    x0 = (0.3 * np.random.RandomState(5).standard_normal((nw, nd))).astype(np.float32)
    a = sampler.EnsembleSampler(nw, nd, lp, seed=21)
    b = sampler.EnsembleSampler(nw, nd, lp, seed=21, fused=False)
    a.set_state(x0); b.set_state(x0)
    for _ in range(6):
        a.step(); b.step()
    torch.cuda.synchronize()
    assert a.fused is True and b.fused is False
    assert torch.equal(a.coords, b.coords), "fused bf16 stretch moved differently"
    assert torch.equal(a.logp, b.logp), "fused bf16 stretch lnP differ"
    assert torch.equal(a.naccept, b.naccept)
    assert 0 < int(a.naccept.sum()) < 6 * nw


def test_follows_weight_updates():
    """The bf16 stream is re-laid by the fp32 copy's triggers: a parameter overwrite + linna_weights_changed, an AdamW step."""
    prob = _custom_problem(33, 33, 77, 512, 4)
    prob = dict(prob, invcov=np.diag(np.diagonal(prob["invcov"])))
    w = np.diagonal(prob["invcov"]).copy()
    lp32, pred, _, _ = build_logprob(None, 1.0, prob)
    lp = as_bf16(lp32)
    model = pred.model
    z = (0.5 * np.random.RandomState(3).standard_normal((64, 33))).astype(np.float32)

    def check():
        sd = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
        p2 = dict(prob, weights=sd)
        got = lp(z, returntorch=False).astype(np.float64)
        emu, exact = bf16_emul.log_prob(z, p2, w, 1.0), bf16_emul.log_prob(z, p2, w, 1.0, rounded=False)
        rms, ref = np.sqrt(np.mean((got - emu) ** 2)), np.sqrt(np.mean((emu - exact) ** 2))
        assert rms <= 0.2 * ref, "bf16 output does not follow the weights: rms %.3e vs 0.2 * %.3e" % (rms, 0.2 * ref)
        return got

    a = check()
    with torch.no_grad():
        model.flat_params().mul_(1.01)
    _lib.call("linna_weights_changed", _lib.ctx(0))
    b = check()
    assert np.abs(a - b).max() > 1e-3
    n = model.flat_params().numel()
    g = torch.ones(n, device="cuda"); m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda")
    hyper = torch.tensor([1e-3, 0.0, 0.0, 0.0], device="cuda"); step = torch.zeros(1, dtype=torch.int32, device="cuda")
    flat = model.flat_params()
    _lib.call("linna_adamw_step", _lib.ctx(0), _lib.ptr(flat), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v),
              C.c_size_t(n), _lib.ptr(hyper), _lib.iptr(step), C.c_float(0.9), C.c_float(0.999), C.c_float(1e-8), 0,
              _lib.stream())
    c = check()
    assert np.abs(c - b).max() > 1e-3


def test_refusals_name_their_reason():
    """A dense inverse covariance, a network wider than 1024 and a gradient on a bf16 Log_prob each raise with a message;
    so do the C gradient entries on a bf16 handle."""
    import synth
    prob = cases.serving_problem("mlp_33_33_dense")
    lp = as_bf16(build_logprob(None, 1.0, prob)[0])
    z = np.zeros((4, 33), np.float32)
    with pytest.raises(ValueError, match="dense"):
        lp(z, returntorch=False)
    nin, nout = 12, 1100
    data, cov, priors = synth.gaussian_problem(nin, nout, 1200, dense=False, cond=1e2)
    X_mean, X_std, y_mean, y_std = synth.transform_constants(nin, nout, 1200)
    wide = dict(kind="ChtoModelv2", nin=nin, nout=nout, kw={}, weights=synth.weights("ChtoModelv2", nin, nout, 1200), priors=priors,
                data=data, cov=cov, invcov=np.linalg.inv(cov), sigma=np.sqrt(np.diag(cov)), X_mean=X_mean, X_std=X_std, y_mean=y_mean,
                y_std=y_std, dolog10=None, ypositive=False)
    lpw = as_bf16(build_logprob(None, 1.0, wide)[0])
    with pytest.raises(ValueError, match="1024"):
        lpw(np.zeros((4, nin), np.float32), returntorch=False)
    prob, _ = diag_problem("v2_33_33")
    lp = as_bf16(build_logprob(None, 1.0, prob)[0])
    zd = torch.zeros((8, 33), device="cuda")
    with pytest.raises(ValueError, match="gradient"):
        lp.evaluate_with_grad(zd)
    lp(np.zeros((8, 33), np.float32), returntorch=False)           # the handle exists and is bf16
    p = lp._ensure()
    out = C.c_int(-7)
    _lib.call("linna_logprob_precision", p["handle"], C.byref(out))
    assert out.value == 1
    ws = lp._workspace(8, True)
    lnp = torch.empty(8, device="cuda"); G = torch.empty((8, 33), device="cuda")
    rc = _lib.load().linna_logprob_grad(p["handle"], C.c_void_p(zd.data_ptr()), 33, 8, _lib.ptr(ws), _lib.ptr(lnp),
                                        C.c_void_p(G.data_ptr()), 33, _lib.stream())
    assert rc == _lib.ERR_UNSUPPORTED and "bf16" in _lib.load().linna_last_error().decode()


@pytest.mark.parametrize("name", ["v2_33_33", "mlp_33_33"])
def test_opt_in_only(name):
    """A default Log_prob returns bit-identical results before and after a bf16 handle exists on the same network."""
    prob, _ = diag_problem(name)
    lp32 = build_logprob(None, 1.0, prob)[0]
    z = (0.5 * np.random.RandomState(2).standard_normal((4096, 33))).astype(np.float32)
    before = lp32(z, returntorch=False)
    lpb = as_bf16(lp32)
    zb = lpb(z, returntorch=False)
    after = lp32(z, returntorch=False)
    assert np.array_equal(before, after), "fp32 results changed once a bf16 handle existed"
    assert not np.array_equal(zb, after), "the bf16 handle computed the fp32 values"
    assert lp32.precision == "fp32" and lpb.precision == "bf16"


def test_ml_sampler_core_bf16_end_to_end(tmp_path):
    """The reference's 2-D ``testmain`` configuration (test_ml_sampler_core_end_to_end) sampling through a bf16 emulator."""
    from linna_amd.main import ml_sampler_core
    from linna_amd.nn import ChtoModelv2
    from copy import deepcopy
    np.random.seed(0)
    ndim = 2
    init = np.random.uniform(size=ndim)
    cov = np.diag([0.5, 0.2])
    means = np.array([0.1, 1])
    priors = [{"param": "test_%d" % i, "dist": "flat", "arg1": -2.0, "arg2": 2.0} for i in range(ndim)]

    def theory(x, outdirs):
        return deepcopy(x[1])

    params = {"trainingoption": 1, "num_epochs": 10, "batch_size": 5}
    out = str(tmp_path) + "/2dgaussian/"
    chain, logprob = ml_sampler_core([20], [5], [1], [2], [0.5], [100], [100], out, theory, priors, means, cov, init, None, 4,
                                     "cuda", None, False, [1.0], omegab2cut=None, docuda=False, tsize=1, gpunode=None,
                                     nnmodel_in=ChtoModelv2, params=params, method="emcee", emulator_precision="bf16")
    assert chain.ndim == 2 and chain.shape[1] == ndim and len(chain) > 0
    assert np.all(np.isfinite(chain)) and np.all(np.abs(chain) <= 2.0)
