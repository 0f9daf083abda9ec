"""GPU: lnP and d lnP / d z of a DENSE inverse covariance in ONE launch of the whole-network kernel (fp32, opt-in:
``Log_prob(dense_grad="fused")``): which route a call takes and what the option refuses, parity with the layered route and
the float64 oracle, an ill-conditioned covariance, exact integer tables, independence of the rows, the leapfrog in the
finish, non-finite inputs, whole HMC transitions, weight updates, and the factor's triangle modes."""
import ctypes as C

import numpy as np
import pytest

import cases
import parity
import net_exact as ne
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from test_gpu_serving import build_logprob, _custom_problem  # noqa: E402

T = 2.0
# (nin, nout, width, depth): SPLIT dense pair of one column group, U behind d in the same buffer; two column groups; four;
# WIDE, one pass, d in the other buffer; two passes; 16 column blocks (the forward factor's balanced mode); ChtoModelv2(26, 457)
# with its own dense covariance, 22 segments
MLPS = [(8, 33, 64, 2), (12, 100, 128, 2), (20, 250, 256, 3), (9, 457, 512, 2), (9, 700, 1000, 2), (10, 1000, 64, 1)]
SHAPES = MLPS + ["v2_26_457"]
IDS = ["%d-%d-%d-%d" % s if isinstance(s, tuple) else s for s in SHAPES]
V2_SEED = 457              # the 300 rows of tests/test_gpu_grad_wide.py: the float64 oracle alone flags no ReLU-kink row of them
_SETS = {}


def as_fused(lp):
    """A ``dense_grad="fused"`` Log_prob on the same emulator, data and priors as `lp`."""
    from linna_amd import util
    return util.Log_prob(lp.data_new, lp.invcov_new, lp.model, lp.y_invtransform_data, lp.transform, lp.T, lp.loglikelihoodfunc,
                         nograd=True, dense_grad="fused")


def the_set(shape):
    """Per shape, built once and left unchanged: the problem, the fused object, the layered (default) object, 300 rows and the
    float64 oracle's lnP and gradient at them."""
    if shape in _SETS:
        return _SETS[shape]
    from oracle import likelihood
    if isinstance(shape, tuple):
        nin, nout, width, depth = shape
        prob = _custom_problem(nin, nout, 900 + nout + width, width, depth, dense=True)
        prob["dolog10"] = [0]                               # one input with a log10 prior
        prob["priors"][0] = {"param": "p0", "dist": "flat", "arg1": 0.1, "arg2": 2.0}
        seed = 300 + nout
    else:
        prob, seed = cases.serving_problem(shape), V2_SEED   # dense as it stands
    layered = build_logprob(None, T, prob=prob)[0]
    layered._ensure()
    fused = as_fused(layered)
    fused._ensure()
    z = (0.6 * np.random.RandomState(seed).standard_normal((300, prob["nin"]))).astype(np.float32)
    emu = cases.oracle_emulator(prob)
    lref, gref = likelihood.grad_log_prob(z.astype(np.float64), emu, prob["priors"], prob["data"], prob["invcov"], T, dtype=np.float64)
    _SETS[shape] = dict(prob=prob, fused=fused, layered=layered, z=z, emu=emu, lref=lref, gref=gref)
    return _SETS[shape]


@pytest.fixture(autouse=True)
def automatic_engine():
    lib = _lib.load()
    tri = lib.linna_dense_tri(-1)
    _lib.engine_rows(0)
    yield
    _lib.engine_rows(0)
    lib.linna_dense_tri(tri)


def fits(lp, rows, B=300):
    """Whether the one-launch gradient runs on the forced engine `rows` (the engine is left forced)."""
    _lib.engine_rows(rows)
    return lp.grad_launches(B) == 1


def grad(lp, z):
    zd = torch.as_tensor(z, device="cuda")
    lnp, g = lp.evaluate_with_grad(zd)
    return lnp.cpu().numpy().copy(), g.cpu().numpy().copy()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_route(shape):
    from linna_amd import nn
    s = the_set(shape)
    assert s["fused"].dense_grad == "fused" and s["layered"].dense_grad == "layered"
    out = C.c_int(-1)
    _lib.call("linna_logprob_dense_grad", s["fused"]._ensure()["handle"], C.byref(out)); assert out.value == 1
    _lib.call("linna_logprob_dense_grad", s["layered"]._ensure()["handle"], C.byref(out)); assert out.value == 0
    # the engines the planner names are the engines the route takes: 1 on every engine that fits, 0 elsewhere
    txt = nn.describe_grad_dense_program(s["fused"].model.model, 8)[1].strip().splitlines()[-1]
    planned = [int(r) for r in txt.split("(rows")[1].rstrip(")").split()]
    on = [rows for rows in (16, 8, 4) if fits(s["fused"], rows)]
    assert on == planned and 8 in on and 4 in on, (on, txt)
    if isinstance(shape, tuple):
        assert on == [16, 8, 4]
    for rows in (16, 8, 4):
        _lib.engine_rows(rows)
        assert s["layered"].grad_launches(300) == 0
    _lib.engine_rows(0)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (1, 17, 300, 4 * ncu, 4 * ncu + 1, 8 * ncu, 8 * ncu + 1, 16 * ncu):
        assert s["fused"].grad_launches(B) == (1 if B <= 8 * ncu or 16 in on else 0), B
        assert s["layered"].grad_launches(B) == 0, B
    # switching the option off on the handle gives the layered route back, and on again the one launch
    h = s["fused"]._ensure()["handle"]
    try:
        _lib.call("linna_logprob_set_dense_grad", h, 0)
        assert s["fused"].grad_launches(17) == 0
    finally:
        _lib.call("linna_logprob_set_dense_grad", h, 1)
    assert s["fused"].grad_launches(17) == 1


def test_what_the_option_refuses(monkeypatch):
    from linna_amd import util
    from test_gpu_bf16 import diag_problem
    sib = lambda lp, **kw: util.Log_prob(lp.data_new, lp.invcov_new, lp.model, lp.y_invtransform_data, lp.transform, lp.T,
                                         lp.loglikelihoodfunc, nograd=True, dense_grad="fused", **kw)
    # a diagonal covariance
    lp = build_logprob(None, T, prob=_custom_problem(8, 33, 997, 64, 2))[0]
    with pytest.raises(ValueError, match="diagonal"):
        sib(lp)._ensure()
    # bf16 (a diagonal problem: bf16 serves nothing else)
    with pytest.raises(ValueError):
        sib(build_logprob(None, T, prob=diag_problem("v2_33_33")[0])[0], precision="bf16")._ensure()
    # an indefinite inverse covariance (how="singular" of test_dense_covariance_in_the_direct_form_as_a_side_segment): no factor
    prob = _custom_problem(8, 33, 900 + 33, 64, 2, dense=True)
    w, v = np.linalg.eigh(prob["invcov"])
    w[:3] = 0.0
    prob["invcov"] = (v * w[None, :]) @ v.T
    lp = build_logprob(None, T, prob=prob)[0]
    assert "Sfac" not in lp._ensure()["keep"]
    with pytest.raises(ValueError, match="Sfac"):
        sib(lp)._ensure()
    assert lp.grad_launches(17) == 0
    # ... and the direct form on request
    monkeypatch.setenv("LINNA_DENSE_FACTORED", "0")
    with pytest.raises(ValueError, match="LINNA_DENSE_FACTORED"):
        sib(build_logprob(None, T, prob=_custom_problem(8, 33, 933, 64, 2, dense=True))[0])._ensure()


# Tolerances: lnP rtol 2e-5 (the dense serving tolerance of test_dense_covariance_as_last_segment); the gradient rtol 1e-4,
# atol 1e-5 max|G| (test_fused_gradient_against_layered_path_and_oracle).  The layered route's errors on the same rows are
# printed beside the fused route's and recorded (parity._record).
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_parity_with_the_layered_route_and_the_oracle(shape):
    s = the_set(shape)
    fused, layered = s["fused"], s["layered"]
    v2 = not isinstance(shape, tuple)
    for B, rows in ((1, 0), (17, 0), (300, 16), (300, 8), (300, 4)):
        _lib.engine_rows(rows)
        if rows and fused.grad_launches(B) == 0:
            assert rows == 16 and v2, (shape, rows)         # the program beyond the 16-row engine's LDS: the layered route there
            continue
        assert fused.grad_launches(B) == 1 and layered.grad_launches(B) == 0
        z, lref, gref = s["z"][:B], s["lref"][:B], s["gref"][:B]
        lf, gf = grad(fused, z)
        ll, gl = grad(layered, z)
        le = fused.evaluate(torch.as_tensor(z, device="cuda")).cpu().numpy()
        tag = "%s B %d rows %d" % (shape, B, rows)
        scale = np.abs(gref).max()
        print("%s: |lnP - oracle| / |lnP| fused %.3g layered %.3g; |lnP - evaluate| / |lnP| %.3g; max |G - oracle| / max|G| fused %.3g layered %.3g"
              % (tag, np.abs((lf - lref) / lref).max(), np.abs((ll - lref) / lref).max(), np.abs((lf - le) / le).max(),
                 np.abs(gf - gref).max() / scale, np.abs(gl - gref).max() / scale))
        if parity.REPORT:
            parity._record("dense_grad.fused.lnP", lf, lref, 2e-5, 0.0)
            parity._record("dense_grad.layered.lnP", ll, lref, 2e-5, 0.0)
            parity._record("dense_grad.fused.G", gf, gref, 1e-4, 1e-5 * scale)
            parity._record("dense_grad.layered.G", gl, gref, 1e-4, 1e-5 * scale)
        np.testing.assert_allclose(lf, lref, rtol=2e-5, err_msg=tag)
        np.testing.assert_allclose(lf, le, rtol=2e-5, err_msg=tag)
        if not v2:
            np.testing.assert_allclose(gf, gref, rtol=1e-4, atol=1e-5 * scale, err_msg=tag)
            continue
        # ChtoModelv2: ~3000 hidden units -- a row beyond the tolerance must sit on a ReLU kink, and at most max(1, B // 200) may
        beyond = np.where((np.abs(gf - gref) > 1e-5 * scale + 1e-4 * np.abs(gref)).any(axis=1))[0]
        assert len(beyond) <= max(1, B // 200), (tag, sorted(beyond))
        for r in beyond:
            assert parity.near_relu_kink(z[r], s["emu"], s["prob"]["priors"]), "%s: row %d differs away from any ReLU kink" % (tag, r)


def test_ill_conditioned_covariance(capsys):
    """The condition-1e6 problem of tests/test_gpu_cond.py with the numbers that file asserts for the layered route: lnP within
    bound(l64, cond, True), the gradient within 6e-4 of the row maximum against float64."""
    import test_gpu_cond as tc
    from oracle import likelihood
    g = cases.golden(tc.NAME)
    ci = len(g["conds"]) - 1
    worst = []
    for k in range(g["z"].shape[0]):
        prob, cond = tc.problem(ci, k, g)
        layered = build_logprob(None, 1.0, prob)[0]
        fused = as_fused(layered)
        B = len(g["z"][k])
        assert fused.grad_launches(B) == 1 and layered.grad_launches(B) == 0
        lf, gf = grad(fused, g["z"][k])
        ll, gl = grad(layered, g["z"][k])
        l64 = tc.truth64(prob, g["z"][k])
        _, g64 = likelihood.grad_log_prob(g["z"][k], cases.oracle_emulator(prob), prob["priors"], prob["data"].astype(np.float32),
                                          prob["invcov"].astype(np.float32), 1.0, dtype=np.float64)
        rowmax = np.abs(g64).max(axis=1, keepdims=True)
        b = tc.bound(l64, cond, True)
        ef, el = (np.abs(gf - g64) / rowmax).max(), (np.abs(gl - g64) / rowmax).max()
        worst.append(((np.abs(lf - l64) / b).max(), (np.abs(ll - l64) / b).max(), ef, el))
        assert np.all(np.abs(lf - l64) <= b), (k, worst[-1])
        assert ef <= 6e-4, (k, ef, el)
    with capsys.disabled():
        print("\ncondition 1e6: worst |lnP - f64| / bound fused %.3g layered %.3g; worst |G - g64| / row max fused %.3g layered %.3g" % (
            max(w[0] for w in worst), max(w[1] for w in worst), max(w[2] for w in worst), max(w[3] for w in worst)))


def exact_logprob(name):
    """tests/test_gpu_net_exact.py's dense serving object, with the option on."""
    from linna_amd import predictor_gpu, util
    c = ne.serving_consts(name, "dense")
    c["y_std"], c["sigma"], c["y_mean"], c["data"] = np.ones(c["nout"]), np.ones(c["nout"]), np.zeros(c["nout"]), np.zeros(c["nout"])
    t = lambda a: torch.as_tensor(np.asarray(a, ne.F))
    Xt = util.X_transform_class(t(c["X_mean"]), t(c["X_std"]), "cpu", None)
    Yt = util.Y_transform_class(t(c["y_mean"]), t(c["y_std"]), "cpu", ypositive=False)
    pred = predictor_gpu.Predictor(c["nin"], c["nout"], model=ne.fresh_model(name), X_transform=Xt, y_transform=Yt, device="cuda")
    yinv = util.Y_invtransform_data(np.asarray(c["sigma"], ne.F), "cpu")
    lp = util.Log_prob(t(c["data"]), t(c["invcov"]), pred, yinv, util.Transform(c["priors"]), c["T"], util.gaussianlogliklihood, nograd=True,
                       dense_grad="fused")
    lp._ensure()
    c["cscale"], c["cshift"] = np.ones(c["nout"]), np.zeros(c["nout"])
    return lp, pred.model, c


@pytest.mark.parametrize("name", ["dense33", "dense1000"])
def test_exact_integer_tables(name):
    """Small-integer weights, an integer lower-triangular L of unit-magnitude entries (net_exact.dense_factor: diagonal from
    {1, 2}), T a power of two, the identity output map: every product and partial sum is exact in fp32, so lnP and G equal
    the integer reference BIT FOR BIT on every engine -- a misplaced element of L or L^T in the stream cannot hide behind a
    tolerance.  dense33: U behind d in the same buffer; dense1000: two passes (and the forward factor's balanced mode)."""
    lp, model, c = exact_logprob(name)
    ops = ne.model(name).ops
    n = ne.n_maps(name)
    for dense, B in ((n - 1, ne.ROWS), (0, ne.ROWS), (n - 1, 33)):
        P = ne.weights(name, dense)
        z = ne.z_of(c, ne.inputs(name, dense, B))
        ref = ne.serving_ref(ops, P, c, z, grad=True)
        # the exactness conditions, on the CPU: every sum's |terms| below 2^24 quanta (integers in front of the turnaround,
        # multiples of 1 / T behind it, halves and eighths in lnP)
        assert ne.exact_sum(ref["terms"])
        assert all(float(np.abs(t).max()) < 2.0 ** 24 for t in ref["mid_terms"])
        assert all(float(np.abs(t).max()) < 2.0 ** 24 / float(c["T"]) for t in ref["bterms"])
        model.load_state_dict({k: torch.as_tensor(v) for k, v in P.items()})
        first = None
        for rows in ne.ENGINES:
            assert fits(lp, rows, B), (name, rows)
            lnp, g = grad(lp, z)
            tag = "%s dense map %d rows %d engine %d" % (name, dense, B, rows)
            assert np.array_equal(lnp, ref["lnP"].astype(ne.F)) and np.array_equal(ref["lnP"].astype(ne.F).astype(np.float64), ref["lnP"]), tag + " lnP"
            assert np.array_equal(ref["G"].astype(ne.F).astype(np.float64), ref["G"]), tag
            bad = np.argwhere(g != ref["G"].astype(ne.F))
            assert not len(bad), "%s G: %d elements differ, first at %s: %r against %r" % (tag, len(bad), tuple(bad[0]), g[tuple(bad[0])], ref["G"][tuple(bad[0])])
            first = (lnp, g) if first is None else first
            assert np.array_equal(lnp, first[0]) and np.array_equal(g, first[1]), tag


def test_rows_are_independent():
    for shape in ((8, 33, 64, 2), (9, 700, 1000, 2)):
        s = the_set(shape)
        z = s["z"]
        for rows in (16, 8, 4):
            assert fits(s["fused"], rows)
            lnp, g = grad(s["fused"], z)
            perm = np.random.RandomState(3).permutation(len(z))
            lp_, gp_ = grad(s["fused"], z[perm])
            np.testing.assert_array_equal(lp_, lnp[perm])
            np.testing.assert_array_equal(gp_, g[perm])
            lr, gr = grad(s["fused"], np.repeat(z[7:8], 33, axis=0))
            assert np.all(lr == lr[0]) and np.all(gr == gr[0])
            assert np.all(np.isfinite(lnp)) and np.all(np.isfinite(g))


@pytest.mark.parametrize("shape", [(12, 100, 128, 2), (9, 457, 512, 2)], ids=["12-100-128-2", "9-457-512-2"])
@pytest.mark.parametrize("B", [17, 300])
def test_leapfrog_in_the_finish(shape, B):
    """linna_logprob_grad_leapfrog and _eps (a constant array): lnP and G are linna_logprob_grad's bits; P and Q are the
    separate linna_hmc_kick_drift entry's on that G; the pad columns of Q and P stay as they were."""
    s = the_set(shape)
    lp = s["fused"]
    assert lp.grad_launches(B) == 1
    h, ws = lp._ensure()["handle"], _lib.ptr(lp._workspace(B, True))
    nin, ld = shape[0], 16
    rs = np.random.RandomState(B)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32), device="cuda")
    q0 = np.full((B, ld), 7.0, np.float32); q0[:, :nin] = s["z"][:B]
    p0 = np.full((B, ld), 5.0, np.float32); p0[:, :nin] = rs.standard_normal((B, nin))
    mass = dev(np.linspace(0.5, 2.0, nin))
    eps = 0.0125
    lnp, g = torch.zeros(B, device="cuda"), torch.zeros(B, ld, device="cuda")
    Q = dev(q0)
    _lib.call("linna_logprob_grad", h, _lib.ptr(Q), ld, B, ws, _lib.ptr(lnp), _lib.ptr(g), ld, _lib.stream())
    for ek, ed in ((1.0, 1.0), (0.5, 0.0)):                  # a full step; the last half kick without a drift
        P, Qs = dev(p0), dev(q0)
        _lib.call("linna_hmc_kick_drift", _lib.ctx(0), B, nin, _lib.ptr(mass), C.c_float(ek * eps), C.c_float(ed * eps), _lib.ptr(g), ld,
                  _lib.ptr(P), ld, _lib.ptr(Qs), ld, _lib.stream())
        for form in ("scalar", "array"):
            P2, Q2 = dev(p0), dev(q0)
            l2, g2 = torch.zeros(B, device="cuda"), torch.zeros(B, ld, device="cuda")
            if form == "scalar":
                _lib.call("linna_logprob_grad_leapfrog", h, _lib.ptr(Q2), ld, B, ws, _lib.ptr(l2), _lib.ptr(g2), ld, _lib.ptr(P2), ld,
                          _lib.ptr(mass), C.c_float(ek * eps), C.c_float(ed * eps), _lib.stream())
            else:
                E = torch.full((B,), eps, device="cuda")
                _lib.call("linna_logprob_grad_leapfrog_eps", h, _lib.ptr(Q2), ld, B, ws, _lib.ptr(l2), _lib.ptr(g2), ld, _lib.ptr(P2), ld,
                          _lib.ptr(mass), _lib.ptr(E), C.c_float(ek), C.c_float(ed), _lib.stream())
            torch.cuda.synchronize()
            what = (shape, B, ek, ed, form)
            assert torch.equal(l2, lnp) and torch.equal(g2[:, :nin], g[:, :nin]), what
            assert torch.equal(P2[:, :nin], P[:, :nin]) and torch.equal(Q2[:, :nin], Qs[:, :nin]), what
            assert bool((Q2[:, nin:] == 7.0).all()) and bool((P2[:, nin:] == 5.0).all()), what
            if ed == 0.0:
                assert torch.equal(Q2, dev(q0)), what
            else:
                assert not torch.equal(Q2[:, :nin], dev(q0)[:, :nin]), what


def test_a_non_finite_row_is_minus_infinity_and_leaves_its_neighbours_alone():
    for shape in ((8, 33, 64, 2), (9, 457, 512, 2)):
        s = the_set(shape)
        z = s["z"][:40].copy()
        for rows in (16, 4):
            assert fits(s["fused"], rows, 40)
            base_l, base_g = grad(s["fused"], z)
            bad = z.copy()
            bad[5, 3] = np.nan
            bad[22, 0] = np.inf
            l, g = grad(s["fused"], bad)
            assert l[5] == -np.inf and l[22] == -np.inf
            keep = np.setdiff1d(np.arange(40), [5, 22])
            np.testing.assert_array_equal(l[keep], base_l[keep])
            np.testing.assert_array_equal(g[keep], base_g[keep])


@pytest.mark.parametrize("dense_mass", [False, True], ids=["diag-mass", "dense-mass"])
def test_hmc_run_equals_the_step_loop(dense_mass):
    from linna_amd import sampler
    s = the_set((12, 100, 128, 2))
    lp, B, nd, nleap, e = s["fused"], 64, 12, 3, 2e-3
    assert lp.grad_launches(B) == 1
    x0 = (0.2 * np.random.RandomState(B).standard_normal((B, nd))).astype(np.float32)
    if dense_mass:                                          # adapt_mass="dense"'s whitened route: a dense mass from the start
        A = np.random.RandomState(5).standard_normal((nd, nd))
        mass = A @ A.T / nd + np.diag(np.linspace(0.5, 2.0, nd))
    else:
        mass = np.linspace(0.5, 2.0, nd).astype(np.float32)
    a, b = sampler.BatchedHMC(lp, x0, mass=mass, seed=3), sampler.BatchedHMC(lp, x0, mass=mass, seed=3)
    assert (a.chol is not None) == dense_mass
    a.eps.fill_(e)
    chain, lnp = a.run(8, nleap, Madapt=0)
    want_c, want_l = torch.empty_like(chain), torch.empty_like(lnp)
    for i in range(8):
        b.step(nleap, e)
        want_c[i].copy_(b.x[:, :nd]); want_l[i].copy_(b.lnp)
    torch.cuda.synchronize()
    assert torch.equal(chain, want_c) and torch.equal(lnp, want_l)
    assert torch.equal(a.naccept, b.naccept) and 0 < int(a.naccept.sum()) <= 8 * B
    assert bool(torch.isfinite(lnp).all())


def test_the_stream_follows_weight_updates():
    """The fused route reads a copy of the weights laid out for its program -- the folded output map forward and backward,
    the factor and its transpose: after a write to the network's weights (linna_weights_changed through the accessor) it
    follows the layered route, which reads them where they are."""
    prob = _custom_problem(12, 100, 77, 128, 2, dense=True)
    layered = build_logprob(None, T, prob=prob)[0]
    fused = as_fused(layered)
    model = layered.model.model
    z = (0.5 * np.random.RandomState(3).standard_normal((64, 12))).astype(np.float32)
    assert fused.grad_launches(64) == 1 and layered.grad_launches(64) == 0

    def check():
        lf, gf = grad(fused, z)
        ll, gl = grad(layered, z)
        np.testing.assert_allclose(lf, ll, rtol=2e-5)
        np.testing.assert_allclose(gf, gl, rtol=1e-4, atol=1e-5 * np.abs(gl).max())
        return lf, gf

    l0, g0 = check()
    model.flat_params().mul_(1.02)
    l1, g1 = check()
    assert np.abs(l1 - l0).max() > 1e-3 * np.abs(l0).max() and np.abs(g1 - g0).max() > 1e-3 * np.abs(g0).max()
    _lib.call("linna_weights_changed", _lib.ctx(0))        # the entry itself, with nothing changed: the same bits
    l2, g2 = grad(fused, z)
    assert np.array_equal(l2, l1) and np.array_equal(g2, g1)


@pytest.mark.parametrize("nout", [700, 1000])
def test_triangle_modes_of_the_forward_factor_are_bit_identical(nout):
    """The forward dense segment keeps linna_dense_tri's modes (the transposed one multiplies every zero in each): lnP and G
    identical bit for bit under modes 0 / 1 / 2 -- the skipped products are zeros."""
    lib = _lib.load()
    s = the_set((9, 700, 1000, 2) if nout == 700 else (10, 1000, 64, 1))
    z = s["z"][:40]
    for rows in (16, 4):
        got = {}
        for mode in (0, 1, 2):
            lib.linna_dense_tri(mode)                       # (applies to objects created afterwards)
            lp = as_fused(s["layered"])
            assert fits(lp, rows, 40)
            got[mode] = grad(lp, z)
        for mode in (1, 2):
            assert np.array_equal(got[mode][0], got[0][0]) and np.array_equal(got[mode][1], got[0][1]), (nout, rows, mode)
