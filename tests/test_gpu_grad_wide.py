"""GPU: lnP and d lnP / d z in ONE launch of the whole-network kernel for networks with more than 64 outputs (fp32, diagonal
covariance): which route a call takes, parity with the layered route and the float64 oracle, independence of the rows, the
leapfrog in the finish, non-finite inputs, whole HMC transitions, and the <= 64-output launches next to them."""
import ctypes as C
import os

import numpy as np
import pytest

import cases
import parity
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from test_gpu_serving import build_logprob, _custom_problem  # noqa: E402
from test_gpu_bf16 import diag_problem  # noqa: E402

T = 2.0
# (nin, nout, width, depth): the first tail column of the turnaround (one lane only); a ragged second tail round; a SPLIT
# last layer of two column groups; of four; a WIDE last layer of one pass; of two passes; ChtoModelv2(26, 457)
MLPS = [(10, 65, 64, 1), (10, 97, 64, 1), (12, 100, 128, 2), (20, 250, 256, 3), (9, 457, 512, 2), (9, 700, 1000, 2)]
SHAPES = MLPS + ["v2_26_457"]
IDS = ["%d-%d-%d-%d" % s if isinstance(s, tuple) else s for s in SHAPES]
# ChtoModelv2(26, 457): ~3000 hidden units, so a row may sit on a ReLU kink (tests/parity.py near_relu_kink).  Seed 457 of
# the 300 test rows: the float64 oracle alone flags no row of them (checked on the CPU: seeds 457, 458 and 459 flag none,
# seed 460 flags rows 47 and 296), within the cap max(1, B // 200) of test_networks_wider_than_the_whole_network_kernel.
V2_SEED = 457
_SETS = {}


def the_set(shape):
    """Per shape, built once and left unchanged: the problem, the one-launch object, the layered object
    (LINNA_DISABLE_FUSED_GRAD=1 at creation), 300 rows and the float64 oracle's lnP and gradient at them."""
    if shape in _SETS:
        return _SETS[shape]
    from oracle import likelihood
    if isinstance(shape, tuple):
        nin, nout, width, depth = shape
        prob = _custom_problem(nin, nout, 900 + nout + width, width, depth)
        prob["dolog10"] = [0]                               # one input with a log10 prior (nin > 4 everywhere here)
        prob["priors"][0] = {"param": "p0", "dist": "flat", "arg1": 0.1, "arg2": 2.0}
        seed = 300 + nout
    else:
        prob, seed = diag_problem(shape)[0], V2_SEED
    fused = build_logprob(None, T, prob=prob)[0]
    fused._ensure()
    assert "LINNA_DISABLE_FUSED_GRAD" not in os.environ
    os.environ["LINNA_DISABLE_FUSED_GRAD"] = "1"            # linna_logprob_create reads the switch: create inside the window
    try:
        layered = build_logprob(None, T, prob=prob)[0]
        layered._ensure()
    finally:
        del os.environ["LINNA_DISABLE_FUSED_GRAD"]
    z = (0.6 * np.random.RandomState(seed).standard_normal((300, prob["nin"]))).astype(np.float32)
    emu = cases.oracle_emulator(prob)
    lref, gref = likelihood.grad_log_prob(z.astype(np.float64), emu, prob["priors"], prob["data"], prob["invcov"], T, dtype=np.float64)
    _SETS[shape] = dict(prob=prob, fused=fused, layered=layered, z=z, emu=emu, lref=lref, gref=gref)
    return _SETS[shape]


@pytest.fixture(autouse=True)
def automatic_engine():
    _lib.engine_rows(0)
    yield
    _lib.engine_rows(0)


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
    s = the_set(shape)
    on = [rows for rows in (16, 8, 4) if fits(s["fused"], rows)]
    assert 8 in on and 4 in on, on
    if isinstance(shape, tuple):
        assert on == [16, 8, 4]
    for rows in (16, 8, 4):
        _lib.engine_rows(rows)
        assert s["layered"].grad_launches(300) == 0
    # the automatic engines: 4 rows per workgroup up to 4 workgroups per CU's worth of rows, 8 up to 8, 16 beyond -- a batch
    # whose engine the program does not fit takes the layered route
    _lib.engine_rows(0)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    for B in (1, 17, 300, 4 * ncu, 4 * ncu + 1, 8 * ncu, 8 * ncu + 1, 16 * ncu):
        assert s["fused"].grad_launches(B) == (1 if B <= 8 * ncu or 16 in on else 0), B
        assert s["layered"].grad_launches(B) == 0, B


def test_route_of_a_dense_covariance_stays_layered():
    lp = build_logprob(None, T, prob=_custom_problem(12, 100, 1128, 128, 2, dense=True))[0]
    for B in (17, 300, 4096):
        assert lp.grad_launches(B) == 0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_parity_with_the_layered_route_and_the_oracle(shape):
    """Tolerances of test_fused_gradient_against_layered_path_and_oracle; lnP of the gradient launch against the serving
    launch as test_full_size_gradient_properties asserts it.  ChtoModelv2: a row beyond a gradient tolerance must sit on a
    ReLU kink, and at most max(1, B // 200) rows may."""
    s = the_set(shape)
    fused, layered = s["fused"], s["layered"]
    v2 = not isinstance(shape, tuple)
    for B, rows in ((1, 0), (17, 0), (300, 16), (300, 8), (300, 4)):
        _lib.engine_rows(rows)
        if rows and fused.grad_launches(B) == 0:
            assert rows == 16 and v2, (shape, rows)         # program + sign bits beyond the 16-row engine's LDS: the layered route there
            continue
        assert fused.grad_launches(B) == 1
        z, lref, gref = s["z"][:B], s["lref"][:B], s["gref"][:B]
        lf, gf = grad(fused, z)
        ll, gl = grad(layered, z)
        tag = "%s B %d rows %d" % (shape, B, rows)
        scale = np.abs(gl).max()
        print("%s: max |lnP - layered| %.3g, |lnP - oracle| / |lnP| %.3g, max |G - layered| / scale %.3g, max |G - oracle| / scale %.3g"
              % (tag, np.abs(lf - ll).max(), np.abs((lf - lref) / lref).max(), np.abs(gf - gl).max() / scale, np.abs(gf - gref).max() / scale))
        np.testing.assert_allclose(lf, ll, rtol=5e-6, atol=2e-5, err_msg=tag)
        np.testing.assert_allclose(lf, fused(z, returntorch=False).reshape(-1), rtol=4e-6, atol=4e-6, err_msg=tag)
        beyond = set(np.where((np.abs(gf - gl) > 2e-7 * scale + 2e-6 * np.abs(gl)).any(axis=1))[0])
        beyond |= set(np.where((np.abs(gf - gref) > 1e-5 * scale + 1e-4 * np.abs(gref)).any(axis=1))[0])
        if not v2:
            assert not beyond, (tag, sorted(beyond))
        assert len(beyond) <= max(1, B // 200), (tag, sorted(beyond))
        for r in beyond:
            assert parity.near_relu_kink(z[r], s["emu"], s["prob"]["priors"]), "%s: row %d differs away from any ReLU kink" % (tag, r)


def test_rows_are_independent():
    s = the_set((9, 457, 512, 2))
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
    separate linna_hmc_kick_drift entry's on that G; the pad columns of Q stay as they were."""
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
    s = the_set((10, 97, 64, 1))
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


def test_hmc_run_equals_the_step_loop():
    from linna_amd import sampler
    s = the_set((12, 100, 128, 2))
    lp, B, nd, nleap, e = s["fused"], 64, 12, 3, 2e-2
    assert lp.grad_launches(B) == 1
    x0 = (0.2 * np.random.RandomState(B).standard_normal((B, nd))).astype(np.float32)
    mass = np.linspace(0.5, 2.0, nd).astype(np.float32)
    a, b = sampler.BatchedHMC(lp, x0, mass=mass, seed=3), sampler.BatchedHMC(lp, x0, mass=mass, seed=3)
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


@pytest.mark.parametrize("name", ["v2_33_33", "mlp_33_33"])
def test_networks_of_at_most_64_outputs_run_as_before(name):
    """Their kernels keep their instructions (compared per symbol when the wide instantiations were added); here: still one
    launch on every engine, and evaluate_with_grad and the leapfrog entry agree bit for bit."""
    lp = build_logprob(name, T)[0]
    B, nin, ld = 300, 33, 36
    z = (0.5 * np.random.RandomState(12).standard_normal((B, nin))).astype(np.float32)
    h, ws = lp._ensure()["handle"], _lib.ptr(lp._workspace(B, True))
    for rows in (16, 8, 4):
        assert fits(lp, rows)
        lnp, g = grad(lp, z)
        q = np.zeros((B, ld), np.float32); q[:, :nin] = z
        Q, P = torch.as_tensor(q, device="cuda"), torch.zeros(B, ld, device="cuda")
        mass = torch.ones(nin, device="cuda")
        l2, g2 = torch.zeros(B, device="cuda"), torch.zeros(B, ld, device="cuda")
        _lib.call("linna_logprob_grad_leapfrog", h, _lib.ptr(Q), ld, B, ws, _lib.ptr(l2), _lib.ptr(g2), ld, _lib.ptr(P), ld,
                  _lib.ptr(mass), C.c_float(0.01), C.c_float(0.01), _lib.stream())
        torch.cuda.synchronize()
        np.testing.assert_array_equal(l2.cpu().numpy(), lnp)
        np.testing.assert_array_equal(g2.cpu().numpy()[:, :nin], g)
        assert np.all(np.isfinite(lnp)) and np.all(np.isfinite(g))
