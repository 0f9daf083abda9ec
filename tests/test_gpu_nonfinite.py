"""GPU: non-finite points through serving, the gradient and every move.

A point whose transformed network input is NaN or -inf while z itself is finite (tests/poison.py: log10 of a parameter
<= 0) is a REJECTED point in the reference (NaN -> -inf, util.py:1013-1016).  Here: lnP = -inf exactly on every path, the
other rows of the batch untouched bit for bit, and no move ever takes such a point -- against the oracle, the clean twin of
the batch, and the scenarios tests/test_nonfinite_host.py pins on the oracle alone."""
import ctypes as C

import numpy as np
import pytest

import poison
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from test_gpu_serving import build_logprob  # noqa: E402

BAD = sorted(poison.SERVING_ROWS)
SERVING = ["mlp_7_5_small", "simple_6_4", "v2_33_33", "v2lin_5_3_log10", "mlp_33_33_dense", "v2_26_457", "v2_4_2_ypos"]
GRAD = [n for n in SERVING if n != "v2_4_2_ypos"]                 # (the exp output map has no gradient entry: it raises)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32), device="cuda")


_ORACLE = {}


def oracle(name, diag=False):
    """(prob, z, twin, lnP float64 of z, theta of z), computed once per problem and shared read-only."""
    key = (name, diag)
    if key not in _ORACLE:
        from oracle import likelihood
        prob = poison.poisoned_problem(name, (0, 1))
        if diag:
            prob = poison.diagonal(prob)
        z, twin = poison.batch(prob["nin"])
        ref = poison.oracle_fn(prob, 1.0, np.float64)(z)
        th = likelihood.prior_map(z, prob["priors"])
        for a in (z, twin, ref, th):
            a.setflags(write=False)
        _ORACLE[key] = (prob, z, twin, ref, th)
    return _ORACLE[key]


def check_lnp(got, ref, what):
    """The non-finite rows are the oracle's, each exactly -inf; nothing is NaN or +inf."""
    bad = ~np.isfinite(ref)
    assert list(np.flatnonzero(bad)) == BAD
    print("  %-46s lnP of the poisoned rows %s" % (what, got[bad]))
    assert not np.isnan(got).any() and not np.any(got == np.inf), (what, got)
    assert np.array_equal(~np.isfinite(got), bad), (what, np.flatnonzero(~np.isfinite(got)), got[bad])
    assert np.all(got[bad] == -np.inf), (what, got[bad])
    return ~bad


def serve(lp, z, twin, ref, th, what):
    zd, td = dev(z), dev(twin)
    theta = torch.full_like(zd, 7.0)
    got = lp.evaluate(zd, theta=theta).cpu().numpy()
    clean = lp.evaluate(td).cpu().numpy()
    ok = check_lnp(got, ref, what)
    assert np.all(np.isfinite(clean)), what
    np.testing.assert_array_equal(got[ok], clean[ok], err_msg=what)            # a poisoned row leaves its neighbours alone
    np.testing.assert_array_equal(theta.cpu().numpy()[BAD, 0], th[BAD, 0], err_msg=what)     # -0.5, 0, -2, -0.5: exact in fp32
    np.testing.assert_array_equal(th[BAD, 0], np.float32([-0.5, 0.0, -2.0, -0.5]))
    np.testing.assert_allclose(theta.cpu().numpy()[ok], th[ok], rtol=1e-5, atol=1e-5, err_msg=what)
    return got, ok


@pytest.mark.parametrize("name", SERVING)
def test_serving_rejects_a_nonfinite_input_on_every_path(name, monkeypatch):
    """B = 37, rows 0 / 36 at theta0 = -0.5, row 15 at theta0 = 0 exactly, row 16 at theta0 = -2: the whole-network kernel on
    each engine (4, 8, 16 rows and the one the batch selects), the layer-by-layer path, and the bf16 engine where the
    handle takes it (a diagonal covariance).  What the test guards against: a ReLU written as fmaxf returns 0 on a NaN, so
    the layers turn a NaN input into a finite, meaningless lnP -- see DESIGN.md section 4."""
    prob, z, twin, ref, th = oracle(name)
    lp = build_logprob(None, 1.0, prob=prob)[0]
    try:
        for rows in (4, 8, 16, 0):
            _lib.engine_rows(rows)
            got, ok = serve(lp, z, twin, ref, th, "%s engine rows %d" % (name, rows))
            np.testing.assert_allclose(got[ok], ref[ok], rtol=1.5e-5, err_msg="%s rows %d" % (name, rows))
    finally:
        _lib.engine_rows(0)
    monkeypatch.setenv("LINNA_DISABLE_FUSED", "1")            # read when the log-probability object is created
    layered = build_logprob(None, 1.0, prob=prob)[0]
    layered._ensure()
    monkeypatch.delenv("LINNA_DISABLE_FUSED")
    got, ok = serve(layered, z, twin, ref, th, "%s layer by layer" % name)
    np.testing.assert_allclose(got[ok], ref[ok], rtol=1.5e-5, err_msg="%s layered" % name)
    # bf16: where the handle accepts it -- the bound of tests/test_gpu_bf16.py (test_error_bound_against_the_exact_network)
    from test_gpu_bf16 import as_bf16, sensitivity, _lnp_bound
    import bf16_emul
    dprob, dz, dtwin, dref, dth = oracle(name, diag=True)
    try:
        lpb = as_bf16(build_logprob(None, 1.0, prob=dprob)[0])
        lpb._ensure()
    except ValueError as e:                                   # (an input skip, ...: the engine says why it refuses)
        print("  %s: no bf16 engine (%s)" % (name, e))
        return
    w = np.diagonal(np.asarray(dprob["invcov"], np.float64)).copy()
    got, ok = serve(lpb, dz, dtwin, dref, dth, "%s bf16" % name)
    L = bf16_emul.stages(dprob["kind"], dprob["nin"], dprob["nout"], **dprob["kw"])
    h, A = sensitivity(dprob, w, dz[ok], 1.0)
    bound = _lnp_bound(dprob, w, h, A, 1.0, L + 1) + 1e-5 * (1 + np.abs(dref[ok]))
    err = np.abs(got[ok].astype(np.float64) - dref[ok])
    assert np.all(err <= bound), "%s bf16: |dlnP| reaches %.3g of its bound" % (name, np.max(err / bound))


def test_a_dense_likelihood_launch_behind_the_network_sees_the_poisoned_row(monkeypatch):
    """LINNA_DENSE_FUSED=0: the whole-network kernel writes d = m - data and a row-dot launch turns it into lnP -- the
    poison has to travel in d."""
    prob, z, twin, ref, th = oracle("mlp_33_33_dense")
    monkeypatch.setenv("LINNA_DENSE_FUSED", "0")
    lp = build_logprob(None, 1.0, prob=prob)[0]
    lp._ensure()
    monkeypatch.delenv("LINNA_DENSE_FUSED")
    got, ok = serve(lp, z, twin, ref, th, "mlp_33_33_dense, network launch + row-dot")
    np.testing.assert_allclose(got[ok], ref[ok], rtol=1.5e-5)


def grad_all(lp, z, leap):
    """(lnP, G, P, Q) as device tensors: ``evaluate_with_grad``, or linna_logprob_grad_leapfrog with a kick and a drift."""
    zd = dev(z)
    B, nd = zd.shape
    if not leap:
        l, g = lp.evaluate_with_grad(zd)
        return l, g, None, None
    ld = _lib.ld4(nd)
    Q = torch.zeros((B, ld), device="cuda"); Q[:, :nd].copy_(zd)
    P = torch.zeros((B, ld), device="cuda"); P[:, :nd].copy_(dev(0.3 * np.random.RandomState(3).standard_normal((B, nd))))
    G = torch.zeros((B, ld), device="cuda")
    l = torch.zeros(B, device="cuda")
    mass = dev(np.linspace(0.5, 2.0, nd))
    p = lp._ensure()
    _lib.call("linna_logprob_grad_leapfrog", p["handle"], _lib.ptr(Q), ld, B, _lib.ptr(lp._workspace(B, True)), _lib.ptr(l),
              _lib.ptr(G), ld, _lib.ptr(P), ld, _lib.ptr(mass), 0.01, 0.02, _lib.stream())
    torch.cuda.synchronize()
    return l, G[:, :nd], P[:, :nd], Q[:, :nd]


def check_grad(lp, z, twin, ref, what):
    for leap in (False, True):
        a = grad_all(lp, z, leap)
        b = grad_all(lp, twin, leap)
        w = what + (", leapfrog entry" if leap else "")
        ok = check_lnp(a[0].cpu().numpy(), ref, w)
        assert torch.isfinite(b[0]).all() and torch.isfinite(b[1]).all(), w
        for nm, ta, tb in zip(("lnP", "G", "P", "Q"), a, b):
            if ta is not None:                                     # (int32 views: equal NaNs would compare unequal)
                np.testing.assert_array_equal(bits(ta)[ok], bits(tb)[ok], err_msg="%s: %s of the clean rows" % (w, nm))
        assert np.all(np.isfinite(a[1].cpu().numpy()[ok]))


@pytest.mark.parametrize("name", GRAD)
def test_gradient_rejects_a_nonfinite_input_on_every_path(name, monkeypatch):
    """The serving batch through ``evaluate_with_grad`` and linna_logprob_grad_leapfrog: the one-launch form (each engine),
    LINNA_DISABLE_FUSED_GRAD=1 (forward with stored activations + dX chain), and the bf16 gradient where the handle takes
    it.  lnP = -inf on exactly the poisoned rows; lnP, G, P and Q of the clean rows are those of the clean twin, bit for bit.
    G, P, Q of a poisoned row are unspecified (autograd gives NaN; the Metropolis test discards them)."""
    prob, z, twin, ref, th = oracle(name)
    lp = build_logprob(None, 1.0, prob=prob)[0]
    try:
        for rows in (0, 4, 16):
            _lib.engine_rows(rows)
            check_grad(lp, z, twin, ref, "%s gradient, engine rows %d" % (name, rows))
    finally:
        _lib.engine_rows(0)
    monkeypatch.setenv("LINNA_DISABLE_FUSED_GRAD", "1")
    layered = build_logprob(None, 1.0, prob=prob)[0]
    layered._ensure()
    monkeypatch.delenv("LINNA_DISABLE_FUSED_GRAD")
    check_grad(layered, z, twin, ref, "%s gradient, layered" % name)
    from test_gpu_bf16_grad import as_bf16_grad
    dprob, dz, dtwin, dref, dth = oracle(name, diag=True)
    try:
        lpb = as_bf16_grad(build_logprob(None, 1.0, prob=dprob)[0])
        lpb._ensure()
    except ValueError as e:
        print("  %s: no bf16 gradient (%s)" % (name, e))
        return
    check_grad(lpb, dz, dtwin, dref, "%s gradient, bf16" % name)


@pytest.mark.parametrize("ndim", [7, 70])
def test_hmc_acceptance_table(ndim):
    """linna_hmc_accept on given numbers, one row per case (tests/poison.py ``hmc_table``): accepted exactly where
    ``u < exp(minimum(H0 - H1, 0)) & isfinite(lnp_new)`` says so in numpy -- a NaN energy (NaN in P, H0 NaN) REJECTS, as
    HMCSampler.py:57-59 does -- and X, lnp, G, naccept of a rejected row are untouched.  With
    ``expf(fminf(dH, 0))`` the rows "NaN in P" and "H0 NaN" are accepted: ``fminf(NaN, 0)`` is 0."""
    t = poison.hmc_table(ndim)
    want = poison.hmc_table_expected(t)
    B, ld = 11, _lib.ld4(ndim)

    def pad(a):
        out = torch.zeros((B, ld), device="cuda")
        out[:, :ndim].copy_(dev(a))
        return out
    P, Qn, Gn, X, G = (pad(t[k]) for k in ("P", "Qnew", "Gnew", "X", "G"))
    U, H0, lnp_new, lnp, mass = (dev(t[k]) for k in ("U", "H0", "lnp_new", "lnp", "mass"))
    nacc = torch.zeros(B, dtype=torch.int32, device="cuda")
    step = torch.zeros(1, dtype=torch.int32, device="cuda")
    X0, G0, lnp0 = bits(X).copy(), bits(G).copy(), bits(lnp).copy()
    _lib.call("linna_hmc_accept", _lib.ctx(), B, ndim, _lib.ptr(mass), C.c_uint64(1), _lib.iptr(step), _lib.ptr(H0), _lib.ptr(P), ld,
              _lib.ptr(Qn), ld, _lib.ptr(lnp_new), _lib.ptr(Gn), ld, _lib.ptr(U), _lib.ptr(X), ld, _lib.ptr(lnp), _lib.ptr(G),
              _lib.iptr(nacc), _lib.stream())
    torch.cuda.synchronize()
    got = nacc.cpu().numpy().astype(bool)
    print("  accepted: " + ", ".join("%s=%d" % (w, g) for w, g in zip(t["what"], got)))
    np.testing.assert_array_equal(got, want, err_msg=str(list(zip(t["what"], got, want))))
    assert nacc.max().item() == 1
    rej = ~want
    np.testing.assert_array_equal(bits(X)[rej], X0[rej])
    np.testing.assert_array_equal(bits(G)[rej], G0[rej])
    np.testing.assert_array_equal(bits(lnp)[rej], lnp0[rej])
    np.testing.assert_array_equal(bits(X)[want], bits(Qn)[want])
    np.testing.assert_array_equal(bits(G)[want], bits(Gn)[want])
    np.testing.assert_array_equal(bits(lnp)[want], bits(lnp_new)[want])


def test_hmc_transition_never_takes_a_rejected_point():
    """BatchedHMC.step on poisoned mlp_7_5_small, 64 chains next to theta0 = 0, a step size at which a third of the oracle's
    trajectories end at -inf (tests/test_nonfinite_host.py): the oracle's decisions, those chains exactly where they
    were, fused and unfused equal bit for bit."""
    from oracle import sampling
    from linna_amd import sampler
    s = poison.HMC
    prob = poison.poisoned_problem(s["name"])
    lp = build_logprob(None, s["T"], prob=prob)[0]
    fg = poison.oracle_grad_fn(prob, s["T"])
    x0, p0, u, mass = poison.hmc_start()
    l0, g0 = fg(x0)
    det = {}
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xn, ln, gn, acc = sampling.hmc_batched_step(fg, x0, l0, g0, mass, s["nleap"], s["eps"], p0, u, details=det)
    pois = det["lnp_new"] == -np.inf
    assert 0.10 <= pois.mean() <= 0.60
    out = {}
    for fused in (True, False):
        h = sampler.BatchedHMC(lp, x0, mass=mass, fused=fused)
        np.testing.assert_allclose(h.lnp.cpu().numpy(), l0, rtol=1e-5)
        lnp_start, x_start = bits(h.lnp).copy(), bits(h.x).copy()
        h.step(s["nleap"], s["eps"], p0=p0, u=u)
        torch.cuda.synchronize()
        got = h.naccept.cpu().numpy().astype(bool)
        print("  fused %s: %d accepted (oracle %d), %d proposals at -inf on the device (oracle %d)" % (
            fused, got.sum(), acc.sum(), int((h.lnp_new == -float("inf")).sum()), pois.sum()))
        assert (got == acc).mean() >= 0.95
        assert not got[pois].any()
        np.testing.assert_array_equal(bits(h.x)[pois], x_start[pois])
        np.testing.assert_array_equal(bits(h.lnp)[pois], lnp_start[pois])
        assert torch.isfinite(h.lnp).all() and torch.isfinite(h.x).all() and torch.isfinite(h.g[:, :7]).all()
        assert np.all(h.lnp_new.cpu().numpy()[pois] == -np.inf) and not torch.isnan(h.lnp_new).any()
        out[fused] = h
    a, b = out[True], out[False]
    for nm in ("x", "lnp", "g", "naccept"):
        np.testing.assert_array_equal(bits(getattr(a, nm)[..., :7] if nm in ("x", "g") else getattr(a, nm)),
                                      bits(getattr(b, nm)[..., :7] if nm in ("x", "g") else getattr(b, nm)), err_msg=nm)


def _stretch_half(ens, it, h, S, Cc, fused):
    """One half step of ``EnsembleSampler.step`` (sampler.py), so that the oracle can be put in lockstep between the halves."""
    st = _lib.stream()
    lib_seed = C.c_uint64(poison.stretch_lib_seed(ens.seed))
    if fused:
        _lib.call("linna_stretch_half_step", ens.lp._ensure()["handle"], _lib.ptr(ens.coords), ens.ld, ens.ndim, _lib.ptr(ens.logp),
                  _lib.iptr(S), ens.half, _lib.ptr(ens.coords), ens.ld, _lib.iptr(Cc), ens.half, lib_seed, _lib.iptr(ens.step_dev), it, h,
                  ens.a, _lib.iptr(ens.naccept), st)
        return
    ens.step_dev.fill_(it)
    _lib.call("linna_stretch_propose", ens.ctx, _lib.ptr(ens.coords), ens.ld, ens.ndim, _lib.iptr(S), ens.half, _lib.ptr(ens.coords),
              ens.ld, _lib.iptr(Cc), ens.half, lib_seed, _lib.iptr(ens.step_dev), h, ens.a, _lib.ptr(ens.Q), ens.ld,
              _lib.ptr(ens.factors), st)
    ens._lnp(ens.Q, ens.lp_new)
    _lib.call("linna_stretch_accept", ens.ctx, _lib.ptr(ens.coords), ens.ld, ens.ndim, _lib.ptr(ens.logp), _lib.iptr(S), ens.half,
              _lib.ptr(ens.Q), ens.ld, _lib.ptr(ens.lp_new), _lib.ptr(ens.factors), lib_seed, _lib.iptr(ens.step_dev), h,
              _lib.iptr(ens.naccept), st)


def test_stretch_move_never_takes_a_rejected_point():
    """Poisoned simple_6_4 at T = 4, 64 walkers just inside theta0 > 0, 4 iterations: the fused half step, the three-launch
    form and linna_stretch_run, with the oracle in lockstep half step by half step.  A walker whose oracle proposal is -inf
    keeps its coordinates and lnP bit for bit (the decision has infinite margin); the three forms are bit-identical."""
    from linna_amd import sampler
    s = poison.STRETCH
    nw, nd = s["nw"], 6
    prob = poison.poisoned_problem(s["name"])
    lp = build_logprob(None, s["T"], prob=prob)[0]
    f = poison.oracle_fn(prob, s["T"])
    x0 = poison.stretch_start()
    a = sampler.EnsembleSampler(nw, nd, lp, seed=s["seed"], randomize_split=False)
    b = sampler.EnsembleSampler(nw, nd, lp, seed=s["seed"], randomize_split=False, fused=False)
    c = sampler.EnsembleSampler(nw, nd, lp, seed=s["seed"], randomize_split=False)
    for e in (a, b, c):
        e.set_state(x0)
    chain, lps = c.run(s["iters"])
    assert c.block_run is True
    halves = np.arange(nw).reshape(2, nw // 2)
    hd = torch.as_tensor(halves.astype(np.int32), device="cuda")
    lib_seed = poison.stretch_lib_seed()
    npois = nsame = nacc = 0
    for it in range(s["iters"]):
        for h in (0, 1):
            S, Cc = halves[h], halves[1 - h]
            before_x, before_l = b.coords[:, :nd].cpu().numpy().copy(), b.logp.cpu().numpy().copy()
            bx, bl = bits(b.coords).copy(), bits(b.logp).copy()
            _stretch_half(a, it, h, hd[h], hd[1 - h], True)
            _stretch_half(b, it, h, hd[h], hd[1 - h], False)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(bits(a.coords), bits(b.coords), err_msg="fused against three launches, iteration %d half %d" % (it, h))
            np.testing.assert_array_equal(bits(a.logp), bits(b.logp))
            assert torch.equal(a.naccept, b.naccept)
            q, new_lp, acc, ox, ol = poison.stretch_half(before_x, before_l, S, Cc, lib_seed, it, h, f)
            pois = new_lp == -np.inf
            npois += int(pois.sum())
            ax, al = bits(b.coords), bits(b.logp)
            np.testing.assert_array_equal(ax[S[pois]], bx[S[pois]], err_msg="a walker moved to a rejected point")
            np.testing.assert_array_equal(al[S[pois]], bl[S[pois]])
            np.testing.assert_array_equal(ax[Cc], bx[Cc])                               # the complementary half stands still
            moved = np.any(ax[S] != bx[S], axis=1)
            same = moved == acc
            nsame += int(same.sum()); nacc += int(moved.sum())
            gx, gl = b.coords[:, :nd].cpu().numpy(), b.logp.cpu().numpy()
            k = S[same]
            assert np.all(np.abs(gx[k] - ox[k]) <= 1e-5 * (1 + np.abs(ox[k])))
            np.testing.assert_allclose(gl[k], ol[k], rtol=8e-6)
            assert np.all(np.isfinite(gl)) and np.all(1.0 + gx[:, 0] > 0)              # no walker ever has theta0 <= 0
        np.testing.assert_array_equal(bits(chain[it]), bits(a.coords[:, :nd]), err_msg="linna_stretch_run, iteration %d" % it)
        np.testing.assert_array_equal(bits(lps[it]), bits(a.logp))
    total = s["iters"] * nw
    print("  stretch: %d of %d proposals -inf in the oracle, %d accepted, %d decisions equal" % (npois, total, nacc, nsame))
    assert npois >= 10
    assert nsame >= 0.97 * total, (nsame, total)
    assert torch.equal(c.naccept, a.naccept) and 0 < nacc < total


def _slice_runs(s, prob, paths):
    """Replay runs of scenario ``s`` over ``paths`` = [(label, engine rows, fusion mask or None, fast)]; returns
    {label: (coords, logp, expansions and contractions)} and checks the tallies the replay keeps."""
    from test_gpu_slice_replay import _run
    out = {}
    prev = _lib.slice_fusion(-1)
    try:
        for label, rows, mask, fast in paths:
            _lib.engine_rows(rows)
            if mask is not None:
                _lib.slice_fusion(mask)
            prepare = (lambda e: e.set_schedule(*poison.SLICE_SCHEDULE)) if fast else (lambda e: None)
            ens, rp, _ = _run(None, s["T"], s["nw"], seed=s["seed"], iters=s["iters"], x_scale=poison.SLICE_XSCALE, prepare=prepare,
                              prob=prob, tune=False, mu=poison.SLICE_MU, fast=fast)
            assert rp.paths == {"one-call" if fast else "rounds"}, (label, rp.paths)
            assert rp.walker_half_steps == s["iters"] * s["nw"]
            assert rp.exempt <= 0.02 * rp.walker_half_steps + 2, (label, rp.exempt)
            assert torch.isfinite(ens.logp).all() and bool((1.0 + ens.coords[:, 0] > 0).all()), label
            out[label] = (bits(ens.coords).copy(), bits(ens.logp).copy(), rp.gpu_counts.copy(), rp.unfinished, rp.ninf)
            print("  %-40s exempt %d of %d, unfinished %d, oracle evaluations at -inf %d" % (
                label, rp.exempt, rp.walker_half_steps, rp.unfinished, rp.ninf))
    finally:
        _lib.engine_rows(0)
        _lib.slice_fusion(prev)
    return out


@pytest.mark.parametrize("k", range(len(poison.SLICE)))
def test_slice_move_never_takes_a_rejected_point(k, monkeypatch):
    """tests/test_gpu_slice_replay.py's lockstep replay (its assertions as they are) on a poisoned problem at mu = 1: the
    round loop, and linna_slice_half_step under fusion masks 0, 1, 3, 7 on the 4- and the 16-row engine.  A comparison
    against a -inf lnP has infinite margin: such walkers are never exempt, so every one of them must agree exactly.  The
    chain is the same under every mask."""
    import test_gpu_slice_replay as R
    s = poison.SLICE[k]
    prob = poison.poisoned_problem(s["name"])

    Base = R.Replay                                            # (bound here: the module's name is replaced below)

    class Counting(Base):                                     # the replay's oracle, with a tally of its -inf evaluations
        def __init__(self, ens, prob_, temperature, seed):
            Base.__init__(self, ens, prob_, temperature, seed)
            inner, self.ninf = self.f, 0

            def f(q):
                with np.errstate(invalid="ignore", divide="ignore"):
                    out = inner(q)
                self.ninf += int(np.sum(out == -np.inf))
                return out
            self.f = f
    monkeypatch.setattr(R, "Replay", Counting)
    paths = [("rounds", 0, None, False)]
    paths += [("one call, engine rows %d, fusion %d" % (rows, m), rows, m, True) for rows in (4, 16) for m in (0, 1, 3, 7)]
    out = _slice_runs(s, prob, paths)
    for label, v in out.items():
        assert v[4] >= 50, (label, v[4])
    for rows in (4, 16):
        base = out["one call, engine rows %d, fusion 0" % rows]
        for m in (1, 3, 7):
            v = out["one call, engine rows %d, fusion %d" % (rows, m)]
            np.testing.assert_array_equal(v[0], base[0], err_msg="engine rows %d, fusion %d" % (rows, m))
            np.testing.assert_array_equal(v[1], base[1])
            assert (v[2] == base[2]).all() and v[3] == base[3]


def test_bf16_slice_masks_give_the_same_chain_through_rejected_points():
    """The one-call half step on a bf16 handle (poisoned simple_6_4, the diagonal of its inverse covariance), 4-row engine:
    the chain and the counts are the same under fusion masks 0, 1, 3, 7, no walker ends on a rejected point, and the
    walkers did meet the edge (trial points with theta0 <= 0 among those the move evaluated)."""
    from linna_amd import sampler
    from test_gpu_bf16 import as_bf16
    s = poison.SLICE[0]
    prob = poison.diagonal(poison.poisoned_problem(s["name"]))
    lp = as_bf16(build_logprob(None, s["T"], prob=prob)[0])
    nw, nd = s["nw"], prob["nin"]
    x0 = poison.slice_start(nw, nd)
    prev = _lib.slice_fusion(-1)
    _lib.engine_rows(4)
    try:
        out = {}
        for mask in (0, 1, 3, 7):
            _lib.slice_fusion(mask)
            a = sampler.SliceEnsembleSampler(nw, nd, lp, seed=s["seed"], tune=False, mu=poison.SLICE_MU, fast=True)
            a.set_schedule(*poison.SLICE_SCHEDULE)
            a.set_state(x0)
            for it in range(s["iters"]):
                a._step()
            torch.cuda.synchronize()
            assert a._fast_ok is True
            assert torch.isfinite(a.logp).all() and bool((1.0 + a.coords[:, 0] > 0).all())
            out[mask] = (bits(a.coords).copy(), bits(a.logp).copy(), a._fast_bufs["counters"][:4].cpu().numpy().copy())
        for mask in (1, 3, 7):
            np.testing.assert_array_equal(out[mask][0], out[0][0], err_msg="fusion %d" % mask)
            np.testing.assert_array_equal(out[mask][1], out[0][1])
            np.testing.assert_array_equal(out[mask][2], out[0][2])
        assert out[0][2][0] > 0 and out[0][2][1] > 0                     # expansions and contractions both happened
    finally:
        _lib.engine_rows(0)
        _lib.slice_fusion(prev)
