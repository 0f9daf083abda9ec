"""GPU: zeus' ensemble slice move fused on the opt-in bf16 serving engine (net_stream_slice_bf16_kernel behind
linna_slice_half_step and linna_logprob_eval_slice_points on a bf16 handle).

The procedures are those of tests/test_gpu_sampling.py's fp32 slice tests, run on a bf16 Log_prob.  Bit-identity is the claim
the fp32 kernels make (same Philox counters, same fp32 arithmetic for the trial point, the same rounding behind it): plain
``torch.equal``, no tolerance, and always on ONE forced engine -- another engine sums in another order, which can move an
operand across a bf16 rounding boundary."""
import ctypes as C

import numpy as np
import pytest

from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from test_gpu_serving import build_logprob  # noqa: E402
from test_gpu_sampling import identity_emulator_logprob, _gaussian_33  # noqa: E402
from test_gpu_bf16 import as_bf16, diag_problem, _posterior_gate  # noqa: E402


def bf16_logprob(name, T=2.0):
    """(fp32 Log_prob, bf16 Log_prob) on golden network `name` with the diagonal of its inverse covariance."""
    lp32 = build_logprob(None, T, diag_problem(name)[0])[0]
    return lp32, as_bf16(lp32)


def test_one_call_path_engages_on_a_bf16_log_prob():
    """A bf16 Log_prob in SliceEnsembleSampler(fast=True): linna_slice_half_step serves it (it returned LINNA_ERR_UNSUPPORTED
    before the bf16 slice evaluation existed, and `_fast_ok` went False)."""
    from linna_amd import sampler
    _, lp = bf16_logprob("v2_33_33")
    nw, nd = 128, 33
    a = sampler.SliceEnsembleSampler(nw, nd, lp, seed=2, tune=False, mu=0.7, fast=True)
    a.set_state((0.3 * np.random.RandomState(1).standard_normal((nw, nd))).astype(np.float32))
    for _ in range(4):
        a.step()
    torch.cuda.synchronize()
    assert a._fast_ok is True, "the one-call half step refused a bf16 handle: %r" % _lib.load().linna_last_error().decode()
    assert a.lp.precision == "bf16" and torch.isfinite(a.logp).all()
    # ... and so does the round loop's evaluation (trial points formed in the prologue), when that route is asked for
    b = sampler.SliceEnsembleSampler(nw, nd, lp, seed=2, tune=False, mu=0.7, fast=False)
    b.set_state((0.3 * np.random.RandomState(1).standard_normal((nw, nd))).astype(np.float32))
    b.step()
    torch.cuda.synchronize()
    assert b.fused_points is True and b._fast_ok is None


@pytest.mark.parametrize("name,nw", [("mlp_33_33", 96), ("v2_33_33", 16), ("mlp_33_33", 1024)])
def test_bf16_one_call_slice_half_step_equals_the_round_loop(name, nw):
    """test_one_call_slice_half_step_equals_the_round_loop's procedure on a bf16 handle: 12 iterations, coordinates, lnP,
    expansion and contraction counts equal, no unfinished walker; then the overflow case (mu = 0.05, one stepping-out end)
    ending on the round loop's chain."""
    from linna_amd import sampler
    _, lp = bf16_logprob(name)
    nd = 33
    x0 = (0.3 * np.random.RandomState(8).standard_normal((nw, nd))).astype(np.float32)
    _lib.engine_rows(4)                                     # one engine for every batch size: bit-equal evaluations
    try:
        a = sampler.SliceEnsembleSampler(nw, nd, lp, seed=4, tune=False, mu=0.7, fast=True)
        b = sampler.SliceEnsembleSampler(nw, nd, lp, seed=4, tune=False, mu=0.7, fast=False)
        a.set_state(x0); b.set_state(x0)
        for it in range(12):
            a.step(); b.step()
            torch.cuda.synchronize()
            assert torch.equal(a.coords, b.coords) and torch.equal(a.logp, b.logp), it
            ca = a._fast_bufs["counters"].cpu().numpy()
            cb = b.counters.cpu().numpy()
            assert ca[0] == cb[0] and ca[1] == cb[1] and ca[2] == 0, (it, ca[:4], cb)      # expansions, contractions, none unfinished
        assert a._fast_ok is True and a.iteration == b.iteration == 12
        assert a.neval > 0 and b.neval > 0
        assert not torch.equal(a.coords[:, :nd], torch.as_tensor(x0, device=a.coords.device))     # the walkers did move
        c = sampler.SliceEnsembleSampler(nw, nd, lp, seed=4, tune=False, mu=0.05, fast=True)
        d = sampler.SliceEnsembleSampler(nw, nd, lp, seed=4, tune=False, mu=0.05, fast=False)
        c.set_schedule([1], c.nt_sched)
        c.set_state(x0); d.set_state(x0)
        cc, cl = c.run(3)
        dc, dl = d.run(3)
        assert c.noverflow == 1 and d.noverflow == 0
        assert torch.equal(cc, dc) and torch.equal(cl, dl) and torch.equal(c.coords, d.coords) and c.iteration == d.iteration == 3
        assert int(c.step_dev.item()) == int(d.step_dev.item())
    finally:
        _lib.engine_rows(0)


@pytest.mark.parametrize("rows", [4, 8, 16])
def test_bf16_slice_fusion_masks_give_the_same_chain(rows):
    """test_slice_fusion_masks_give_the_same_chain's procedure on a bf16 handle: masks 0, 1, 3, 7 (the plain weights, the
    derived trial points of bit 0, the set-up fused by bit 1) on each engine, three (walkers, schedule) pairs -- chains and
    counts equal to mask 0."""
    from linna_amd import sampler
    _, lp = bf16_logprob("mlp_33_33")
    nd = 33
    prev = _lib.slice_fusion(-1)
    _lib.engine_rows(rows)
    try:
        for nw, sched in [(128, ([8], [16, 16])), (44, ([5], [9])), (600, ([2], [4, 8]))]:
            x0 = (0.3 * np.random.RandomState(nw).standard_normal((nw, nd))).astype(np.float32)
            out = {}
            for mask in (0, 1, 3, 7):
                _lib.slice_fusion(mask)
                a = sampler.SliceEnsembleSampler(nw, nd, lp, seed=21, tune=False, mu=0.8, fast=True)
                a.set_schedule(*sched)
                a.set_state(x0)
                for it in range(7):
                    a._step()                              # (no guard: an unfinished walker is part of the comparison)
                torch.cuda.synchronize()
                assert a._fast_ok is True
                out[mask] = (a.coords.clone(), a.logp.clone(), a._fast_bufs["counters"][:4].cpu().numpy(), int(a.step_dev.item()))
            for mask in (1, 3, 7):
                assert torch.equal(out[mask][0], out[0][0]) and torch.equal(out[mask][1], out[0][1]), (nw, mask)
                assert (out[mask][2] == out[0][2]).all() and out[mask][3] == out[0][3], (nw, mask, out[mask][2], out[0][2])
    finally:
        _lib.engine_rows(0)
        _lib.slice_fusion(prev)


def _trial_setup(lp, nw, nd, nrep, seed):
    """Device buffers of one evaluation of trial points: coords [nw, ld], a half ensemble S, directions DIR [ns, ld], weights
    w [nrep ns] (row j ns + k is coords[S[k]] + w[j ns + k] DIR[k])."""
    p = lp._ensure()
    dev, ld, ns = p["dev"], _lib.ld4(nd), nw // 2
    rs = np.random.RandomState(seed)
    t = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    coords = torch.zeros((nw, ld), device=dev); coords[:, :nd] = t(0.3 * rs.standard_normal((nw, nd)))
    DIR = torch.zeros((ns, ld), device=dev); DIR[:, :nd] = t(0.2 * rs.standard_normal((ns, nd)))
    S = t(rs.permutation(nw)[:ns], torch.int32)
    w = t(rs.uniform(-2.0, 2.0, nrep * ns))
    return dict(dev=dev, ld=ld, ns=ns, nd=nd, nrep=nrep, coords=coords, DIR=DIR, S=S, w=w)


def _fused_points(lp, s):
    """linna_logprob_eval_slice_points: lnP [nrep ns] of the trial points, which are never written."""
    Z = torch.full((s["nrep"] * s["ns"],), float("nan"), device=s["dev"])
    rc = _lib.load().linna_logprob_eval_slice_points(lp._ensure()["handle"], _lib.ptr(s["coords"]), s["ld"], s["nd"], _lib.iptr(s["S"]),
                                                     s["ns"], _lib.ptr(s["DIR"]), s["ld"], _lib.ptr(s["w"]), s["nrep"], _lib.ptr(Z), None,
                                                     _lib.stream())
    assert rc == 0, "linna_logprob_eval_slice_points: %d %r" % (rc, _lib.load().linna_last_error().decode())
    torch.cuda.synchronize()
    return Z


def _materialised_points(lp, s):
    """linna_slice_points, then linna_logprob_eval_if on the points it wrote: (points [nrep ns, ld], lnP)."""
    B = s["nrep"] * s["ns"]
    Q = torch.zeros((B, s["ld"]), device=s["dev"])
    Z = torch.full((B,), float("nan"), device=s["dev"])
    _lib.call("linna_slice_points", _lib.ctx(s["dev"].index), _lib.ptr(s["coords"]), s["ld"], s["nd"], _lib.iptr(s["S"]), s["ns"],
              _lib.ptr(s["DIR"]), s["ld"], _lib.ptr(s["w"]), _lib.ptr(Q), s["ld"], s["nrep"], _lib.stream())
    _lib.call("linna_logprob_eval_if", lp._ensure()["handle"], _lib.ptr(Q), Q.stride(0), B, _lib.ptr(lp._workspace(B, False)),
              _lib.ptr(Z), None, 0, None, _lib.stream())
    torch.cuda.synchronize()
    return Q, Z


@pytest.mark.parametrize("rows", [4, 8, 16])
@pytest.mark.parametrize("name", ["v2_33_33", "mlp_33_33"])
def test_bf16_eval_slice_points_equals_materialised_points(name, rows):
    """linna_logprob_eval_slice_points on a bf16 handle against linna_slice_points + a bf16 linna_logprob_eval_if on the
    materialised points, bit for bit on a forced engine, ragged launches included (137 and 2 x 1031 points: not a multiple of
    any engine's rows).  The C entry takes no row list -- the list and its device-side count exist inside
    linna_slice_half_step only -- so the row-list launches are compared where they occur: a schedule of several rounds under
    fusion mask 0 (every launch behind the first of each kind evaluates listed rows only, with plain weights), against the
    round loop, which materialises every point."""
    from linna_amd import sampler
    _, lp = bf16_logprob(name)
    prev_mask = _lib.slice_fusion(-1)
    _lib.engine_rows(rows)
    try:
        for nw, nrep in ((274, 1), (2062, 2), (64, 5)):
            s = _trial_setup(lp, nw, 33, nrep, 100 + nw)
            got = _fused_points(lp, s)
            _, ref = _materialised_points(lp, s)
            assert torch.isfinite(ref).all()
            assert torch.equal(got, ref), "%s rows=%d nw=%d nrep=%d: %d of %d lnP differ (max %.3e)" % (
                name, rows, nw, nrep, int((got != ref).sum()), got.numel(), float((got - ref).abs().max()))
        # with a row list: later rounds of the one-call half step, nothing else fused
        _lib.slice_fusion(0)
        nw, m_sched, nt_sched = 250, [1, 2, 4, 8], [2, 4, 8, 16, 32]
        x0 = (0.3 * np.random.RandomState(nw).standard_normal((nw, 33))).astype(np.float32)
        a = sampler.SliceEnsembleSampler(nw, 33, lp, seed=9, tune=False, mu=0.9, fast=True)
        b = sampler.SliceEnsembleSampler(nw, 33, lp, seed=9, tune=False, mu=0.9, fast=False)
        a.set_schedule(m_sched, nt_sched)
        a.set_state(x0); b.set_state(x0)
        for it in range(6):
            a.step(); b.step()
            torch.cuda.synchronize()
            assert torch.equal(a.coords, b.coords) and torch.equal(a.logp, b.logp), (name, rows, it)
            if a.noverflow:                              # (a walker left unfinished: the guarded step redid the iteration on the
                break                                    #  round loop and deepened the schedule -- new buffers)
            ca, cb = a._fast_bufs["counters"].cpu().numpy(), b.counters.cpu().numpy()
            assert ca[0] == cb[0] and ca[1] == cb[1], (it, ca[:4], cb)
        assert a._fast_ok is True
        if not a.noverflow:
            use = a.round_usage()
            assert use["active_after_expand_round"][0] > 0 and use["active_after_shrink_round"][0] > 0, use   # listed rows were evaluated
    finally:
        _lib.engine_rows(0)
        _lib.slice_fusion(prev_mask)


@pytest.mark.parametrize("rows", [4, 8, 16])
def test_fused_slice_points_are_bf16_and_not_fp32(rows):
    """The lnP the fused launch returns on a bf16 handle are the bf16 Log_prob.evaluate of the same (materialised) points on
    the same engine, bit for bit, and differ from what the fp32 handle's fused launch returns for them."""
    lp32, lp = bf16_logprob("v2_33_33")
    _lib.engine_rows(rows)
    try:
        s = _trial_setup(lp, 512, 33, 2, 7)
        got = _fused_points(lp, s)
        Q, _ = _materialised_points(lp, s)
        ref = lp.evaluate(Q).clone()
        ref32 = lp32.evaluate(Q).clone()
        got32 = _fused_points(lp32, s)
        torch.cuda.synchronize()
        assert torch.equal(got, ref), "fused bf16 slice points are not the bf16 evaluation of those points (max %.3e)" % float((got - ref).abs().max())
        assert torch.equal(got32, ref32)
        assert not torch.equal(got, got32), "the bf16 handle's slice launch returned the fp32 values"
    finally:
        _lib.engine_rows(0)


def test_bf16_slice_posterior_33d_gaussian_on_the_one_call_path(capsys):
    """test_posterior_33d_gaussian_emcee_and_slice's slice half: the 33-D Gaussian through a bf16 Log_prob, mu tuned, the
    tuned iterations on linna_slice_half_step; same gates (mean within 0.05 sigma, standard deviation within 6 %), and the
    stored lnP are the bf16 lnP of the stored positions within that test's 1e-4 (1 + |lnP|)."""
    from linna_amd import sampler, util
    ndim, means, cov, priors = _gaussian_33()
    lp = as_bf16(identity_emulator_logprob(ndim, means, cov, priors))
    nw = 512
    sl = sampler.SliceEnsembleSampler(nw, ndim, lp, seed=5)
    z0 = util.invTransform(priors)(means)[None, :] + 0.001 * np.random.RandomState(1).standard_normal((nw, ndim))
    sl.set_state(z0)
    sl.run(300, store=False)
    assert not sl.tune and 0.05 < sl.mu < 50.0
    c, l = sl.run(500)
    assert sl._fast_ok is True, "the bf16 slice driver did not run on the one-call path"
    assert getattr(sl, "_fast_steps", 0) >= 500, "one-call iterations: %d" % getattr(sl, "_fast_steps", 0)
    _posterior_gate(sl.theta_of(c).cpu().numpy().reshape(-1, ndim), means, cov, "slice bf16, one call per half step")
    again = lp.evaluate(torch.nn.functional.pad(c[-1], (0, sl.ld - ndim))).cpu().numpy().astype(np.float64)
    stored = l[-1].cpu().numpy().astype(np.float64)
    worst = np.max(np.abs(again - stored) / (1e-4 * (1 + np.abs(stored))))
    with capsys.disabled():
        print("\n  bf16 slice posterior: mu %.3f, one-call iterations %d, overflows %d, max |stored - fresh lnP| = %.3e (%.3g of 1e-4 (1 + |lnP|))" % (
            sl.mu, sl._fast_steps, sl.noverflow, np.max(np.abs(again - stored)), worst))
    assert worst <= 1.0, "slice chain lnP are not the bf16 lnP of the stored positions: %.3g of 1e-4 (1 + |lnP|)" % worst


def test_ml_sampler_core_zeus_bf16_end_to_end(tmp_path, monkeypatch, capsys):
    """test_ml_sampler_core_bf16_end_to_end's 2-D problem with the reference's default sampler: method="zeus" through a bf16
    emulator completes with a finite chain inside the priors.  (4 walkers, mu still being tuned: the driver may stay on the
    round loop -- how often the one-call path engaged is printed, not asserted.)"""
    from linna_amd import sampler
    from linna_amd.main import ml_sampler_core
    from linna_amd.nn import ChtoModelv2
    from copy import deepcopy
    calls = []
    inner = sampler.SliceEnsembleSampler._step_fast

    def recording(self, halves, seed):
        r = inner(self, halves, seed)
        calls.append((bool(r), getattr(self.lp, "precision", None)))
        return r

    monkeypatch.setattr(sampler.SliceEnsembleSampler, "_step_fast", recording)
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
                                     nnmodel_in=ChtoModelv2, params=params, method="zeus", emulator_precision="bf16")
    with capsys.disabled():
        print("\n  zeus through bf16: %d one-call attempts, %d engaged, precisions %s" % (
            len(calls), sum(1 for ok, _ in calls if ok), sorted(set(str(p) for _, p in calls))))
    assert chain.ndim == 2 and chain.shape[1] == ndim and len(chain) > 0
    assert np.all(np.isfinite(chain)) and np.all(np.abs(chain) <= 2.0)
    assert all(p == "bf16" for _, p in calls)
