"""GPU: the trajectory-length adaptation of ``method="hmc"`` (ChEES) -- linna_hmc_chees_begin / linna_hmc_chees_end against the
float64 emulation (tests/hmc_chees_emul.py), ``run()`` in trajectory mode against the loop of ``run(1, L_i)`` bit for bit,
``BatchedHMC.adapt_traj`` on the Gaussian the host test runs the emulation on, and the keyword through the drivers with its
sidecar file."""
import math
import os

import numpy as np
import pytest

import hmc_adapt_emul as emul
import hmc_chees_emul as chees
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from test_gpu_sampling import identity_emulator_logprob  # noqa: E402
from test_gpu_hmc_adapt import chains, assert_same_state, ND  # noqa: E402
from test_gpu_hmc_dense import _dense_chains  # noqa: E402

U53 = 2.0 ** -53
GUARD = -7.5
NG = 8


def _padded(a, fill=float("nan")):
    B, nd = a.shape
    X = torch.full((B, _lib.ld4(nd)), fill, device="cuda")
    X[:, :nd].copy_(torch.as_tensor(np.ascontiguousarray(a, np.float32)))
    return X


def _guarded(values, dtype):
    t = torch.full((len(values) + NG,), GUARD, dtype=dtype, device="cuda")
    t[:len(values)].copy_(torch.as_tensor(np.asarray(values), dtype=dtype))
    return t


def _inputs(B, nd, k, rs, dense, none_valid):
    """Transition k's positions, proposal, momenta and acceptance probabilities: the cloud expands (the criterion has a clear
    sign, so that g is not a rounding residue), with one NaN proposal, one alpha = 0 and one infinite momentum for B > 3."""
    scale = np.geomspace(1e-2, 1.0, nd)
    x = (0.3 * k + scale * rs.standard_normal((B, nd))).astype(np.float32)
    q = (x + 0.5 * (x - x.mean(0)) + 0.05 * scale * rs.standard_normal((B, nd))).astype(np.float32)
    mass = np.linspace(0.5, 2.0, nd).astype(np.float32)
    p = ((q - q.mean(0)) * (1.0 if dense else mass) * (1.0 + 0.3 * rs.standard_normal((B, nd)))).astype(np.float32)
    alpha = rs.uniform(0.05, 1.0, B).astype(np.float32)
    alpha[rs.uniform(size=B) < 0.2] = 1.0
    kinds = (0, 1, 2) if B > 3 else ((k % 3,) if B == 3 else ())          # (three chains: one kind a transition)
    if 0 in kinds:
        q[k % B, (3 * k) % nd] = np.nan
    if 1 in kinds:
        alpha[(k + 1) % B] = 0.0
    if 2 in kinds:
        p[(k + 2) % B, (5 * k + 1) % nd] = np.inf if k % 2 else -np.inf
    if none_valid:
        alpha[:] = 0.0
    return x, q, p, alpha, mass, len(kinds)


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) / np.maximum(np.abs(b), 1e-300)


@pytest.mark.parametrize("B,nd,dense", [(1, 1, False), (3, 7, False), (67, 33, False), (256, 65, False), (4096, 33, False), (33, 33, True)],
                         ids=["1x1", "3x7", "67x33", "256x65", "4096x33", "33x33-dense"])
def test_begin_and_end_against_the_emulation(B, nd, dense):
    """14 successive transitions with M = 10 (across the freeze), transition 6 without a valid chain; NaN in the pad columns,
    guard words behind every output.  m0, m1 and r0 within 64 B 2^-53 relative (the worst-case error of a float64 sum of B
    terms is (B - 1) 2^-53 of the sum of magnitudes; the means on the scale |mean| + std, as tests/test_gpu_hmc_mass.py
    argues; every term of r0 is positive), g within 64 B ndim 2^-53 of sum alpha |c| / sum alpha (what it cancels from), the
    state words within 1e-12 relative of the emulation's own sequence, eps[b] within 1 ulp of its float32 rounding.  The
    same input twice gives identical bits."""
    ld, M, delta, maxL, eps0, ntr = _lib.ld4(nd), 10, 0.65, 64, 0.05, 14
    n = int(_lib.load().linna_hmc_chees_doubles(nd))
    assert n == chees.HEAD + 2 * nd
    Cl = cm = None
    if dense:
        Cl = np.tril(np.random.RandomState(nd).standard_normal((nd, nd)) / np.sqrt(nd)).astype(np.float32)
        Cl[np.diag_indices(nd)] = np.abs(np.diag(Cl)) + 0.5
        pair = np.full((2, nd, ld), np.nan, np.float32)
        pair[0, :, :nd], pair[1, :, :nd] = Cl, Cl.T
        cm = torch.as_tensor(pair, device="cuda")
    tol = 64.0 * B * U53
    runs = []
    for rep in range(2):
        rs = np.random.RandomState(1000 * B + nd)
        ref = chees.new_state(eps0)
        state = _guarded(chees.pack(ref, np.zeros(nd), np.zeros(nd)), torch.float64)
        r0d = _guarded(np.zeros(B), torch.float64)
        epsd = _guarded(np.zeros(B), torch.float32)
        worst = dict(m0=0.0, r0=0.0, m1=0.0, g=0.0, state=0.0)
        last = state.cpu().numpy()
        for k in range(1, ntr + 1):
            none_valid = k == 6
            x, q, p, alpha, mass, ninvalid = _inputs(B, nd, k, rs, dense, none_valid)
            X, Q, P = _padded(x), _padded(q), _padded(p)
            al = torch.as_tensor(alpha, device="cuda")
            ms = torch.as_tensor(np.ones(nd, np.float32) if dense else mass, device="cuda")
            _lib.call("linna_hmc_chees_begin", _lib.ctx(), B, nd, _lib.ptr(X), ld, _lib.ptr(state, torch.float64),
                      _lib.ptr(r0d, torch.float64), _lib.stream())
            _lib.call("linna_hmc_chees_end", _lib.ctx(), B, nd, _lib.ptr(ms), _lib.ptr(cm) if dense else None, ld if dense else 0,
                      _lib.ptr(Q), ld, _lib.ptr(P), ld, _lib.ptr(al), _lib.ptr(r0d, torch.float64), _lib.ptr(state, torch.float64),
                      _lib.ptr(epsd), M, delta, maxL, _lib.stream())
            torch.cuda.synchronize()
            if rep:
                continue
            got, r0g, eg = state.cpu().numpy(), r0d.cpu().numpy(), epsd.cpu().numpy()
            assert np.all(got[n:] == GUARD) and np.all(r0g[B:] == GUARD) and np.all(eg[B:] == GUARD), k
            m0, r0 = chees.begin(x)
            out = chees.end(ref, q, p, alpha, r0, M, delta, maxL, mass=None if dense else mass, chol=Cl)
            x64 = x.astype(np.float64)
            worst["m0"] = max(worst["m0"], float(np.max(np.abs(got[12:12 + nd] - m0) / (np.abs(m0) + x64.std(0) + (B == 1)))))
            worst["r0"] = max(worst["r0"], float(np.max(np.abs(r0g[:B] - r0) / np.where(r0 > 0, r0, 1.0))))
            nvalid = int(out["valid"].sum())
            assert got[11] == nvalid == (0 if none_valid else B - ninvalid) and got[0] == k + 1.0, (k, nvalid)
            if nvalid:
                qv = q[out["valid"]].astype(np.float64)
                worst["m1"] = max(worst["m1"], float(np.max(np.abs(got[12 + nd:12 + 2 * nd] - out["m1"]) / (np.abs(out["m1"]) + qv.std(0) + (nvalid == 1)))))
                worst["g"] = max(worst["g"], abs(got[9] - ref["g"]) / (out["gscale"] if out["gscale"] > 0 else 1.0))
            else:
                # without a valid chain Adam's moments, the average of log T and the last g keep their bits, log T is only
                # clamped, and the step size moves on with hm = the floor
                assert np.array_equal(got[[2, 3, 4, 9]].view(np.int64), last[[2, 3, 4, 9]].view(np.int64)), k
                assert got[10] == pytest.approx(1e-3, rel=1e-12) and got[7] != last[7]
                assert got[1] == pytest.approx(min(max(last[1], got[7]), got[7] + math.log(maxL)), rel=1e-15)
            want = np.array([ref[w] for w in chees.WORDS])
            worst["state"] = max(worst["state"], float(_rel(got[:12], want).max()))
            ulp = np.abs(eg[:B].view(np.int32).astype(np.int64) - np.int64(np.float32(out["eps"]).view(np.int32)))
            assert ulp.max() <= 1 and np.all(eg[:B] == eg[0]), (k, ulp.max())
            if k == M:
                assert eg[0] == pytest.approx(math.exp(ref["logepsbar"]), rel=1e-6) and got[1] == got[2]      # the freeze
            last = got
        if not rep:
            print("  B %d ndim %d%s: worst errors m0 %.3g r0 %.3g m1 %.3g (bound %.3g), g %.3g (bound %.3g), state %.3g (bound 1e-12)"
                  % (B, nd, " dense" if dense else "", worst["m0"], worst["r0"], worst["m1"], tol, worst["g"], tol * nd, worst["state"]))
            assert worst["m0"] <= tol and worst["r0"] <= tol and worst["m1"] <= tol, worst
            assert worst["g"] <= tol * nd, worst
            assert worst["state"] <= 1e-12, worst
        runs.append((state.cpu().numpy(), r0d.cpu().numpy(), epsd.cpu().numpy()))
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.int64 if a.dtype == np.float64 else np.int32), b.view(np.int64 if b.dtype == np.float64 else np.int32))


def test_dense_velocity_is_refused_beyond_its_limit():
    lib = _lib.load()
    t = torch.zeros(8, device="cuda")
    d = torch.zeros(8, dtype=torch.float64, device="cuda")
    rc = lib.linna_hmc_chees_end(_lib.ctx(), 1, 129, None, _lib.ptr(t), 132, _lib.ptr(t), 132, _lib.ptr(t), 132, _lib.ptr(t),
                                 _lib.ptr(d, torch.float64), _lib.ptr(d, torch.float64), _lib.ptr(t), 10, 0.65, 64, None)
    assert rc == _lib.ERR_UNSUPPORTED and b"hmc_chees_end" in lib.linna_last_error()


def _make(kind, name, B, bf):
    return _dense_chains(name, B, bf)[0] if kind == "densemass" else chains(name, B, bf)


@pytest.mark.parametrize("kind,name,B,bf", [("diag", "mlp_33_33", 64, False), ("diag", "v2_33_33", 5, False), ("diag", "mlp_33_33", 70, True),
                                            ("diag", "mlp_33_33_dense", 33, False), ("densemass", "mlp_33_33", 33, False)],
                         ids=["mlp-64", "v2-5", "mlp-70-bf16", "dense-33", "densemass-33"])
def test_run_by_trajectory_length_equals_the_loop(kind, name, B, bf):
    """``run(7)`` with a trajectory length in place: bit for bit the loop of ``run(1, L_i)``, L_i = the emulation's
    ``steps_for``; an explicit ``num_steps`` is not affected; an object without a length runs ``self.num_steps`` as before."""
    e, T, maxL, n = 2e-2, 0.11, 5, 7
    a, b = _make(kind, name, B, bf), _make(kind, name, B, bf)
    for h in (a, b):
        h.eps.fill_(e)
        h.run(2, 3, store=False)                      # (the sequence does not start at Philox step 0)
    a.set_traj(T, maxL)
    assert a.traj == T and a.max_steps == maxL and a._traj_eps == float(np.float32(e))
    want = [chees.steps_for(i, T, float(np.float32(e)), maxL) for i in range(2, 2 + n)]
    assert want == [a.steps_for(i) for i in range(2, 2 + n)] and len(set(want)) >= 3 and max(want) == maxL
    used = []
    enqueue = a._enqueue
    a._enqueue = lambda ntrans, num_steps, *rest: (used.append((ntrans, num_steps)), enqueue(ntrans, num_steps, *rest))[1]
    ca, la = a.run(n)
    assert used == [(1, L) for L in want]
    rows = [b.run(1, num_steps=L) for L in want]
    torch.cuda.synchronize()
    assert torch.equal(ca, torch.cat([r[0] for r in rows])) and torch.equal(la, torch.cat([r[1] for r in rows]))
    assert_same_state(a, b, "trajectory mode")
    assert a.iteration == b.iteration == 2 + n and torch.equal(a.eps, b.eps) and torch.equal(a.m, b.m)
    assert 0 < int(a.naccept.sum())
    # an explicit num_steps means what it did; without a length run() is the parent's
    c4, l4 = a.run(3, num_steps=4)
    d4, m4 = b.run(3, num_steps=4)
    assert used[-1] == (3, 4) and torch.equal(c4, d4) and torch.equal(l4, m4)
    c, d = _make(kind, name, B, bf), _make(kind, name, B, bf)
    for h in (c, d):
        h.eps.fill_(e)
    assert c.traj is None and c.chees is None and c.num_steps == 5
    cc, lc = c.run(3)
    cd, ld_ = d.run(3, num_steps=5)
    torch.cuda.synchronize()
    assert torch.equal(cc, cd) and torch.equal(lc, ld_)
    assert_same_state(c, d, "no trajectory length")
    a.set_traj(None)
    ce, _ = a.run(2)
    cf, _ = b.run(2, num_steps=5)
    assert torch.equal(ce, cf)


_T = {}


def target():
    """8 parameters with Gaussian priors N(0, 1) (theta = z) behind the identity-exact emulator, the likelihood widths chosen so
    that the posterior in z is the host test's Gaussian: widths geomspace(0.02, 0.6, 8) about linspace(-0.2, 0.2, 8)."""
    if not _T:
        nd, W, mz = len(chees.WIDTHS), chees.WIDTHS, chees.MEAN
        sig = W / np.sqrt(1.0 - W ** 2)
        means = mz * (1.0 + sig ** 2)
        priors = [{"param": "p%d" % i, "dist": "gauss", "arg1": 0.0, "arg2": 1.0} for i in range(nd)]
        _T.update(nd=nd, priors=priors, fg32=emul.gaussian_fg(mz.astype(np.float32), W.astype(np.float32), np.float32),
                  lp=identity_emulator_logprob(nd, means, np.diag(sig ** 2), priors))
    return _T


def test_adapt_traj_against_the_emulation():
    """256 chains from the mode, M = 300, then 300 stored transitions, at unit mass.  The device meets the conditions the
    float64 emulation met in tests/test_hmc_chees_host.py (std within 5 %, acceptance above 0.4, lag-1 autocorrelation of the
    widest parameter below that of 5 fixed steps at the same step size by the recorded margin, traj / the largest width in
    the recorded band); its acceptance over the stored transitions is within 4 standard errors of the float32 emulation's.

    The emulation runs those transitions from the device's own state after the warm-up, with the step size and the length
    the device froze.  All chains share these two numbers, so between two realisations of the warm-up -- the device's and an
    emulation's of it, which part ways after a few dozen transitions as any two arithmetics do -- the acceptance of all
    chains moves together: the float64 emulation froze step sizes 0.0255 ... 0.0263 over its five seeds with acceptances
    0.866 ... 0.877, the float32 one 0.0261 ... 0.0269 with 0.860 ... 0.872, the device 0.02549 with 0.8784, while the
    standard error over 256 chains is 0.0012.  Given the two numbers the chains are independent, and that standard error is
    the one that applies."""
    from linna_amd import sampler
    t = target()
    B, seed, M, N = 256, 1, 300, 300
    z0 = chees.start(B, seed)
    out = []
    for fixed in (None, 5):
        h = sampler.BatchedHMC(t["lp"], z0, seed=seed)
        Ls = []
        enqueue = h._enqueue
        h._enqueue = lambda ntrans, num_steps, *rest: (Ls.append(num_steps), enqueue(ntrans, num_steps, *rest))[1]
        traj, eps = h.adapt_traj(M, 0.65)
        assert h.iteration == M and len(Ls) == M and Ls[0] == 1 and 1 <= min(Ls) and max(Ls) <= 64
        assert traj == h.traj and bool((h.eps == np.float32(eps)).all()) and torch.equal(h.eps, h.epsbar)
        st = h.chees[:12].cpu().numpy()
        assert st[0] == M + 1.0 and st[1] == st[2] and traj == math.exp(st[1])
        n0 = h.naccept.clone()
        after_warmup = h.x[:, :t["nd"]].cpu().numpy()
        chain, _ = h.run(N, num_steps=fixed)
        torch.cuda.synchronize()
        if fixed is None:
            assert Ls[M:] == [chees.steps_for(i, traj, eps) for i in range(M, M + N)]
            print("  device: step size %.4g, mean leapfrog steps %.1f in the warm-up, %.1f afterwards" % (eps, np.mean(Ls[:M]), np.mean(Ls[M:])))
            cur = dict(x=after_warmup, step=M)
            cur["lnp"], cur["g"] = (np.asarray(a, np.float32) for a in t["fg32"](cur["x"]))
            ref = chees.sample(t["fg32"], cur, seed, N, eps, lambda i: chees.steps_for(i, traj, eps), dtype=np.float32)
        out.append((traj, (h.naccept - n0).cpu().numpy() / float(N), chain.cpu().numpy()))
    assert out[0][0] == out[1][0]                                          # (the same warm-up twice: the same bits)
    chees.conditions("device", out[0][0], out[0][1], out[0][2], out[1][2])
    acc, racc = out[0][1], ref[1] / float(N)
    se = float(acc.std(ddof=1) / np.sqrt(B))
    print("  acceptance: device %.4f, float32 emulation %.4f, standard error %.4f" % (acc.mean(), racc.mean(), se))
    assert abs(acc.mean() - racc.mean()) <= 4 * se, (acc.mean(), racc.mean(), se)


def test_adapt_traj_behind_the_mass_adaptation():
    """``adapt(300, adapt_mass=True, adapt_traj=True)`` on tests/test_gpu_hmc_mass.py's widths 0.003 ... 0.3: the mass is that
    test's (mass * var within [0.8, 1.25]), the stored chain's std within 5 %; the mean number of steps is printed."""
    from linna_amd import sampler
    from test_gpu_hmc_mass import target as mass_target, start as mass_start
    t = mass_target()
    B, M, N = 256, 300, 300
    h = sampler.BatchedHMC(t["lp"], mass_start(B), seed=9)
    Ls = []
    enqueue = h._enqueue
    h._enqueue = lambda ntrans, num_steps, *rest: (Ls.append((ntrans, num_steps)), enqueue(ntrans, num_steps, *rest))[1]
    assert h.adapt(M, 0.65, adapt_mass=True, adapt_traj=True) == [(75, 100), (100, 150), (150, 250)]
    assert h.iteration == 2 * M + 1 and h.traj is not None
    n0, first = h.naccept.clone(), len(Ls)
    chain, _ = h.run(N)
    torch.cuda.synchronize()
    prod = h.mass.cpu().numpy().astype(np.float64) * t["sz"] ** 2
    std = chain.cpu().numpy().reshape(-1, t["nd"]).astype(np.float64).std(0) / t["sz"]
    acc = (h.naccept - n0).cpu().numpy() / float(N)
    print("  mass * var %.3f ... %.3f, std / truth %.3f ... %.3f, acceptance %.4f, traj %.4g, step size %.4g, mean leapfrog steps %.1f"
          % (prod.min(), prod.max(), std.min(), std.max(), acc.mean(), h.traj, h._traj_eps, np.mean([L for _, L in Ls[first:]])))
    assert np.all((prod >= 0.8) & (prod <= 1.25)), prod
    assert np.all(np.abs(std - 1.0) <= 0.05), std
    assert acc.mean() > 0.4


def test_through_the_driver(tmp_path, monkeypatch):
    from linna_amd import sampler, util
    t = target()
    nd, nw = t["nd"], 128
    tr = util.Transform(t["priors"])
    z0 = chees.start(nw, 3)
    out = str(tmp_path)
    side, name = os.path.join(out, "chhmc_adapt.npz"), os.path.join(out, "chhmc.h5")
    calls = []
    enqueue = sampler.BatchedHMC._enqueue

    def spy(self, ntrans, num_steps, chain, *rest):
        if chain is not None:
            calls.append((self.iteration, ntrans, num_steps))
        return enqueue(self, ntrans, num_steps, chain, *rest)
    monkeypatch.setattr(sampler.BatchedHMC, "_enqueue", spy)
    s = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, transform=tr, seed=5)
    prof = {}
    s.sample(None, 300, samp_steps=3, samp_eps=0, Madapt=150, outdir=out, method="hmc", profile=prof, adapt_traj=True, max_steps=32)
    assert os.path.isfile(name) and os.path.isfile(side) and prof["host_adapt_s"] > 0
    d = sampler.ChainStore.load(name)
    n1 = len(d["chain"])
    with np.load(side) as f:
        kept = {k: np.array(f[k]) for k in f.files}
    assert {"mass", "eps", "num_steps", "Madapt", "traj", "max_steps", "iteration"} <= set(kept)
    traj, eps, it0 = float(kept["traj"]), float(kept["eps"][0]), int(kept["iteration"])
    assert np.isfinite(traj) and traj > 0 and int(kept["max_steps"]) == 32 and it0 == 2 * 150 + 1 and np.all(kept["eps"] == kept["eps"][0])
    assert calls and all(c == (it0 + k, 1, chees.steps_for(it0 + k, traj, eps, 32)) for k, c in enumerate(calls))
    th = np.asarray(d["chain_transformed"], np.float64).reshape(-1, nd)
    print("  %d iterations stored, traj %.4g, step size %.4g, mean leapfrog steps %.1f, std ratio %.3f ... %.3f"
          % (n1, traj, eps, np.mean([c[2] for c in calls]), (th.std(0) / chees.WIDTHS).min(), (th.std(0) / chees.WIDTHS).max()))
    np.testing.assert_allclose(th.std(0), chees.WIDTHS, rtol=0.08)
    # a second call resumes: no warm-up, the file stays, the sequence of steps goes on where the stored chain ends
    del calls[:]
    s2 = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, transform=tr, seed=6)
    prof2 = {}
    s2.sample(None, n1 + 100, samp_eps=0, Madapt=150, outdir=out, method="hmc", profile=prof2, adapt_traj=True, max_steps=32)
    assert "host_adapt_s" not in prof2 and len(sampler.ChainStore.load(name)["chain"]) > n1
    assert calls and all(c == (it0 + n1 + k, 1, chees.steps_for(it0 + n1 + k, traj, eps, 32)) for k, c in enumerate(calls))
    with np.load(side) as f:
        assert float(f["traj"]) == traj and np.array_equal(f["eps"], kept["eps"])
    # a file without a trajectory length is not taken: the run adapts again and writes a whole one
    np.savez(side, **{k: v for k, v in kept.items() if k not in ("traj", "max_steps", "iteration")})
    prof3 = {}
    s3 = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, transform=tr, seed=7)
    s3.sample(None, n1 + 200, samp_eps=0, Madapt=150, outdir=out, method="hmc", profile=prof3, adapt_traj=True)
    with np.load(side) as f:
        assert prof3["host_adapt_s"] > 0 and float(f["traj"]) > 0 and int(f["max_steps"]) == 64
    # overwrite: the file is gone before the run, which adapts again
    np.savez(side, **dict(kept, traj=np.float64(123.0)))
    prof4 = {}
    s4 = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, transform=tr, seed=8)
    s4.sample(None, 100, samp_eps=0, Madapt=150, outdir=out, method="hmc", profile=prof4, adapt_traj=True, overwrite=True)
    with np.load(side) as f:
        assert float(f["traj"]) != 123.0 and prof4["host_adapt_s"] > 0
    assert len(sampler.ChainStore.load(name)["chain"]) == 100
    # without the keyword: no file, the fixed samp_steps in whole blocks
    sub = os.path.join(out, "plain"); os.makedirs(sub)
    del calls[:]
    s5 = sampler.HMCSampler(t["lp"], None, None, nd, nw, x0=z0, transform=tr, seed=9)
    s5.sample(None, 100, samp_steps=3, samp_eps=0, Madapt=20, outdir=sub, method="hmc")
    assert not os.path.exists(os.path.join(sub, "chhmc_adapt.npz"))
    assert calls and all(c[1:] == (100, 3) for c in calls)
    # the same through run_mcmc
    sub = os.path.join(out, "run_mcmc"); os.makedirs(sub)
    nns = util.NN_samplerv1(sub, None)
    np.random.seed(3)
    del calls[:]
    util.run_mcmc(nns, sub, "hmc", nd, nw, chees.MEAN, t["lp"], transform=tr, max_n=100, adapt_traj=True, max_steps=16)
    d3 = sampler.ChainStore.load(os.path.join(sub, "chhmc.h5"))
    assert d3["chain"].shape == (100, nw, nd) and np.isfinite(d3["log_prob"]).all()
    with np.load(os.path.join(sub, "chhmc_adapt.npz")) as f:
        assert int(f["max_steps"]) == 16 and float(f["traj"]) > 0
    assert calls and all(c[1] == 1 and 1 <= c[2] <= 16 for c in calls)
