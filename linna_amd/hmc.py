"""Batched per-walker HMC chains and their warm-up schemes (linna_amd.sampler re-exports ``BatchedHMC``)."""
import ctypes as C
import math
import warnings

import numpy as np
import torch

from . import _lib
from .ensemble import EnsembleSampler


class BatchedHMC(object):
    """``linna/HMCSampler.py:19-68`` for B independent chains: p ~ N(0, m); half kick; ``num_steps``
    x (drift, gradient, kick); final half kick; Metropolis test on H = p^2/2m - lnP.

    ``log_prob`` may be a ``Log_prob(precision="bf16", grad_precision="bf16")``: lnP and its gradient then come from the one
    bf16 launch (``linna_logprob_set_grad_precision``), in both the fused and the piecewise form.  The leapfrog with any
    deterministic force that depends on q alone is reversible and volume-preserving, and lnP at the start and at the end
    of a trajectory both come from the gradient launch: the chain samples the density that launch returns, the rounded
    force costs acceptance rate only.  A ``precision="bf16"`` object without the second opt-in raises here.

    ``step`` / ``sample`` take one scalar step size and enqueue a transition launch by launch.  ``run`` enqueues a block of
    transitions in one C call (always linna_hmc_run_energy: whatever is off is a null pointer) with a step size per chain (``self.eps``, device), which ``find_reasonable_epsilon`` chooses
    and ``run(..., Madapt=n)`` adapts by dual averaging (``self.epsbar``, ``Hbar``, ``mu``, ``m``): what ``HMCSampler.sample(
    method="hmc")`` drives.  Both routes share one Philox sequence (``iteration``).  ``adapt`` is the whole warm-up, with
    the diagonal mass adapted from the positions of all chains on request (``mass_windows``, ``run(moments=True)``,
    ``mass_from_moments``): ``self.mass`` is rewritten in place on the device.

    A 2-D ``mass[ndim][ndim]`` (symmetric positive definite, ``ndim`` <= 128) or ``adapt(adapt_mass="dense")`` puts the
    object in dense mode: with C = chol(M^-1) the chains carry the whitened momentum w = C^T p -- the draw is w ~ N(0, I), the
    kinetic energy |w|^2 / 2, the kick w += eps C^T g and the drift q += eps C w -- so ``self.mass`` is an array of ones,
    ``self.chol`` the device pair {C, C^T} ``[2][ndim][ld]``, and every route (``step``, ``run``, ``find_reasonable_epsilon``,
    ``run(moments=True)`` with the co-moments in ``self.comom``) enqueues the dense launches (those of linna_hmc_run_dense).

    ``adapt_traj`` (or ``adapt(adapt_traj=True)``) gives all chains one step size and a trajectory length ``self.traj`` learned
    during a warm-up of its own (ChEES-HMC, linna_hmc_chees_begin / linna_hmc_chees_end); ``run()`` without ``num_steps`` then
    runs ``steps_for(i)`` leapfrog steps at Philox step i, under whatever mass the object has.

    ``energy_stats()`` switches the energy diagnostics on: every transition of ``run()`` then also counts as divergent when its
    proposal is not finite or its energy error H1 - H0 exceeds ``max_dH``, and feeds the energy of the state it ends in to
    per-chain float64 accumulators, all inside the Metropolis launch (linna_hmc_run_energy); ``energy_summary()`` reads the
    E-BFMI per chain (Betancourt 2016; Stan's definition) and the divergence counts.  The chains are bit for bit the same.
    A divergence is judged on the end point of the trajectory only.  Warm-ups (``adapt``, ``adapt_traj``,
    ``find_reasonable_epsilon``) are never counted."""

    DENSE_MAX_NDIM = 128                        # LINNA_HMC_DENSE_MAX_NDIM

    def __init__(self, log_prob, x0, mass=None, seed=0, fused=True, dist_group=None):
        self.group = dist_group                 # the process group a driver gathers chain blocks over (gather_chain); chains never exchange
        self.fused = fused                      # kick + drift in the gradient launch's finish (False: the separate entries)
        if not getattr(log_prob, "device_only", True):
            raise NotImplementedError("HMC needs the gradient of the log-probability: a user loglikelihoodfunc / "
                                      "externalloglike is host code without one")
        self.lp = log_prob
        p = log_prob._ensure()
        self.dev, self.ctx = p["dev"], _lib.ctx(p["dev"].index)
        x0 = torch.as_tensor(np.asarray(x0, np.float32), device=self.dev)
        self.B, self.ndim = x0.shape
        self.ld = _lib.ld4(self.ndim)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.dev)
        self.x, self.q, self.p = z(self.B, self.ld), z(self.B, self.ld), z(self.B, self.ld)
        self.x[:, :self.ndim].copy_(x0)
        self._info = 0
        self.chol, self.comom, self._cnt = None, None, None     # dense mode: {C, C^T}, the co-moments, {unsettled chains, info}
        chol = None
        if mass is not None and np.ndim(mass) == 2:
            chol, mass = self.chol_of_mass(mass, self.ndim), None
        self.mass = torch.ones(self.ndim, dtype=torch.float32, device=self.dev) if mass is None else \
            torch.as_tensor(np.asarray(mass, np.float32), device=self.dev)
        if chol is not None:
            self._set_chol(chol)
        self.lnp, self.lnp_new, self.H0 = z(self.B), z(self.B), z(self.B)
        self.g, self.g_new = z(self.B, self.ld), z(self.B, self.ld)
        self.naccept = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.seed = int(seed)
        # run(): a step size per chain and the dual-averaging state of its adaptation (sampler.py:198-211 of the reference)
        self.eps, self.alpha = z(self.B), z(self.B)
        self.epsbar, self.Hbar, self.mu = torch.ones_like(self.eps), z(self.B), z(self.B)
        self.m = torch.ones(self.B, dtype=torch.int32, device=self.dev)
        self.mom = None                         # run(moments=True): {n, mean[ndim], M2[ndim]} of the positions, device float64
        self.num_steps = 5                     # run()'s default (HMCSampler.sample sets it)
        # adapt_traj(): the trajectory length run() then divides into leapfrog steps, its cap, the device state of the adaptation
        self.traj, self.max_steps, self.chees, self._traj_eps = None, _lib.CHEES_MAX_STEPS, None, None
        # energy_stats(): {n, mean, M2, D2, Eprev} per chain (device float64), the divergent transitions per chain, the bound on
        # the energy error; _warm > 0 while a warm-up runs (its transitions are never counted)
        self.estate, self.ndiv, self.max_dH, self._warm = None, None, 1000.0, 0
        self.nw, self.iteration, self._dev_steps = self.B, 0, 0     # (what _run_blocks / _Ranks.gather read; Philox step = iteration)
        self._state = None
        self.lp.evaluate_with_grad(self.x, out=self.lnp, grad=self.g)

    theta_of = EnsembleSampler.theta_of
    gather_chain = EnsembleSampler.gather_chain

    def _hmc_state(self):
        if self._state is None:
            self._state = _lib.HmcState(B=self.B, ld=self.ld, seed=self.seed, step_dev=self.step_dev.data_ptr(),
                                        mass=self.mass.data_ptr(), X=self.x.data_ptr(), lnp=self.lnp.data_ptr(), G=self.g.data_ptr(),
                                        P=self.p.data_ptr(), Q=self.q.data_ptr(), lnp_new=self.lnp_new.data_ptr(),
                                        Gnew=self.g_new.data_ptr(), H0=self.H0.data_ptr())
        return C.byref(self._state)

    @staticmethod
    def chol_of_mass(mass, ndim):
        """C = chol(M^-1) in float64 of a dense mass ``M[ndim][ndim]``; ``ValueError`` unless M is symmetric positive definite
        and ``ndim`` within the dense kernels' limit."""
        M = np.asarray(mass, np.float64)
        if M.shape != (ndim, ndim):
            raise ValueError("a dense mass is m[ndim][ndim] = [%d][%d], not %r" % (ndim, ndim, M.shape))
        if ndim > BatchedHMC.DENSE_MAX_NDIM:
            raise ValueError("a dense mass holds at most %d parameters, not %d" % (BatchedHMC.DENSE_MAX_NDIM, ndim))
        if not np.isfinite(M).all() or not np.allclose(M, M.T, rtol=1e-10, atol=0.0):
            raise ValueError("a dense mass must be a finite symmetric matrix")
        try:
            np.linalg.cholesky(M)
            return np.linalg.cholesky(np.linalg.inv(M))
        except np.linalg.LinAlgError:
            raise ValueError("a dense mass must be positive definite")

    def _set_chol(self, Cl):
        """Dense mode with the lower-triangular factor ``Cl`` of the inverse mass: {C, C^T} to the device (in place once
        allocated), ones into ``self.mass`` in place -- the pointers the kernels hold stay the same."""
        if self.ndim > self.DENSE_MAX_NDIM:
            raise ValueError("a dense mass holds at most %d parameters, not %d" % (self.DENSE_MAX_NDIM, self.ndim))
        Cl = np.tril(np.asarray(Cl, np.float64)).astype(np.float32)
        pair = np.zeros((2, self.ndim, self.ld), np.float32)
        pair[0, :, :self.ndim], pair[1, :, :self.ndim] = Cl, Cl.T
        if self.chol is None:
            self.chol = torch.zeros((2, self.ndim, self.ld), dtype=torch.float32, device=self.dev)
        self.chol.copy_(torch.as_tensor(pair))
        self.mass.fill_(1.0)

    def cov(self):
        """C C^T of dense mode in float64 (the inverse of the mass the chains run under)."""
        Cl = self.chol[0, :, :self.ndim].cpu().numpy().astype(np.float64)
        return Cl @ Cl.T

    def find_reasonable_epsilon(self, max_rounds=40):
        """A first step size per chain (``self.eps``): the reference's ``find_reasonable_epsilon`` (sampler.py:151-184) for all
        chains at once -- ``max_rounds`` one-step trials of every chain enqueued in one C call, nothing read back between them
        (linna_hmc_find_epsilon); then the dual averaging starts over from it (mu = log 10 eps, :202-208).  Returns the number of
        chains that were still searching after the last round (they keep the step size reached; a warning says so)."""
        r0 = torch.empty((self.B, self.ld), dtype=torch.float32, device=self.dev)
        state = torch.empty(self.B, dtype=torch.int32, device=self.dev)
        if self._cnt is None:                   # {chains left searching, info of the last factorisation}: one read for both
            self._cnt = torch.zeros(2, dtype=torch.int32, device=self.dev)
        left = self._cnt
        h, ws = self.lp._ensure()["handle"], _lib.ptr(self.lp._workspace(self.B, True))
        dense = () if self.chol is None else (_lib.ptr(self.chol), self.ld)
        _lib.call("linna_hmc_find_epsilon_dense" if dense else "linna_hmc_find_epsilon", h, self._hmc_state(), ws, *dense,
                  _lib.ptr(r0), _lib.ptr(self.eps), _lib.iptr(state), _lib.iptr(left), self.iteration - self._dev_steps,
                  int(max_rounds), _lib.stream())
        torch.log(10.0 * self.eps, out=self.mu)
        self.epsbar.fill_(1.0); self.Hbar.zero_(); self.m.fill_(1)
        n, self._info = (int(v) for v in left.tolist())
        if n:
            warnings.warn("find_reasonable_epsilon: %d of %d chains had not settled after %d rounds; they keep the step size "
                          "they reached" % (n, self.B, max_rounds))
        return n

    def run(self, ntrans, num_steps=None, store=True, Madapt=0, target_accept=0.65, moments=False, energy=False):
        """``ntrans`` transitions of ``num_steps`` leapfrog steps with the per-chain step sizes ``self.eps``, enqueued by ONE C
        call (``_enqueue``: 2 + num_steps launches per transition, the chain rows written by the Metropolis launch); returns
        (chain[ntrans, B, ndim], lnp[ntrans, B]) as device tensors, (None, None) without ``store``.  Bit for bit a loop of
        ``step()`` at that step size.  ``Madapt`` > 0: every chain whose transition count ``self.m`` is <= Madapt adapts its
        step size by dual averaging towards the acceptance ``target_accept`` and freezes it at the averaged one on transition
        Madapt + 1 (the count carries over from call to call).  ``moments``: one more launch per transition merges the B
        positions behind it into ``self.mom`` = {n, mean[ndim], M2[ndim]} (device float64; what linna_hmc_run_moments adds
        to linna_hmc_run); the chains are bit for bit the same.

        Without ``num_steps`` and with a trajectory length in place (``adapt_traj`` / ``set_traj``): one C call per
        transition, the one at Philox step i with ``steps_for(i)`` leapfrog steps, into the rows of the same block --
        bit for bit a loop of ``run(1, num_steps=steps_for(i))``.  An explicit ``num_steps`` means what it always did.

        With ``energy_stats()`` on, the transitions of every route above are counted.
        ``energy``: returns (chain, lnp, E[ntrans, B], dH[ntrans, B]) -- the energy of the state every transition ended in and
        its energy error H1 - H0, device float32 (with the statistics off too)."""
        by_length = num_steps is None and self.traj is not None
        num_steps = self.num_steps if num_steps is None else int(num_steps)
        chain = torch.empty((ntrans, self.B, self.ndim), dtype=torch.float32, device=self.dev) if store else None
        lps = torch.empty((ntrans, self.B), dtype=torch.float32, device=self.dev) if store else None
        E, dH = ((torch.empty((ntrans, self.B), dtype=torch.float32, device=self.dev) for _ in range(2)) if energy else (None, None))
        if by_length:
            for k in range(ntrans):
                self._enqueue(1, self.steps_for(self.iteration), chain[k:k + 1] if store else None, lps[k:k + 1] if store else None,
                              Madapt, target_accept, moments, (E[k:k + 1], dH[k:k + 1]) if energy else None)
        elif ntrans > 0:
            self._enqueue(ntrans, num_steps, chain, lps, Madapt, target_accept, moments, (E, dH) if energy else None)
        return (chain, lps, E, dH) if energy else (chain, lps)

    def _enqueue(self, ntrans, num_steps, chain, lps, Madapt, target_accept, moments, rows=None):
        """run()'s one C call: ``ntrans`` transitions of ``num_steps`` leapfrog steps, their rows to ``chain`` / ``lps`` (and
        ``rows`` = (E, dH)).  Always linna_hmc_run_energy: what is off -- a dense factor, the moments, the energy statistics,
        the rows -- is a null pointer, and the call is then bit for bit linna_hmc_run / _run_moments / _run_dense."""
        h, ws = self.lp._ensure()["handle"], _lib.ptr(self.lp._workspace(self.B, True))
        count = self.estate is not None and not self._warm
        mom = None if not moments else _lib.ptr(self._moments() if self.chol is None else self._comoments(), torch.float64)
        E, dH = rows if rows is not None else (None, None)
        _lib.call("linna_hmc_run_energy", h, self._hmc_state(), ws, _lib.ptr(self.chol), self.ld if self.chol is not None else 0,
                  _lib.ptr(self.eps), _lib.ptr(self.epsbar), _lib.ptr(self.Hbar), _lib.ptr(self.mu), _lib.iptr(self.m), int(Madapt),
                  float(target_accept), self.iteration - self._dev_steps, int(num_steps), int(ntrans), _lib.iptr(self.naccept),
                  _lib.ptr(self.alpha), _lib.ptr(chain), _lib.ptr(lps), mom,
                  _lib.ptr(self.estate, torch.float64) if count else None, _lib.iptr(self.ndiv) if count else None,
                  float(self.max_dH), _lib.ptr(E), _lib.ptr(dH), _lib.stream())
        self.iteration += ntrans

    def energy_stats(self, on=True, max_dH=1000.0):
        """Switch the energy diagnostics on (the accumulators allocated, or zeroed if they exist) or off.  ``max_dH``: the
        energy error H1 - H0 above which a transition is divergent (Stan's 1000); not positive: a ``ValueError``."""
        if not on:
            self.estate = self.ndiv = None
            return
        if not float(max_dH) > 0.0:
            raise ValueError("energy_stats: max_dH = %r is not positive" % (max_dH,))
        self.max_dH = float(max_dH)
        if self.estate is None:
            self.estate = torch.zeros((self.B, _lib.ENERGY_DOUBLES), dtype=torch.float64, device=self.dev)
            self.ndiv = torch.zeros(self.B, dtype=torch.int32, device=self.dev)
        else:
            self.energy_reset()

    def energy_reset(self):
        """Empty the accumulators and the divergence counts (nothing without ``energy_stats()``)."""
        if self.estate is not None:
            self.estate.zero_()
            self.ndiv.zero_()

    def energy_finish(self, estate=None, ndiv=None):
        """linna_hmc_energy_finish on the accumulators (or on copies of them): (bfmi[B] float32, pooled[3] float64), device."""
        estate, ndiv = self.estate if estate is None else estate, self.ndiv if ndiv is None else ndiv
        bfmi = torch.empty(self.B, dtype=torch.float32, device=self.dev)
        pooled = torch.empty(3, dtype=torch.float64, device=self.dev)
        _lib.call("linna_hmc_energy_finish", self.ctx, self.B, _lib.ptr(estate, torch.float64), _lib.iptr(ndiv), _lib.ptr(bfmi),
                  _lib.ptr(pooled, torch.float64), _lib.stream())
        return bfmi, pooled

    def energy_summary(self):
        """dict(bfmi[B], ndivergent[B], n[B], bfmi_min, ndivergent_total, chains_divergent, max_dH) of the transitions counted
        so far: E-BFMI per chain as D2 / M2 (Stan's definition; NaN for fewer than two energies or a constant one), its
        minimum over the chains (NaN ones ignored), the divergent transitions per chain, their sum and the chains that had one."""
        if self.estate is None:
            raise ValueError("energy_summary: the energy diagnostics are off (energy_stats() first)")
        bfmi, pooled = self.energy_finish()
        pooled = pooled.tolist()
        return dict(bfmi=bfmi.cpu().numpy(), ndivergent=self.ndiv.cpu().numpy(), n=self.estate[:, 0].cpu().numpy().astype(np.int64),
                    bfmi_min=pooled[0], ndivergent_total=int(pooled[1]), chains_divergent=int(pooled[2]), max_dH=self.max_dH)

    @staticmethod
    def halton(t):
        """The base-2 van der Corput number of ``t`` >= 1: 1/2, 1/4, 3/4, 1/8, ..."""
        h, f, t = 0.0, 0.5, int(t)
        while t > 0:
            if t & 1:
                h += f
            f *= 0.5
            t >>= 1
        return h

    @staticmethod
    def traj_steps(h, T, eps, max_steps):
        """clamp(ceil(h T / eps), 1, max_steps) in float64 (anything that is not a number >= 1: one step)."""
        r = h * T / eps
        return int(math.ceil(min(r, float(max_steps)))) if r >= 1.0 else 1

    def steps_for(self, i):
        """The leapfrog steps of the transition at Philox step ``i`` once ``adapt_traj`` has set ``self.traj``:
        clamp(ceil(h_{i + 1} T / eps), 1, max_steps) -- a function of ``i`` alone, so a resumed run continues the sequence."""
        if self.traj is None:
            raise ValueError("steps_for: no trajectory length (adapt_traj or set_traj first)")
        return self.traj_steps(self.halton(int(i) + 1), self.traj, self._traj_eps, self.max_steps)

    def set_traj(self, traj, max_steps=None):
        """``run()`` without ``num_steps`` divides the trajectory length ``traj`` by the step size all chains share
        (``self.eps[0]``) from now on; ``traj`` None: back to ``self.num_steps``."""
        if traj is None:
            self.traj = self._traj_eps = None
            return
        traj, max_steps = float(traj), int(self.max_steps if max_steps is None else max_steps)
        eps = float(self.eps[0])
        if not (np.isfinite(traj) and traj > 0 and np.isfinite(eps) and eps > 0 and max_steps >= 1):
            raise ValueError("set_traj: trajectory length %r, step size %r, max_steps %r" % (traj, eps, max_steps))
        self.traj, self._traj_eps, self.max_steps = traj, eps, max_steps

    def adapt_traj(self, M, target_accept=0.65, max_steps=None):
        """ChEES-HMC's warm-up (Hoffman, Radul & Sountsov 2021; include/linna_hip.h states the scheme): ``M`` transitions in
        which all chains share one step size -- it starts at the median of ``find_reasonable_epsilon()``'s and is adapted by
        dual averaging on the harmonic mean of the acceptance probabilities -- and one trajectory length T, which climbs
        the gradient of the ChEES criterion by Adam.  Transition t runs clamp(ceil(h_t T / eps), 1, max_steps) leapfrog steps
        between linna_hmc_chees_begin and linna_hmc_chees_end under the mass this object has; the host reads the 12 state
        words once per transition to know that number.  The last transition puts the averaged step size and length in
        place: ``self.eps[:]``, ``self.traj``; ``run()`` without ``num_steps`` then runs ``steps_for(i)`` steps.  Nothing is
        stored; ``self.naccept`` counts the warm-up's transitions.  Returns (traj, eps)."""
        M, max_steps = int(M), int(_lib.CHEES_MAX_STEPS if max_steps is None else max_steps)
        if M < 1 or max_steps < 1:
            raise ValueError("adapt_traj: M = %r warm-up transitions, max_steps = %r: both at least 1" % (M, max_steps))
        self._warm += 1
        try:
            return self._adapt_traj(M, target_accept, max_steps)
        finally:
            self._warm -= 1

    def _adapt_traj(self, M, target_accept, max_steps):
        self.traj = self._traj_eps = None
        self.find_reasonable_epsilon()
        eps0 = float(torch.median(self.eps))
        if not (np.isfinite(eps0) and eps0 > 0):
            raise ValueError("adapt_traj: the median step size of the search is %r" % (eps0,))
        self.eps.fill_(eps0)
        head = np.zeros(int(_lib.load().linna_hmc_chees_doubles(self.ndim)), np.float64)
        head[0], head[1], head[5], head[7] = 1.0, math.log(eps0), math.log(10.0 * eps0), math.log(eps0)
        self.chees = torch.as_tensor(head, device=self.dev)
        r0 = torch.empty(self.B, dtype=torch.float64, device=self.dev)
        dense = (None, 0) if self.chol is None else (_lib.ptr(self.chol), self.ld)
        D = lambda t: _lib.ptr(t, torch.float64)
        for t in range(1, M + 1):
            st = self.chees[:_lib.CHEES_HEAD].tolist()        # (the one read of the transition: log T and log eps)
            L = self.traj_steps(self.halton(t), math.exp(st[1]), math.exp(st[7]), max_steps)
            _lib.call("linna_hmc_chees_begin", self.ctx, self.B, self.ndim, _lib.ptr(self.x), self.ld, D(self.chees), D(r0), _lib.stream())
            self._enqueue(1, L, None, None, 0, target_accept, False)
            _lib.call("linna_hmc_chees_end", self.ctx, self.B, self.ndim, _lib.ptr(self.mass), *dense, _lib.ptr(self.q), self.ld,
                      _lib.ptr(self.p), self.ld, _lib.ptr(self.alpha), D(r0), D(self.chees), _lib.ptr(self.eps), M,
                      float(target_accept), max_steps, _lib.stream())
        st = self.chees[:_lib.CHEES_HEAD].tolist()
        self.epsbar.copy_(self.eps)
        self.set_traj(math.exp(st[1]), max_steps)
        return self.traj, self._traj_eps

    def _moments(self):
        if self.mom is None:
            self.mom = torch.zeros(1 + 2 * self.ndim, dtype=torch.float64, device=self.dev)
        return self.mom

    def _comoments(self):
        """``self.comom`` = {n, c[ndim], 8 x {S1[ndim], S2[ndim][ndim]}} (device float64, include/linna_hip.h)."""
        if self.comom is None:
            self.comom = torch.zeros(int(_lib.load().linna_hmc_comoments_doubles(self.ndim)), dtype=torch.float64, device=self.dev)
        return self.comom

    def chol_from_comoments(self, reset=True):
        """``self.chol`` <- the Cholesky factor of the pooled covariance in ``self.comom`` with Stan's shrinkage, on the device
        (linna_hmc_chol_from_comoments); its info word lands in ``self._cnt[1]``, which ``find_reasonable_epsilon`` reads."""
        _lib.call("linna_hmc_chol_from_comoments", self.ctx, self.ndim, _lib.ptr(self._comoments(), torch.float64),
                  _lib.ptr(self.chol), self.ld, C.c_void_p(self._cnt.data_ptr() + 4), int(bool(reset)), _lib.stream())

    @staticmethod
    def mass_windows(Madapt, init_buffer=75, term_buffer=50, base_window=25):
        """Stan's warm-up schedule: the "slow" windows [(start, end), ...] of ``Madapt`` adaptive transitions in which the
        positions are accumulated for the mass, between an initial buffer and a closing one that adapt the step size alone.
        Windows double in length; one whose successor would not fit in front of the closing buffer runs up to it.  A warm-up
        too short for 75 + 25 + 50 splits 15 % / 75 % / 10 %; fewer than 20 transitions: no window."""
        Madapt = int(Madapt)
        if Madapt < 20:
            return []
        init, term, base = int(init_buffer), int(term_buffer), int(base_window)
        if init + base + term > Madapt:
            init, term = int(0.15 * Madapt), int(0.1 * Madapt)
            base = Madapt - init - term
        out, start, size, last = [], init, base, Madapt - term
        while start < last:
            end = start + size
            if end + 2 * size > last:
                end = last
            out.append((start, end))
            start, size = end, 2 * size
        return out

    def mass_from_moments(self, reset=True):
        """``self.mass`` <- 1 / the pooled variance in ``self.mom`` with Stan's shrinkage, in place on the device
        (linna_hmc_mass_from_moments: the pointer the kernels hold stays the same); ``reset`` empties the moments."""
        _lib.call("linna_hmc_mass_from_moments", self.ctx, self.ndim, _lib.ptr(self._moments(), torch.float64), _lib.ptr(self.mass),
                  int(bool(reset)), _lib.stream())

    def adapt(self, Madapt, target_accept=0.65, adapt_mass=True, adapt_traj=False, max_steps=None):
        """The whole warm-up: ``find_reasonable_epsilon()`` and ``Madapt`` transitions of dual averaging plus the one that puts
        the averaged step size in place.  ``adapt_mass``: Stan's windowed scheme around them -- in every window of
        ``mass_windows(Madapt)`` the positions of all chains are accumulated on the device; at its end
        mass[d] <- 1 / var[d], the step-size search runs again under the new mass and the dual averaging starts over, so that
        only the last segment freezes.  Without windows (or ``adapt_mass=False``): the plain sequence.  Nothing is read back
        inside a segment; ``self.naccept`` counts the warm-up's transitions too.

        ``adapt_mass="dense"`` (``True`` and ``"diag"`` are the scheme above): the same windows and segments for a dense mass.
        The object enters dense mode from its diagonal mass (C = diag(1 / sqrt(m))); the windows accumulate co-moments about
        the first chain's position; at a window's end ``self.chol`` <- the Cholesky factor of the pooled covariance
        (``chol_from_comoments``).  A covariance that cannot be factored keeps the factor before it, with a warning.

        ``adapt_traj``: behind all of the above ``adapt_traj(Madapt, target_accept, max_steps)`` adapts one shared step size
        and the trajectory length under the mass the sequence above produced."""
        self._warm += 1
        try:
            windows = self._adapt(Madapt, target_accept, adapt_mass)
            if adapt_traj:
                self.adapt_traj(Madapt, target_accept, max_steps)
        finally:
            self._warm -= 1
        return windows

    def _adapt(self, Madapt, target_accept, adapt_mass):
        Madapt = int(Madapt)
        adapt_mass = self.adapt_mass_mode(adapt_mass)
        dense = adapt_mass == "dense"
        if dense and self.chol is None:
            self._set_chol(np.diag(1.0 / np.sqrt(self.mass.cpu().numpy().astype(np.float64))))
        elif adapt_mass and not dense and self.chol is not None:
            raise ValueError("adapt_mass = %r: this object runs under a dense mass (adapt_mass=\"dense\")" % (adapt_mass,))
        self.find_reasonable_epsilon()
        windows = self.mass_windows(Madapt) if adapt_mass else []
        if not windows:
            if Madapt > 0:
                self.run(Madapt + 1, store=False, Madapt=Madapt, target_accept=target_accept)
            return windows
        never = 2 ** 30                                   # (dual averaging that does not freeze inside the segment)
        self.run(windows[0][0], store=False, Madapt=never, target_accept=target_accept)
        if dense:
            self._comoments().zero_()
            self.comom[1:1 + self.ndim].copy_(self.x[0, :self.ndim])      # the shift c: a point of the cloud
        else:
            self._moments().zero_()
        for start, end in windows:
            self.run(end - start, store=False, Madapt=never, target_accept=target_accept, moments=True)
            if dense:
                self.chol_from_comoments(reset=True)
            else:
                self.mass_from_moments(reset=True)
            self.find_reasonable_epsilon()                # (under the new mass; mu, epsbar, Hbar, m start over)
            if dense and self._info:
                warnings.warn("adapt: the pooled covariance of window (%d, %d) could not be factored (info %d); the factor "
                              "before it stays" % (start, end, self._info))
        left = Madapt - windows[-1][1]
        self.run(left + 1, store=False, Madapt=left, target_accept=target_accept)
        return windows

    @staticmethod
    def adapt_mass_mode(adapt_mass):
        """``adapt_mass`` as one of False, "diag", "dense" (True is "diag"); anything else is a ``ValueError``."""
        if isinstance(adapt_mass, str):
            if adapt_mass in ("diag", "dense"):
                return adapt_mass
        elif isinstance(adapt_mass, (bool, np.bool_)) or adapt_mass is None:
            return "diag" if adapt_mass else False
        raise ValueError("adapt_mass = %r: False, True / \"diag\" or \"dense\"" % (adapt_mass,))

    def step(self, num_steps, step_size, p0=None, u=None):
        """One HMC transition per chain.  ``p0[B, ndim]`` (standard-normal draws) and ``u[B]`` replace
        the Philox draws when given (replaying HMCSampler.py:26 / :59 streams)."""
        st, eps = _lib.stream(), float(step_size)
        seed = C.c_uint64(self.seed)
        args = (self.ctx, self.B, self.ndim, _lib.ptr(self.mass))
        if self._dev_steps != self.iteration:       # run() counts its transitions on the host: the entries here read the device counter
            self.step_dev.fill_(self.iteration)
            self._dev_steps = self.iteration
        p0d = None if p0 is None else torch.as_tensor(np.ascontiguousarray(p0, np.float32), device=self.dev)
        ud = None if u is None else torch.as_tensor(np.ascontiguousarray(u, np.float32), device=self.dev)
        if self.chol is not None:
            # dense mode, launch by launch what linna_hmc_run_dense enqueues: draw + H0 on the unit mass; half kick and drift
            # from x; per step the gradient and the dense kick and drift behind it (a half kick, no drift behind the last)
            dn = (self.ctx, self.B, self.ndim, _lib.ptr(self.chol), self.ld, None)
            _lib.call("linna_hmc_init", *args, seed, _lib.iptr(self.step_dev), _lib.ptr(self.lnp),
                      _lib.ptr(p0d) if p0d is not None else None, self.ndim, _lib.ptr(self.p), self.ld, _lib.ptr(self.H0), st)
            _lib.call("linna_hmc_kick_drift_dense", *dn, 0.5 * eps, eps, _lib.ptr(self.g), self.ld, _lib.ptr(self.p), self.ld,
                      _lib.ptr(self.x), self.ld, _lib.ptr(self.q), self.ld, st)
            for i in range(num_steps):
                last = i == num_steps - 1
                self.lp.evaluate_with_grad(self.q, out=self.lnp_new, grad=self.g_new)
                _lib.call("linna_hmc_kick_drift_dense", *dn, 0.5 * eps if last else eps, 0.0 if last else eps,
                          _lib.ptr(self.g_new), self.ld, _lib.ptr(self.p), self.ld, None, 0, _lib.ptr(self.q), self.ld, st)
            self._accept(args, seed, ud, st)
            return
        if self.fused and num_steps >= 1:
            # 3 + num_steps launches: momentum draw + first half kick + first drift; per leapfrog step the gradient with the
            # next kick (a half one behind the last step, :51) and drift in its finish; Metropolis test; counter
            _lib.call("linna_hmc_start", *args, seed, _lib.iptr(self.step_dev), _lib.ptr(self.lnp),
                      _lib.ptr(p0d) if p0d is not None else None, self.ndim, _lib.ptr(self.g), self.ld, 0.5 * eps, eps,
                      _lib.ptr(self.x), self.ld, _lib.ptr(self.p), self.ld, _lib.ptr(self.q), self.ld, _lib.ptr(self.H0), st)
            h, ws = self.lp._ensure()["handle"], _lib.ptr(self.lp._workspace(self.B, True))
            for i in range(num_steps):
                last = i == num_steps - 1
                _lib.call("linna_logprob_grad_leapfrog", h, _lib.ptr(self.q), self.ld, self.B, ws, _lib.ptr(self.lnp_new),
                          _lib.ptr(self.g_new), self.ld, _lib.ptr(self.p), self.ld, _lib.ptr(self.mass),
                          0.5 * eps if last else eps, 0.0 if last else eps, st)
            self._accept(args, seed, ud, st)
            return
        _lib.call("linna_hmc_init", *args, seed, _lib.iptr(self.step_dev), _lib.ptr(self.lnp),
                  _lib.ptr(p0d) if p0d is not None else None, self.ndim, _lib.ptr(self.p), self.ld, _lib.ptr(self.H0), st)
        self.q.copy_(self.x)
        g = self.g
        for i in range(num_steps):
            ek = 0.5 * eps if i == 0 else eps                     # :35 half kick first, full kicks after
            _lib.call("linna_hmc_kick_drift", *args, ek, eps, _lib.ptr(g), self.ld, _lib.ptr(self.p), self.ld,
                      _lib.ptr(self.q), self.ld, st)
            self.lp.evaluate_with_grad(self.q, out=self.lnp_new, grad=self.g_new)
            g = self.g_new
        _lib.call("linna_hmc_kick_drift", *args, 0.5 * eps, 0.0, _lib.ptr(g), self.ld, _lib.ptr(self.p), self.ld,
                  _lib.ptr(self.q), self.ld, st)                                             # :51
        self._accept(args, seed, ud, st)

    def _accept(self, args, seed, ud, st):
        _lib.call("linna_hmc_accept", *args, seed, _lib.iptr(self.step_dev), _lib.ptr(self.H0), _lib.ptr(self.p), self.ld,
                  _lib.ptr(self.q), self.ld, _lib.ptr(self.lnp_new), _lib.ptr(self.g_new), self.ld,
                  _lib.ptr(ud) if ud is not None else None, _lib.ptr(self.x), self.ld, _lib.ptr(self.lnp), _lib.ptr(self.g),
                  _lib.iptr(self.naccept), st)
        _lib.call("linna_step_increment", self.ctx, _lib.iptr(self.step_dev), st)
        self.iteration += 1
        self._dev_steps += 1

    def sample(self, num_samps, num_steps, step_size):
        chain = torch.empty((num_samps, self.B, self.ndim), dtype=torch.float32, device=self.dev)
        lnps = torch.empty((num_samps, self.B), dtype=torch.float32, device=self.dev)
        for i in range(num_samps):
            self.step(num_steps, step_size)
            chain[i].copy_(self.x[:, :self.ndim])
            lnps[i].copy_(self.lnp)
        return chain, lnps
