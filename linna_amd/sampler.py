"""Ensemble and HMC walkers on MI355X.

Mirrors the sampling layer of the reference: ``linna/sampler.py`` (``HMCSampler`` -- despite
its name the emcee driver, :389-554; ``checkmeanstd`` :370-387; ``ZeusSampler`` :699-737) and
the walker loop they delegate to emcee.  Here the ensemble lives on the GPU:

* ``EnsembleSampler``: affine-invariant stretch move (emcee ``StretchMove`` inside
  ``RedBlueMove``, a = 2, random split of the walkers in two halves every step).  Per half
  step: ``linna_stretch_propose`` -> fused ``Log_prob`` pipeline on the whole half ->
  ``linna_stretch_accept``; Philox draws keyed (seed; walker, step, stream).
* ``BatchedHMC``: the leapfrog of ``linna/HMCSampler.py`` run independently per walker with
  the emulator's reverse-mode gradient (``linna_logprob_grad``).
* walkers shard across ranks (one process per GPU): every rank advances its own
  sub-ensemble, chain state is gathered with one RCCL all-gather per flush.

The emcee and zeus arithmetic itself is third-party code absent from the reference tree: both moves are
restated from the published algorithms; the test suite replays the kernels against its own numpy
restatements of them (``stretch_half_step`` / ``slice_half_step`` in the repo's oracle/sampling.py --
test infrastructure, never imported here) and checks the posteriors statistically.

This module holds the drivers, their rank plumbing and stopping rules and re-exports the rest under the names it always had:
``chainstats`` (host statistics, ``DeviceChain``), ``chainstore`` (``ChainStore``, readers), ``ensemble``, ``hmc`` (``BatchedHMC``).
"""
import os
import time

import numpy as np
import torch

from . import _lib, dist as ldist
from .chainstats import (DeviceChain, _autocorr_1d, _chain3, _ndtri, _next_pow_two, _rank2, _rhat_of_scores, checkmeanstd,
                         integrated_time, multichain_ess, rank_ess, rank_rhat, split_rhat)
from .chainstore import ChainStore, _OnDisk, get_good_walker_list, read_chain_and_cut
from .ensemble import EnsembleSampler, SliceEnsembleSampler, _FastOverflow
from .hmc import BatchedHMC

__all__ = ["EnsembleSampler", "SliceEnsembleSampler", "BatchedHMC", "HMCSampler", "ZeusSampler", "checkmeanstd", "integrated_time",
           "split_rhat", "multichain_ess", "ChainStore", "DeviceChain", "read_chain_and_cut", "get_good_walker_list"]

class _Ranks(object):
    """How a driver's ensemble is split over the ranks of a run (``linna_amd.dist.init()``; the reference farms the walkers'
    log-probability calls out over its MPI pool, util.py:99-256).  Three modes (``exchange``; ``LINNA_ENSEMBLE_EXCHANGE``):

    * ``"local"`` -- the default whenever every rank's share holds a valid ensemble (``nwalkers / world >= 2 ndim``, emcee's and
      zeus' own floor): ``nwalkers / world`` walkers per GPU as a SUB-ENSEMBLE of its own -- stretch / slice partners from the
      rank's LOCAL complementary half, the slice sampler's mu tuned per sub-ensemble -- no collective inside an iteration;
      chain blocks are gathered once per convergence check ("an RCCL gather for chain state"), rank 0 alone keeps the chain
      file ([iterations, nwalkers, ndim], walker blocks in rank order) and the statistics over ALL walkers and tells the
      others when to stop.  Sub-ensembles are valid ensemble samplers of the same posterior, so the merged chain is too.
    * ``"root"`` -- shares too small for that: the whole ensemble runs on rank 0, the other ranks wait at the end of the call.
    * ``"allgather"`` -- on request only: ONE ensemble sharded, partners from the complementary walkers of ALL ranks, i.e. one
      all-gather per half step.  A small collective's latency is of the order of the 30 us half step it follows: this mode is
      slower than one GPU at every ensemble size measured and exists for runs that need the one-ensemble
      chain (its mu is tuned from the all-reduced counts)."""

    def __init__(self, nwalkers, group, ndim=None, exchange=None):
        self.group, self.real_world, self.rank = group, ldist.world_size(group), ldist.rank(group)
        want = exchange or os.environ.get("LINNA_ENSEMBLE_EXCHANGE") or "auto"
        if want not in ("auto", "local", "root", "allgather"):
            raise ValueError("exchange = %r (auto, local, root or allgather)" % (want,))
        even = nwalkers % (2 * self.real_world) == 0
        if self.real_world == 1:
            mode = "single"
        elif want == "allgather" or want == "local":
            if not even:
                raise ValueError("nwalkers = %d cannot be split into even halves over %d ranks" % (nwalkers, self.real_world))
            mode = want
        elif want == "root":
            mode = "root"
        else:
            mode = "local" if even and (ndim is None or nwalkers // self.real_world >= 2 * ndim) else "root"
        self.mode = mode
        self.active = mode != "root" or self.rank == 0               # (root: ranks > 0 do not sample)
        self.world = 1 if mode in ("single", "root") else self.real_world   # ranks that exchange data inside the sampling loop
        self.nw = nwalkers // self.world
        self.exchange = "allgather" if mode == "allgather" else "none"
        self.ens_group = group                                       # the sampler's group (chain gathers)

    def mine(self, x0):
        if self.world == 1:
            return np.asarray(x0)
        return np.asarray(x0)[self.rank * self.nw:(self.rank + 1) * self.nw]

    def bcast(self, obj):
        """A host object of rank 0 on every rank (control plane)."""
        if self.world == 1:
            return obj
        import torch.distributed as tdist
        box = [obj]
        tdist.broadcast_object_list(box, src=0 if self.group is None else tdist.get_global_rank(self.group, 0), group=self.group)
        return box[0]

    def gather(self, ens, c, l):
        """(chain block, log-probabilities, acceptance counts) of the whole ensemble on every rank."""
        if self.world == 1:
            return c, l, ens.naccept
        c, l = ens.gather_chain(c, l)
        return c, l, ldist.gather_rows(ens.naccept.float(), self.group)

    def barrier(self):
        if self.real_world > 1:
            ldist.barrier(self.group)


class _Prof(object):
    """Where a driver run spends its time (``sample(..., profile={})``): host seconds per phase and, from event pairs on
    the streams the work was enqueued on, device seconds per phase.  Without a dict every hook is a no-op."""

    def __init__(self, out):
        import collections
        self.t0 = time.perf_counter()
        self.out, self.h, self.ev = out, collections.defaultdict(float), collections.defaultdict(list)

    class _Span(object):
        __slots__ = ("p", "key", "stream", "t0", "e0")

        def __init__(self, p, key, stream):
            self.p, self.key, self.stream = p, key, stream

        def __enter__(self):
            if self.p.out is not None:
                if self.stream is not False:
                    self.e0 = torch.cuda.Event(enable_timing=True)
                    self.e0.record(self.stream if self.stream is not None else torch.cuda.current_stream())
                self.t0 = time.perf_counter()

        def __exit__(self, *a):
            if self.p.out is not None:
                self.p.h[self.key] += time.perf_counter() - self.t0
                if self.stream is not False:
                    e1 = torch.cuda.Event(enable_timing=True)
                    e1.record(self.stream if self.stream is not None else torch.cuda.current_stream())
                    self.p.ev[self.key].append((self.e0, e1))

    def host(self, key):
        return self._Span(self, key, False)

    def both(self, key, stream=None):
        """Host seconds inside the block and device seconds between two events recorded on ``stream`` around it."""
        return self._Span(self, key, stream)

    def finish(self, **extra):
        if self.out is None:
            return
        torch.cuda.synchronize()
        for k, v in self.h.items():
            self.out["host_%s_s" % k] = v
        for k, pairs in self.ev.items():
            self.out["gpu_%s_s" % k] = 1e-3 * sum(a.elapsed_time(b) for a, b in pairs)
        self.out.update(extra)


class _EnergyLog(object):
    """``energy_stats=True``: what the driver keeps of the chains' energy diagnostics (``BatchedHMC.energy_stats``; single-rank
    runs).  Every block's dH rows and a copy of the accumulators as the block left them -- taken on the sampling stream, so
    that the block sampled during a check does not show in them and a block that is dropped can be taken back -- go to the
    host on the statistics stream behind the block's chain rows; at the check ``drv.diagnostics`` gains ``bfmi``,
    ``ndivergent`` and ``divergent_fraction``, one line is printed, and ``bfmi_min`` / ``max_divergent`` gate a check that
    passed (NaN: not converged).  ``divergent_at`` collects (stored row, walker) of the divergent stored transitions: the
    start point of such a trajectory is the chain row before it.  ``chhmc_energy.npz`` holds all of it and continues a
    resumed run."""

    FILE = "chhmc_energy.npz"

    def __init__(self, drv, ens, path, bfmi_min, max_divergent, resume):
        self.drv, self.ens, self.path, self.bfmi_min, self.max_divergent = drv, ens, path, bfmi_min, max_divergent
        self.at, self.new, self.kept, self.pending, self.last = [np.zeros((0, 2), np.int64)], None, None, None, None
        if resume and os.path.exists(path):
            with np.load(path) as f:
                if {"estate", "ndivergent", "divergent_at"} <= set(f.files) and f["estate"].shape == (ens.B, _lib.ENERGY_DOUBLES) \
                        and f["ndivergent"].shape == (ens.B,):
                    ens.estate.copy_(torch.as_tensor(np.asarray(f["estate"], np.float64)))
                    ens.ndiv.copy_(torch.as_tensor(np.asarray(f["ndivergent"], np.int32)))
                    self.at = [np.asarray(f["divergent_at"], np.int64).reshape(-1, 2)]
        self.kept = (ens.estate.clone(), ens.ndiv.clone())

    def run(self, ncheck):
        """``ens.run(ncheck)`` with the block's dH rows and the accumulators behind it put aside."""
        c, l, _, dh = self.ens.run(ncheck, energy=True)
        self.new = (dh, self.ens.estate.clone(), self.ens.ndiv.clone())
        return c, l

    def drop(self):
        """The block sampled last is not stored: the accumulators go back to where the last stored block left them."""
        self.ens.estate.copy_(self.kept[0])
        self.ens.ndiv.copy_(self.kept[1])

    def keep(self, first_row):
        """The block sampled last is stored as rows ``first_row`` ...: its finish and its way to the host, enqueued on the
        current (statistics) stream."""
        dh, est, nd = self.new
        self.kept = (est, nd)
        bfmi, pooled = self.ens.energy_finish(est, nd)
        host = []
        for t in (dh, est, nd, bfmi, pooled):
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            host.append(h)
        ev = torch.cuda.Event()
        ev.record()
        self.pending = (first_row, host, ev, (dh, bfmi, pooled))        # (the device tensors live until the copies are done)

    @staticmethod
    def divergent(dH, max_dH):
        """The kernel's flag from the energy errors alone: an error that is NaN or above ``max_dH``, and an error of -inf, which
        only a proposal with lnP = +inf gives a chain that started finite."""
        dH = np.asarray(dH)
        with np.errstate(invalid="ignore"):
            return ~(dH <= np.float32(max_dH)) | np.isneginf(dH)

    def check(self, converged, n):
        """Behind a convergence check over ``n`` stored rows: the diagnostics of those rows, and the gates."""
        if self.pending is None:
            return converged
        first_row, host, ev, _ = self.pending
        self.pending = None
        ev.synchronize()
        dh, est, nd, bfmi, pooled = (h.numpy().copy() for h in host)
        t, w = np.nonzero(self.divergent(dh, self.ens.max_dH))
        self.at.append(np.stack([t + first_row, w], axis=1).astype(np.int64))
        stored = est[:, 0].sum()
        frac = float(pooled[1] / stored) if stored > 0 else float("nan")
        self.last = dict(estate=est, ndivergent=nd.astype(np.int64), bfmi=bfmi)
        if self.drv.diagnostics is None or self.drv.diagnostics.get("n") != n:      # (criterion="tau" keeps none of its own)
            self.drv.diagnostics = dict(n=n)
        self.drv.diagnostics.update(bfmi=bfmi, ndivergent=self.last["ndivergent"], divergent_fraction=frac)
        print("min bfmi, divergent transitions, chains with one, ninter: {0}, {1}, {2}, {3}\n".format(
            pooled[0], int(pooled[1]), int(pooled[2]), n), flush=True)
        with np.errstate(invalid="ignore"):
            if self.bfmi_min is not None:
                converged = bool(converged and np.all(bfmi >= self.bfmi_min))
            if self.max_divergent is not None:
                converged = bool(converged and frac <= self.max_divergent)
        return converged

    def save(self):
        """``chhmc_energy.npz``: bfmi[B], ndivergent[B], divergent_at[k][2], n[B], max_dH and the raw accumulators."""
        if self.last is None:
            return
        est = self.last["estate"]
        np.savez(self.path, bfmi=self.last["bfmi"], ndivergent=self.last["ndivergent"], divergent_at=np.concatenate(self.at, axis=0),
                 n=est[:, 0].astype(np.int64), max_dH=np.float64(self.ens.max_dH), estate=est)


def _run_blocks(ens, rk, store, dchain, done, nsamp, ncheck, incremental, rule, prof, elog=None):
    """The sampling loop of both drivers (sampler.py:530-552, :728-735): blocks of ``ncheck`` iterations, each followed by
    the chain-file append and a convergence check.  Software-pipelined: the statistics of block i run on a stream of
    their own WHILE the sampler already advances block i + 1, and the host reads their verdict (33 numbers in pinned
    memory) only after it has enqueued that block -- neither the GPU nor the host waits for a check.  When the verdict is
    "stop" the block sampled meanwhile is dropped, so the chain ends exactly where the reference's criterion ends it.
    ``rule.begin(n)`` enqueues the statistics of the ``n`` stored rows; ``rule.decide(token, n)`` reads them: True = stop."""
    dev = ens.dev
    stats = torch.cuda.Stream(device=dev) if rk.rank == 0 else None
    pending = None
    with _lib.quiet_gc():                 # (no full pass of the cyclic collector while the launch queue is a few ms deep)
        while done < nsamp:
            with prof.both("sampling"):
                c, l = ens.run(ncheck) if elog is None else elog.run(ncheck)
            c, l, acc = rk.gather(ens, c, l)
            stop = False
            if rk.rank == 0 and pending is not None:
                with prof.host("wait_check"), torch.cuda.stream(stats):
                    stop = rule.decide(pending, done)
                    if elog is not None:
                        stop = elog.check(stop, done)
                pending = None
            if rk.bcast(stop):
                if elog is not None:
                    elog.drop()
                break
            done += ncheck
            if rk.rank == 0:
                with prof.both("theta"):
                    th = ens.theta_of(c)
                with prof.host("store_append"):
                    store.append(c, th, l, acc)                               # device tensors: copied off this thread
                    if incremental:
                        store.flush(final=False)
                ready = torch.cuda.Event()
                ready.record(torch.cuda.current_stream(dev))
                stats.wait_event(ready)
                with torch.cuda.stream(stats), prof.both("stats", stats):
                    c.record_stream(stats)
                    dchain.append(c)
                    pending = rule.begin(done)
                    if elog is not None:
                        elog.keep(done - ncheck)
    if rk.rank == 0 and pending is not None:                              # the last block's check: printed, not acted upon
        with prof.host("wait_check"), torch.cuda.stream(stats):
            stop = rule.decide(pending, done)
            if elog is not None:
                elog.check(stop, done)
    if stats is not None:
        stats.synchronize()
    return done


class _TauRule(object):
    """The reference's stopping rule (sampler.py:532-552, at every `ncheck` iterations as there: tau of the whole chain now
    against tau `ncheck` iterations earlier, per parameter).  The estimate is incremental (DeviceChain), so a check costs the
    same however long the chain has grown -- rounds 1-4 thinned the checks out because each was a batch of FFTs over the chain."""

    DISCARD = 0                     # the leading fraction of the chain a check leaves out

    def __init__(self, dchain, ntimes, tautol, ncheck, nk, meanshift, stdshift):
        self.dchain, self.ntimes, self.tautol, self.ncheck, self.nk = dchain, ntimes, tautol, ncheck, nk
        self.meanshift, self.stdshift, self.old_tau = meanshift, stdshift, np.inf

    def begin(self, n):
        return self.dchain.tau_begin(discard=int(n * self.DISCARD))

    def decide(self, tok, n):
        dchain, tau = self.dchain, self.dchain.tau_end(tok)      # sampler.py:538
        old_tau, self.old_tau = self.old_tau, tau
        if np.isnan(np.sum(tau)) and n > 10:
            return True
        with np.errstate(invalid="ignore", divide="ignore"):
            converged = np.all(tau * self.ntimes < n)                          # :545-547
            converged &= np.all(np.abs(old_tau - tau) / tau < self.tautol)
            if converged and dchain.subset:
                # the estimate above averaged over a subset of the walkers: the decision is taken on all of them
                tau = dchain.integrated_time(upto=n, all_walkers=True)
                old_tau = dchain.integrated_time(upto=n - self.ncheck, all_walkers=True) if n > self.ncheck else np.inf
                converged = np.all(tau * self.ntimes < n) and np.all(np.abs(old_tau - tau) / tau < self.tautol)
            converged = converged and dchain.checkmeanstd(max(2, int(self.nk * np.mean(tau))), self.meanshift, self.stdshift)
            print("max, min tau diff, max tau, ninter: {0}, {1}, {2}, {3}\n".format(
                np.max(np.abs(old_tau - tau) / tau), np.min(np.abs(old_tau - tau) / tau), np.max(tau), n), flush=True)
        return bool(converged)


class _ZeusRule(_TauRule):
    """zeus' callback (sampler.py:667-696, every `ncheck` iterations): the mean tau of the last 80 % of the chain."""

    DISCARD = 0.2                   # sampler.py:684,729

    def decide(self, tok, n):
        dchain, tau = self.dchain, float(np.mean(self.dchain.tau_end(tok)))
        old_tau, self.old_tau = self.old_tau, tau
        with np.errstate(invalid="ignore", divide="ignore"):
            converged = tau * self.ntimes < n
            converged &= abs(old_tau - tau) / tau < self.tautol
            if converged and dchain.subset:               # decide on all walkers (the routine checks use a subset)
                tau = float(np.mean(dchain.integrated_time(discard=int(n * 0.2), upto=n, all_walkers=True)))
                prev = n - self.ncheck
                old_tau = float(np.mean(dchain.integrated_time(discard=int(prev * 0.2), upto=prev, all_walkers=True))) if prev > 0 else np.inf
                converged = tau * self.ntimes < n and abs(old_tau - tau) / tau < self.tautol
            converged = converged and bool(dchain.checkmeanstd(max(2, int(self.nk * tau)), self.meanshift, self.stdshift))
        return bool(converged)


class _RhatRule(object):
    """``criterion="rhat"``: every parameter's split-R-hat below ``rhat_tol`` and multi-chain ESS at least ``ess_min`` over the
    rows [rhat_discard n, n), both enqueued behind the block's append.  A NaN in either (a chain that never moved, a value that
    is not finite) is "not converged".  ``drv.diagnostics`` keeps the last check's values."""

    def __init__(self, dchain, drv, rhat_tol, ess_min, rhat_discard, rhat_rank, ess_rank=False):
        self.dchain, self.drv, self.rhat_tol, self.ess_min, self.rhat_discard, self.rhat_rank = dchain, drv, rhat_tol, ess_min, rhat_discard, rhat_rank
        self.ess_rank = ess_rank

    def begin(self, n):
        lo = int(float(self.rhat_discard) * n)
        if n - lo < 4:                                                    # (two halves of two rows at least)
            return dict(lo=lo, r=None, e=None)
        return dict(lo=lo, r=self.dchain.rhat_begin(lo), e=self.dchain.ess_begin(lo))

    def decide(self, tok, n):
        dchain, drv, rhat_tol, lo = self.dchain, self.drv, self.rhat_tol, tok["lo"]
        if tok["r"] is None:
            return False
        rhat, ess = dchain.rhat_end(tok["r"]), dchain.ess_end(tok["e"])
        converged = drv.rhat_rule(rhat, ess, rhat_tol, self.ess_min)
        if converged and dchain.subset:
            # the ESS above is the walker subset's: the decision is taken on all walkers (R-hat always is)
            ess = dchain.ess(lo, upto=n, all_walkers=True)
            converged = drv.rhat_rule(rhat, ess, rhat_tol, self.ess_min)
        drv.diagnostics = dict(rhat=rhat, ess=ess, n=n)
        print("max rhat, min ess, ninter: {0}, {1}, {2}\n".format(np.max(rhat), np.min(ess), n), flush=True)
        if converged and self.rhat_rank:
            # a check that passes is confirmed with the rank-normalised, folded R-hat of all walkers (a sort of the window
            # per parameter: nothing of it is enqueued, or allocated, before the cheap rule passes)
            rr = dchain.rank_rhat(lo, upto=n)
            with np.errstate(invalid="ignore"):
                converged = bool(np.all(rr < rhat_tol))
            drv.diagnostics.update(rhat_rank=rr, rhat_bulk=dchain.last_rank_rhat[:, 1].copy(), rhat_tail=dchain.last_rank_rhat[:, 2].copy())
            print("max bulk rhat, max tail rhat, ninter: {0}, {1}, {2}\n".format(
                np.max(dchain.last_rank_rhat[:, 1]), np.max(dchain.last_rank_rhat[:, 2]), n), flush=True)
        if converged and self.ess_rank:
            # and with the rank-normalised bulk-ESS and tail-ESS of all walkers (one sort of the window per parameter and the
            # lagged products of its scores: nothing of it is enqueued, or allocated, before everything above passes)
            bulk, tail = dchain.rank_ess(lo, upto=n)
            with np.errstate(invalid="ignore"):
                converged = bool(np.all(bulk >= self.ess_min) and np.all(tail >= self.ess_min))
            drv.diagnostics.update(ess_bulk=bulk, ess_tail=tail)
            print("min bulk ess, min tail ess, ninter: {0}, {1}, {2}\n".format(np.min(bulk), np.min(tail), n), flush=True)
        return converged


def _open_run(drv, entry, filename, overwrite, profile):
    """What both drivers do first: the ranks enter the call and split the ensemble; rank 0 opens the chain file -- removed with
    ``overwrite``, else continued from its last row (``resume``) -- and its ``done`` stored rows go to the device for the
    statistics.  A rank that does not sample (``rk.active`` False) has passed the closing barrier on return."""
    prof = _Prof(profile)
    ldist.enter(entry, drv.group)
    rk = _Ranks(drv.nwalkers, drv.group, drv.nparams, drv.exchange)
    store = ChainStore(filename, drv.transform)
    if not rk.active:                                    # ("root": the whole ensemble runs on rank 0)
        rk.barrier()
        return prof, rk, store, None, False, 0, None
    x0, resume = drv.x0, False
    if rk.rank == 0 and store.exists():
        if overwrite:
            store.remove()
        else:
            print("init from previous")
            prev = ChainStore.load(filename)
            x0, resume = prev["chain"][-1], True
            store.append(prev["chain"], prev["chain_transformed"], prev["log_prob"], prev["accepted"])   # re-chunked into the new file at the first flush
    x0, resume = rk.bcast((x0, resume))
    done = rk.bcast(sum(len(c) for c in store.chain))
    dchain = DeviceChain()                                               # convergence statistics stay on the GPU
    for blk in store.chain:
        dchain.append(np.asarray(blk, np.float32))
    return prof, rk, store, x0, resume, done, dchain


def _close_run(prof, rk, store, dchain, done):
    """What both drivers do last: rank 0 completes the chain file, the ranks meet, the profile is filled in."""
    if rk.rank == 0:
        with prof.host("final_flush"), _lib.stage("run_mcmc.final_flush"):
            store.flush()
    rk.barrier()                                                          # the file is complete before any rank reads it
    prof.finish(total_s=time.perf_counter() - prof.t0, iterations=done, writer_fetch_s=store.busy["fetch"], writer_append_s=store.busy["append"],
                lag_capacity=0 if dchain._S is None else len(dchain._S), lag_growths=dchain.lag_growths)
    return store


class HMCSampler(object):
    """The reference's emcee driver (sampler.py:389-554): burn-in, restart from the best region,
    sample until the integrated autocorrelation time and the mean/std drift have converged.  ``method="hmc"`` runs the same
    burn-in, restart and convergence loop with per-walker HMC chains (``BatchedHMC.run``) in place of the stretch move and
    writes ``chhmc.h5`` (``_hmc_chains``); ``"nuts"`` is not built.
    Multi-rank runs give every rank a sub-ensemble of ``nwalkers / world`` walkers and gather the chain once per convergence
    check (``_Ranks``); every rank of the run must make the call (``dist.enter`` raises within two minutes otherwise).

    ``sample(method="hmc", adapt_mass=True)`` also adapts the diagonal mass during the warm-up (``BatchedHMC.adapt``; ``m``
    is then the starting mass) and, in a single-rank run, writes the result -- ``mass[ndim]``, ``eps[nwalkers]``,
    ``num_steps``, ``Madapt`` -- to ``chhmc_adapt.npz`` next to ``chhmc.h5``: a resumed run with ``adapt_mass=True`` whose
    file matches ``ndim`` / ``nwalkers`` loads it and skips the search and the adaptation; ``overwrite=True`` removes it.
    Multi-rank runs adapt per rank from their own chains and neither write nor read that file.  ``self.mass`` is the mass
    the chains of the last hmc run ended up with.

    ``adapt_mass="dense"`` adapts a dense mass instead (``ndim`` <= 128), and ``m`` may be a symmetric positive definite
    ``m[ndim][ndim]`` (the starting mass, or with a fixed ``samp_eps`` the mass of the run).  After such a run ``self.cov`` is
    C C^T (float64), the inverse of the mass, and ``self.mass`` = 1 / diag(cov); the file then also holds
    ``metric="dense"`` and ``chol[ndim][ndim]``, and is handed only to a run of the same metric (files without ``metric``
    are diagonal).

    ``adapt_traj=True`` adapts one step size for all walkers and the trajectory length behind that warm-up
    (``BatchedHMC.adapt_traj``, at most ``max_steps`` leapfrog steps an iteration; ``samp_steps`` is then not used).  The file
    is then written and read with or without ``adapt_mass`` and also holds ``traj``, ``max_steps`` and ``iteration``; a resumed
    ``adapt_traj`` run takes it only with a finite positive ``traj`` and continues the sequence of step counts.

    ``criterion="rhat"`` (``method="hmc"`` only) replaces the reference's stopping rule -- tau, its change and the drift of the
    halves, all within-chain statistics that cannot see independent chains disagree -- by the between-chain one: the run
    stops at the first check with split-R-hat < ``rhat_tol`` (1.01, Vehtari et al. 2021) and multi-chain ESS >= ``ess_min``
    (400) for every parameter, both computed on the device over the stored rows behind the first ``rhat_discard`` fraction
    (``DeviceChain.rhat_begin`` / ``ess_begin``); ``self.diagnostics`` keeps the last check's values.  The default ``"tau"``
    is the reference's rule, unchanged.  Plain split-R-hat compares only the means of the chains: ``rhat_rank=True`` (with
    ``criterion="rhat"`` only) confirms every check that passes with the rank-normalised, folded R-hat of Vehtari et al. 2021
    over all walkers (``DeviceChain.rank_rhat``: bulk and tail, which also see chains that differ in scale) and stops only
    when max(bulk, tail) < ``rhat_tol`` for every parameter as well (NaN: not converged); ``self.diagnostics`` then also holds
    ``rhat_bulk``, ``rhat_tail`` and ``rhat_rank`` of the last confirmation.  With ``rhat_rank=False`` nothing of it runs.
    The rule's ESS is that of the raw chain: it assumes a finite variance and measures the mean only.  ``ess_rank=True`` (with
    ``criterion="rhat"`` only) confirms every check that passed all of the above with that paper's rank-normalised bulk-ESS
    and tail-ESS over all walkers (``DeviceChain.rank_ess``; tail: the smaller ESS of the 5 % and the 95 % quantile) and stops
    only when both are at least ``ess_min`` for every parameter (NaN: not converged); ``self.diagnostics`` then also holds
    ``ess_bulk`` and ``ess_tail``.  With ``ess_rank=False`` nothing of it runs.

    ``energy_stats=True`` (``method="hmc"``, single-rank runs; otherwise a ``ValueError``) reports whether the Hamiltonian
    dynamics are healthy, which neither R-hat nor ESS can: the stored transitions whose proposal was not finite or whose
    energy error H1 - H0 exceeded ``max_dH`` (divergent; judged on the trajectory's end point only) and every chain's E-BFMI
    (Betancourt 2016, Stan's definition), both accumulated inside the Metropolis launch (``BatchedHMC.energy_stats``); the
    warm-up is not counted.  At every check ``self.diagnostics`` gains ``bfmi[nwalkers]``, ``ndivergent[nwalkers]`` and
    ``divergent_fraction`` (a ``"tau"`` run gets a dict of its own) and a line is printed; at the end ``chhmc_energy.npz``
    next to ``chhmc.h5`` holds ``bfmi``, ``ndivergent``, ``divergent_at[k][2]`` = (stored row, walker) of every divergent
    stored transition -- the trajectory started at the row before it --, ``n``, ``max_dH`` and the raw accumulators
    ``estate``; a resumed run whose file fits ``nwalkers`` continues them, ``overwrite=True`` removes the file.  ``bfmi_min``
    and ``max_divergent`` (a fraction of the stored transitions; with ``criterion="rhat"`` and ``energy_stats`` only) gate the
    stopping rule: a check that passed everything else converges only with every chain's E-BFMI >= ``bfmi_min`` and the
    divergent fraction <= ``max_divergent`` (NaN: not converged).  Both default to None, report only: no threshold has been
    measured on this emulator (Stan warns below an E-BFMI of 0.3).  ``chhmc.h5`` and the chains are the same either way."""

    ADAPT_FILE = "chhmc_adapt.npz"

    def __init__(self, lnp, dlnp, ddlnp, ndim, nwalkers, x0=None, m=None, transform=None, torchspeed=False, seed=0,
                 dist_group=None, exchange=None):
        self.lnp, self.dlnp, self.ddlnp = lnp, dlnp, ddlnp
        self.exchange = exchange                             # how a multi-rank run splits the ensemble (_Ranks); None: automatic
        self.transform, self.x0, self.nparams, self.nwalkers = transform, x0, ndim, nwalkers
        self.m = np.ones(ndim) if m is None else m
        self.mass, self.cov = None, None
        self.sampler = None
        self.diagnostics = None                              # criterion="rhat": dict(rhat, ess, n) of the last check (+ rhat_rank's, ess_rank's)
        self.seed, self.group = seed, dist_group

    def sample(self, pool, nsamp, samp_steps=0, samp_eps=0, Madapt=1000, outdir="./", progress=False, overwrite=False,
               ntimes=10, tautol=0.01, method="emcee", incremental=True, meanshift=0.1, stdshift=0.1, nk=2, ncheck=100,
               burnin=100, profile=None, adapt_mass=False, adapt_traj=False, max_steps=64, criterion="tau", rhat_tol=1.01,
               ess_min=400, rhat_discard=0.0, rhat_rank=False, ess_rank=False, energy_stats=False, max_dH=1000.0, bfmi_min=None,
               max_divergent=None):
        hmc = method == "hmc"
        adapt_mass = self._check(self.lnp, method, samp_eps, Madapt, adapt_mass, adapt_traj, max_steps, criterion, rhat_tol, ess_min, rhat_discard, rhat_rank,
                                 ess_rank, energy_stats, max_dH, bfmi_min, max_divergent, world=ldist.world_size(self.group))
        filename = os.path.join(outdir, "chhmc.h5" if hmc else "chemcee_256.h5")       # sampler.py:466-469
        prof, rk, store, x0, resume, done, dchain = _open_run(self, "sampler.HMCSampler.sample", filename, overwrite, profile)
        if not rk.active:
            return store
        efile = os.path.join(outdir, _EnergyLog.FILE)
        if hmc and rk.rank == 0 and overwrite and os.path.exists(efile):
            os.remove(efile)
        # the warm-up's result next to the chain file (single-rank runs; written and read with adapt_mass or adapt_traj only,
        # removed with the chain)
        sidecar = os.path.join(outdir, self.ADAPT_FILE) if hmc and rk.real_world == 1 else None
        if sidecar and overwrite and os.path.exists(sidecar):
            os.remove(sidecar)
        ens = self.sampler = EnsembleSampler(rk.nw, self.nparams, self.lnp, seed=self.seed, dist_group=self.group, exchange=rk.exchange)
        print("start", flush=True)
        if not resume:
            print("burnin...", flush=True)                                   # sampler.py:519-529
            with prof.host("burnin"), _lib.stage("run_mcmc.burnin"):
                ens.set_state(rk.mine(x0))
                c, l = ens.run(burnin)
                c, l, _ = rk.gather(ens, c, l)
                if rk.rank == 0:
                    # the 50 nwalkers best burn-in samples, nwalkers of them drawn with numpy's generator as the reference
                    # does (sampler.py:524-528); ranked on the device, only the drawn rows come to the host (at 4096
                    # walkers the host's argsort of 409600 log-probabilities took as long as 400 iterations)
                    order = torch.argsort(l.reshape(-1), descending=True, stable=True)[:int(50 * self.nwalkers)]
                    pick = torch.as_tensor(np.random.randint(0, len(order), self.nwalkers), device=order.device)
                    x0 = c.reshape(-1, self.nparams)[order[pick]].cpu().numpy()
                x0 = rk.bcast(x0)
            print("burnin done...", flush=True)
            ens.naccept.zero_()
        if hmc:
            ens = self.sampler = self._hmc_chains(rk, x0, samp_steps, samp_eps, Madapt, prof, adapt_mass=adapt_mass,
                                                  sidecar=sidecar if adapt_mass or adapt_traj else None, resume=resume,
                                                  adapt_traj=bool(adapt_traj), max_steps=max_steps, stored=done,
                                                  max_dH=max_dH if energy_stats else None)
        else:
            ens.set_state(rk.mine(x0))
        rule = _RhatRule(dchain, self, rhat_tol, ess_min, rhat_discard, rhat_rank, ess_rank) if criterion == "rhat" else \
            _TauRule(dchain, ntimes, tautol, ncheck, nk, meanshift, stdshift)
        elog = _EnergyLog(self, ens, efile, bfmi_min, max_divergent, resume) if energy_stats else None
        self.diagnostics = None
        with _lib.stage("run_mcmc.blocks"):
            done = _run_blocks(ens, rk, store, dchain, done, nsamp, ncheck, incremental, rule, prof, elog)
        if elog is not None:
            elog.save()
        self.sampler = None
        return _close_run(prof, rk, store, dchain, done)

    @staticmethod
    def _check(lnp, method, samp_eps, Madapt, adapt_mass, adapt_traj, max_steps, criterion, rhat_tol, ess_min, rhat_discard, rhat_rank,
               ess_rank=False, energy_stats=False, max_dH=1000.0, bfmi_min=None, max_divergent=None, world=1):
        """``sample``'s arguments that exclude each other, before anything is built; returns ``BatchedHMC.adapt_mass_mode(adapt_mass)``.
        ``world``: the ranks of the run."""
        if method not in ("emcee", "hmc"):
            # sampler.py's "nuts" branch is unreachable in the reference and not built here
            raise NotImplementedError(method)
        hmc = method == "hmc"
        if energy_stats:
            if not hmc:
                raise ValueError("energy_stats with method = %r: divergences and E-BFMI are diagnostics of Hamiltonian "
                                 "trajectories; they belong to method=\"hmc\"" % (method,))
            if not float(max_dH) > 0.0:
                raise ValueError("energy_stats: max_dH = %r is not positive" % (max_dH,))
            if world > 1:
                raise ValueError("energy_stats=True in a multi-rank run (%d ranks): the energy diagnostics are single-rank only, the "
                                 "accumulators of the ranks are not gathered" % (world,))
        for name, v in (("bfmi_min", bfmi_min), ("max_divergent", max_divergent)):
            if v is not None and not (energy_stats and criterion == "rhat"):
                raise ValueError("%s = %r without %s: it gates the checks of criterion=\"rhat\" on the diagnostics of "
                                 "energy_stats=True" % (name, v, "energy_stats=True" if not energy_stats else "criterion=\"rhat\""))
        if criterion not in ("tau", "rhat"):
            raise ValueError("criterion = %r: \"tau\" (the reference's rule) or \"rhat\" (split-R-hat and multi-chain ESS)" % (criterion,))
        if criterion == "rhat":
            if not hmc:
                raise ValueError("criterion=\"rhat\" with method = %r: R-hat compares independent chains, and the walkers of an "
                                 "ensemble exchange positions at every move; it belongs to method=\"hmc\"" % (method,))
            if not (float(rhat_tol) > 1.0 and float(ess_min) > 0.0 and 0.0 <= float(rhat_discard) < 1.0):
                raise ValueError("criterion=\"rhat\": rhat_tol = %r (> 1), ess_min = %r (> 0), rhat_discard = %r (in [0, 1))"
                                 % (rhat_tol, ess_min, rhat_discard))
        elif rhat_rank:
            raise ValueError("rhat_rank = %r with criterion = %r: the rank-normalised, folded R-hat confirms the checks of "
                             "criterion=\"rhat\"" % (rhat_rank, criterion))
        elif ess_rank:
            raise ValueError("ess_rank = %r with criterion = %r: the rank-normalised bulk-ESS and tail-ESS confirm the checks of "
                             "criterion=\"rhat\"" % (ess_rank, criterion))
        adapt_mass = BatchedHMC.adapt_mass_mode(adapt_mass)
        if hmc and not getattr(lnp, "device_only", True):
            raise NotImplementedError("HMC needs the gradient of the log-probability: a user loglikelihoodfunc / "
                                      "externalloglike is host code without one")
        if hmc and adapt_mass and samp_eps:
            raise ValueError("adapt_mass with a fixed samp_eps = %r: the mass is adapted together with the step sizes "
                             "(samp_eps 0 or None)" % (samp_eps,))
        if adapt_traj:
            if not hmc:
                raise ValueError("adapt_traj with method = %r: the trajectory length belongs to method=\"hmc\"" % (method,))
            if samp_eps:
                raise ValueError("adapt_traj with a fixed samp_eps = %r: the trajectory length is adapted together with the "
                                 "step size (samp_eps 0 or None)" % (samp_eps,))
            if int(max_steps) < 1 or int(Madapt) < 1:
                raise ValueError("adapt_traj: max_steps = %r, Madapt = %r: both at least 1" % (max_steps, Madapt))
        return adapt_mass

    def _hmc_chains(self, rk, x0, samp_steps, samp_eps, Madapt, prof, adapt_mass=False, sidecar=None, resume=False,
                    adapt_traj=False, max_steps=64, stored=0, max_dH=None):
        """The chains of ``method="hmc"`` (sampler.py:491-493: ``HamiltonianMove(dlnp, samp_steps, samp_eps, m)``), one per
        walker of this rank, ready for ``_run_blocks``.  ``m`` is the move's ``cov``: momenta ~ N(0, m), drift p / m
        (``_hmc_matrix``, sampler.py:311-320; tests/golden/hmc_move.npz).  ``samp_eps`` > 0: that step size for every chain,
        the reference's semantics.  ``samp_eps`` 0 / None: a step size per chain from ``find_reasonable_epsilon`` and
        ``Madapt`` transitions of dual averaging (NUTSMove's scheme, sampler.py:198-240) plus the one on which that scheme
        puts the averaged step size in place -- none of them stored or counted; the convergence loop then runs on frozen
        step sizes.  ``samp_steps`` 0 means 5.  ``adapt_mass``: ``m`` is the starting mass of ``BatchedHMC.adapt``'s windowed
        scheme; ``sidecar`` (a file name): where its result is kept, and taken from in place of a warm-up when ``resume`` says
        the chain file was continued and the file holds ``ndim`` masses and one step size per walker.  ``adapt_traj``:
        ``BatchedHMC.adapt_traj`` behind that warm-up -- one step size for all chains and a trajectory length; ``samp_steps``
        is then not used, the file also holds ``traj``, ``max_steps`` and ``iteration`` (the Philox step of the first stored
        transition) and is taken only with a finite positive ``traj``; such a resumed run goes on at Philox step
        ``iteration + stored``, so that ``steps_for`` continues the sequence the first run began.  ``max_dH``: the chains
        count their energy diagnostics (``BatchedHMC.energy_stats``), emptied behind the warm-up."""
        if samp_eps is not None and samp_eps < 0:
            raise ValueError("samp_eps = %r: a step size is positive (0 or None: found and adapted per chain)" % (samp_eps,))
        adapt_mass = BatchedHMC.adapt_mass_mode(adapt_mass)
        m = np.asarray(self.m, np.float64)
        if m.shape not in ((self.nparams,), (self.nparams, self.nparams)):
            raise ValueError("HMC needs a mass m[ndim] (diagonal) or m[ndim][ndim] (dense)")
        if m.ndim == 2:
            BatchedHMC.chol_of_mass(m, self.nparams)           # (ValueError before anything is built)
            if adapt_mass == "diag":
                raise ValueError("adapt_mass = True with a dense m[ndim][ndim]: adapt_mass=\"dense\"")
        self.cov = None
        lib_seed = self.seed + 0x9E3779B97F4A7C15 * rk.rank & 0xFFFFFFFFFFFFFFFF       # (every rank its own momenta)
        ens = BatchedHMC(self.lnp, rk.mine(x0), mass=m, seed=lib_seed, dist_group=self.group)
        if not bool(torch.isfinite(ens.lnp).all()):
            raise ValueError("initial state has non-finite log-probability")
        ens.num_steps = int(samp_steps) if samp_steps else 5
        if max_dH is not None:
            ens.energy_stats(True, max_dH)
        if adapt_traj and samp_steps:
            print("samp_steps = %r is ignored: adapt_traj chooses the leapfrog steps of every transition" % (samp_steps,), flush=True)
        if samp_eps:
            if adapt_mass or adapt_traj:
                raise ValueError("adapt_mass / adapt_traj with a fixed samp_eps = %r" % (samp_eps,))
            ens.eps.fill_(float(samp_eps))
            self._keep_mass(ens, m)
            if ens.chol is None:
                self.mass = m.copy()
            return ens
        metric = "dense" if adapt_mass == "dense" or ens.chol is not None else "diag"
        kept = self._load_adaptation(sidecar, ens, metric, traj=adapt_traj) if resume and sidecar else None
        if kept is not None:
            if metric == "dense":
                ens._set_chol(kept["chol"])
            else:
                ens.mass.copy_(torch.as_tensor(kept["mass"], device=ens.dev))
            ens.eps.copy_(torch.as_tensor(kept["eps"], device=ens.dev))
            ens.epsbar.copy_(ens.eps)
            if adapt_traj:
                ens.set_traj(kept["traj"], kept["max_steps"])
                ens.iteration = kept["iteration"] + int(stored)
            print("hmc step sizes and mass from %s" % sidecar, flush=True)
        else:
            with prof.host("adapt"), _lib.stage("run_mcmc.hmc_adapt"):
                ens.adapt(int(Madapt), adapt_mass=adapt_mass, adapt_traj=adapt_traj, max_steps=max_steps)
                ens.naccept.zero_()
                ens.energy_reset()
        e = ens.eps.cpu().numpy()
        self._keep_mass(ens, m)
        mm = self.mass.astype(np.float32)
        extra = {}
        if ens.chol is not None:
            extra = dict(metric="dense", chol=ens.chol[0, :, :ens.ndim].cpu().numpy())
        if adapt_traj:
            extra.update(traj=np.float64(ens.traj), max_steps=np.int64(ens.max_steps), iteration=np.int64(ens.iteration))
            print("hmc trajectory length %.4g: %.4g step sizes, at most %d leapfrog steps"
                  % (ens.traj, ens.traj / ens._traj_eps, ens.max_steps), flush=True)
        if sidecar and kept is None:
            np.savez(sidecar, mass=mm, eps=e, num_steps=np.int64(ens.num_steps), Madapt=np.int64(Madapt), **extra)
        print("hmc step sizes %s: min %.3g median %.3g max %.3g; mass min %.3g median %.3g max %.3g%s"
              % ("after %d adaptive transitions" % Madapt if kept is None else "kept", e.min(), np.median(e), e.max(),
                 mm.min(), np.median(mm), mm.max(),
                 "" if self.cov is None else "; dense, condition number of C C^T %.3g" % np.linalg.cond(self.cov)), flush=True)
        return ens

    @staticmethod
    def rhat_rule(rhat, ess, rhat_tol=1.01, ess_min=400):
        """The stopping rule of ``criterion="rhat"``: every R-hat below ``rhat_tol`` and every ESS at least ``ess_min``.  A NaN
        in either compares false: "not converged" (not the tau rule's NaN stop)."""
        with np.errstate(invalid="ignore"):
            return bool(np.all(np.asarray(rhat) < rhat_tol) and np.all(np.asarray(ess) >= ess_min))

    def _keep_mass(self, ens, m):
        """``self.mass`` / ``self.cov`` of the chains as they run now (dense mode: C C^T and 1 / its diagonal)."""
        if ens.chol is not None:
            self.cov = ens.cov()
            self.mass = 1.0 / np.diag(self.cov)
        else:
            self.mass = ens.mass.cpu().numpy().astype(np.float64)

    @staticmethod
    def _load_adaptation(name, ens, metric="diag", traj=False):
        """{mass, eps} (``metric`` "dense": and chol) of ``chhmc_adapt.npz`` if it is there, holds that metric (a file
        without the word is diagonal) and fits these chains, else None.  ``traj``: and {traj, max_steps, iteration}, None
        unless the file holds a finite positive trajectory length."""
        if not os.path.exists(name):
            return None
        with np.load(name) as f:
            if not {"mass", "eps"} <= set(f.files):
                return None
            if (str(f["metric"]) if "metric" in f.files else "diag") != metric:
                return None
            mass, eps = np.asarray(f["mass"], np.float32), np.asarray(f["eps"], np.float32)
            chol = np.asarray(f["chol"], np.float32) if metric == "dense" and "chol" in f.files else None
            tr = None
            if traj:
                if not {"traj", "max_steps"} <= set(f.files):
                    return None
                tr = dict(traj=float(f["traj"]), max_steps=int(f["max_steps"]), iteration=int(f["iteration"]) if "iteration" in f.files else 0)
                if not (np.isfinite(tr["traj"]) and tr["traj"] > 0 and tr["max_steps"] >= 1 and tr["iteration"] >= 0):
                    return None
        ok = mass.shape == (ens.ndim,) and eps.shape == (ens.B,) and np.isfinite(mass).all() and (mass > 0).all() \
            and np.isfinite(eps).all() and (eps > 0).all()
        if metric == "dense":
            ok = ok and chol is not None and chol.shape == (ens.ndim, ens.ndim) and bool(np.isfinite(chol).all()) \
                and bool((np.diag(chol) > 0).all())
            return dict(mass=mass, eps=eps, chol=chol, **(tr or {})) if ok else None
        return dict(mass=mass, eps=eps, **(tr or {})) if ok else None


class ZeusSampler(object):
    """sampler.py:699-737: zeus' ensemble slice sampler (``SliceEnsembleSampler``) with the reference's
    convergence callback (IAT on the last 80 %, sampler.py:684,729; mean/std drift) and file names.
    Multi-rank runs give every rank a sub-ensemble with a mu of its own and gather the chain once per convergence check
    (``_Ranks``); every rank of the run must make the call (``dist.enter``)."""

    def __init__(self, lnp, ndim, nwalkers, x0=None, transform=None, seed=0, dist_group=None, exchange=None):
        self.lnp, self.transform, self.x0, self.nparams, self.nwalkers = lnp, transform, x0, ndim, nwalkers
        self.sampler = None
        self.seed, self.group = seed, dist_group
        self.exchange = exchange                             # how a multi-rank run splits the ensemble (_Ranks); None: automatic

    def sample(self, pool, nsamp, outdir="./", progress=False, overwrite=False, ntimes=10, tautol=0.01, incremental=True,
               meanshift=0.1, stdshift=0.1, nk=2, ncheck=100, profile=None):
        prof, rk, store, x0, _, done, dchain = _open_run(self, "sampler.ZeusSampler.sample", os.path.join(outdir, "zeus_256.h5"), overwrite, profile)
        if not rk.active:
            return store
        ens = self.sampler = SliceEnsembleSampler(rk.nw, self.nparams, self.lnp, seed=self.seed, dist_group=self.group, exchange=rk.exchange)
        ens.set_state(rk.mine(x0))
        with _lib.stage("run_mcmc.blocks"):
            done = _run_blocks(ens, rk, store, dchain, done, min(nsamp, 100000), ncheck, incremental,
                               _ZeusRule(dchain, ntimes, tautol, ncheck, nk, meanshift, stdshift), prof)
        return _close_run(prof, rk, store, dchain, done)
