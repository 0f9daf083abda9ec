"""The two ensemble samplers on the device: stretch move and zeus' slice move (linna_amd.sampler re-exports them)."""
import ctypes as C

import numpy as np
import torch

from . import _lib, dist as ldist


class EnsembleSampler(object):
    """Affine-invariant ensemble sampler with every walker evaluated in one batched GPU call.

    ``log_prob`` is a ``linna_amd.util.Log_prob`` (device pipeline).  ``nwalkers`` is the number
    of walkers OWNED BY THIS RANK; with ``exchange='allgather'`` and a process group the
    complementary set of a half step is drawn from the walkers of all ranks (one all-gather of
    ``[nwalkers, ndim]`` per half step), otherwise ranks run independent sub-ensembles and only
    chain state is gathered.
    """

    def __init__(self, nwalkers, ndim, log_prob, a=2.0, seed=0, randomize_split=True, dist_group=None,
                 exchange="none", fused=True):
        self.nw, self.ndim, self.lp, self.a, self.seed = int(nwalkers), int(ndim), log_prob, float(a), int(seed)
        if self.nw < 2 or self.nw % 2:
            raise ValueError("need an even number of walkers >= 2")
        self.randomize_split = randomize_split
        self.group, self.exchange = dist_group, exchange
        self.fused = None if fused else False        # None: try linna_stretch_half_step on the first half step
        # a user loglikelihoodfunc / externalloglike is host code: proposals and the Metropolis test stay kernels,
        # the log-probability of a half ensemble goes through Log_prob.evaluate_any (emulator on the GPU + callbacks)
        self.host_lp = not getattr(log_prob, "device_only", True)
        if self.host_lp:
            self.fused = False
        p = log_prob._ensure()
        self.dev = p["dev"]
        self.ctx = _lib.ctx(self.dev.index)
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=self.dev)
        self.ld = _lib.ld4(self.ndim)
        self.coords, self.logp = z(self.nw, self.ld), z(self.nw)
        self.half = self.nw // 2
        self.Q, self.factors, self.lp_new = z(self.half, self.ld), z(self.half), z(self.half)
        self.naccept = torch.zeros(self.nw, dtype=torch.int32, device=self.dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.iteration = 0
        self._dev_steps = 0                          # value of the device step counter (== iteration unless fused)
        self._rs = np.random.RandomState(self.seed ^ 0x5EED)
        self._split_pos, self._split_host, self._split_dev, self._split_evt = 0, None, None, None
        self._split, self._draws, self._split_idx = None, 0, np.arange(self.nw)
        self.block_run = None                        # None: try linna_stretch_run (a whole block of iterations per C call)
        self.rank, self.world = ldist.rank(dist_group), ldist.world_size(dist_group)
        self._gathered = None

    # -- state
    def set_state(self, x0):
        x0 = torch.as_tensor(np.asarray(x0, np.float32), device=self.dev)
        if x0.shape != (self.nw, self.ndim):
            raise ValueError("x0 must be [nwalkers, ndim]")
        self.coords.zero_()
        self.coords[:, :self.ndim].copy_(x0)
        self._lnp(self.coords, self.logp)
        if not bool(torch.isfinite(self.logp).all()):
            raise ValueError("initial state has non-finite log-probability")   # emcee raises the same way

    def _lnp(self, X, out):
        """lnP of the rows of ``X[B, ld]`` into ``out[B]``."""
        if self.host_lp:
            out.copy_(self.lp.evaluate_any(X))
        else:
            self.lp.evaluate(X, out=out)

    _SPLIT_CHUNK = 64

    def _draw_splits(self, n):
        """Device int32 [n, 2, nw/2]: the random equal splits of the next ``n`` iterations (== the shuffled ``arange % 2``
        of emcee's RedBlueMove), drawn on the host in one go and shipped in ONE asynchronous copy from pinned memory (a
        per-iteration blocking copy left the GPU idle for ~25 us of every 150 us iteration)."""
        slot = self._draws & 1
        self._draws += 1
        if self._split_host is None:
            self._split_host, self._split_evt = [None, None], [None, None]
        if self._split_evt[slot] is not None:
            self._split_evt[slot].synchronize()                 # the copy that last read this pinned buffer is done
        if self._split_host[slot] is None or len(self._split_host[slot]) < n:
            self._split_host[slot] = torch.empty((max(n, self._SPLIT_CHUNK), 2, self.half), dtype=torch.int32).pin_memory()
        host = self._split_host[slot].numpy()
        idx = self._split_idx
        for i in range(n):
            self._rs.shuffle(idx)
            host[i] = idx.reshape(2, self.half)
        dev = torch.empty((n, 2, self.half), dtype=torch.int32, device=self.dev)
        dev.copy_(self._split_host[slot][:n], non_blocking=True)
        self._split_evt[slot] = torch.cuda.Event()
        self._split_evt[slot].record()
        return dev

    def _splits(self):
        """This iteration's split, device int32 [2, nw/2] (drawn 64 iterations at a time)."""
        if not self.randomize_split:
            if self._split is None:
                self._split = torch.as_tensor(np.arange(self.nw, dtype=np.int32).reshape(2, self.half), device=self.dev)
            return self._split
        if self._split_dev is None or self._split_pos >= len(self._split_dev):
            self._split_dev, self._split_pos = self._draw_splits(self._SPLIT_CHUNK), 0
        halves = self._split_dev[self._split_pos]
        self._split_pos += 1
        return halves

    def _splits_block(self, n):
        """The splits of the next ``n`` iterations as one device tensor [n, 2, nw/2] (what is left of the chunk `_splits`
        was handing out first: both routes consume the same sequence of permutations)."""
        rem = None
        if self._split_dev is not None and self._split_pos < len(self._split_dev):
            rem = self._split_dev[self._split_pos:self._split_pos + n]
            self._split_pos += len(rem)
            if len(rem) == n:
                return rem
        new = self._draw_splits(n - (0 if rem is None else len(rem)))
        return new if rem is None else torch.cat([rem, new])

    @property
    def lib_seed(self):
        """The Philox key of this rank's moves (every rank its own draws)."""
        return C.c_uint64(self.seed + 0x9E3779B97F4A7C15 * (self.rank + 1) & 0xFFFFFFFFFFFFFFFF)

    def step(self):
        """One ensemble iteration (both halves).  Everything is enqueued on the current stream."""
        st = _lib.stream()
        halves = self._splits()
        lib_seed = self.lib_seed
        for h in (0, 1):
            S, Cc = halves[h], halves[1 - h]
            comp, ldc, cidx, nc = self._complement(Cc)
            if self.fused is not False:
                # propose + log-probability + accept in ONE launch (bit-identical to the three below)
                rc = _lib.load().linna_stretch_half_step(
                    self.lp._ensure()["handle"], _lib.ptr(self.coords), self.ld, self.ndim, _lib.ptr(self.logp),
                    _lib.iptr(S), self.half, _lib.ptr(comp), ldc, _lib.iptr(cidx), nc, lib_seed,
                    _lib.iptr(self.step_dev), self.iteration - self._dev_steps, h, self.a, _lib.iptr(self.naccept), st)
                if rc == 0:
                    self.fused = True
                    continue
                if rc != _lib.ERR_UNSUPPORTED or self.fused is True:
                    _lib.check(rc)
                self.fused = False                   # this log-probability cannot: three launches from now on
            _lib.call("linna_stretch_propose", self.ctx, _lib.ptr(self.coords), self.ld, self.ndim, _lib.iptr(S), self.half,
                      _lib.ptr(comp), ldc, _lib.iptr(cidx), nc, lib_seed, _lib.iptr(self.step_dev), h, self.a,
                      _lib.ptr(self.Q), self.ld, _lib.ptr(self.factors), st)
            self._lnp(self.Q, self.lp_new)
            _lib.call("linna_stretch_accept", self.ctx, _lib.ptr(self.coords), self.ld, self.ndim, _lib.ptr(self.logp),
                      _lib.iptr(S), self.half, _lib.ptr(self.Q), self.ld, _lib.ptr(self.lp_new), _lib.ptr(self.factors),
                      lib_seed, _lib.iptr(self.step_dev), h, _lib.iptr(self.naccept), st)
        if self.fused is not True:                   # the fused entry takes the iteration as an offset instead
            _lib.call("linna_step_increment", self.ctx, _lib.iptr(self.step_dev), st)
            self._dev_steps += 1
        self.iteration += 1

    def _complement(self, Cc):
        """The complementary set of a half step as (coords, row stride, device indices, count): this rank's other half, or
        with ``exchange="allgather"`` over several ranks the other halves of all of them."""
        if self.exchange == "allgather" and self.world > 1:
            comp, cidx, nc = self._allgather_complement(Cc)
            return comp, self.ld, cidx, nc
        return self.coords, self.ld, Cc, self.half

    def _allgather_complement(self, Cc):
        """Complementary walkers of ALL ranks: gather this rank's complementary half."""
        gathered = ldist.gather_rows(self.coords[Cc.long()], self.group)
        if self._gathered is None:
            self._gidx = torch.arange(gathered.shape[0], dtype=torch.int32, device=self.dev)
        self._gathered = gathered
        return gathered, self._gidx, gathered.shape[0]

    def run(self, nsteps, store=True):
        """Advance ``nsteps``; returns (chain[nsteps, nw, ndim], logp[nsteps, nw]) as device tensors.  One rank, fused half
        steps: ONE C call enqueues the whole block (linna_stretch_run: 2 launches per iteration whose finish also writes the
        chain rows -- the per-iteration host work of the loop below, two ctypes calls and two device copies, cost as much
        as the 60 us an iteration of 128 walkers takes on the GPU); bit-identical to that loop."""
        chain = torch.empty((nsteps, self.nw, self.ndim), dtype=torch.float32, device=self.dev) if store else None
        lps = torch.empty((nsteps, self.nw), dtype=torch.float32, device=self.dev) if store else None
        if (nsteps > 0 and self.block_run is not False and self.fused is not False and type(self).step is EnsembleSampler.step
                and not (self.exchange == "allgather" and self.world > 1)):
            # the splits are host draws (41 us each at 4096 walkers): big ensembles go out in pieces of a few iterations, so
            # that the GPU starts on the first piece while the host shuffles the next
            piece = nsteps if not self.randomize_split else max(8, min(nsteps, 65536 // self.nw))
            lib_seed = self.lib_seed
            i0 = 0
            while i0 < nsteps:
                n = min(piece, nsteps - i0)
                if self.randomize_split:
                    sp, stride = self._splits_block(n), self.nw
                else:
                    sp, stride = self._splits(), 0
                rc = _lib.load().linna_stretch_run(
                    self.lp._ensure()["handle"], _lib.ptr(self.coords), self.ld, self.ndim, _lib.ptr(self.logp), self.nw, _lib.iptr(sp),
                    stride, n, lib_seed, _lib.iptr(self.step_dev), self.iteration - self._dev_steps, self.a, _lib.iptr(self.naccept),
                    _lib.ptr(chain[i0:]) if store else None, _lib.ptr(lps[i0:]) if store else None, _lib.stream())
                if rc != 0:
                    break
                self.block_run = self.fused = True
                self.iteration += n
                i0 += n
            if i0 == nsteps:
                return chain, lps
            if rc != _lib.ERR_UNSUPPORTED or self.block_run is True:
                _lib.check(rc)
            self.block_run = False
            if self.randomize_split:                 # hand the drawn splits back to the per-iteration route
                self._split_dev, self._split_pos = sp, 0
        for i in range(nsteps):
            self.step()
            if store:
                chain[i].copy_(self.coords[:, :self.ndim])
                lps[i].copy_(self.logp)
        return chain, lps

    def theta_of(self, z):
        """Physical parameters of latent points ``z[..., ndim]`` (device), via the prior-map kernel."""
        p = self.lp._ensure()
        flat = z.reshape(-1, self.ndim).contiguous()
        n = flat.shape[0]
        th = torch.empty_like(flat)
        x = torch.empty((n, self.ld), dtype=torch.float32, device=self.dev)
        k, d = p["keep"], p["desc"]
        _lib.call("linna_prior_map_fwd", self.ctx, _lib.ptr(flat), self.ndim, n, self.ndim, _lib.iptr(k["is_flat"]),
                  _lib.ptr(k["a1"]), _lib.ptr(k["a2"]), None, _lib.ptr(k["xmean"]), _lib.ptr(k["xstd"]), _lib.ptr(x), self.ld,
                  _lib.ptr(th), self.ndim, _lib.stream())
        return th.reshape(z.shape)

    def gather_chain(self, chain, lps):
        """RCCL all-gather of this rank's chain block: [nsteps, world*nw, ndim] on every rank."""
        return ldist.gather_chain(chain, lps, self.group)


# ------------------------------------------------------------------ ensemble slice sampling (zeus)
class _FastOverflow(Exception):
    """A walker of the one-call slice half step needed more rounds than the call holds (SliceEnsembleSampler._guard)."""


class SliceEnsembleSampler(EnsembleSampler):
    """zeus' ensemble slice sampler (Karamanis & Beutler 2021; driven by sampler.py:728-735) with
    every trial point of a half ensemble evaluated in one batched GPU call.

    Per half step: differential-move directions ``mu (c_a - c_b)``, slice height
    ``Z0 = logp + log u``, stepping out (both bracket ends evaluated together, 2 x nw/2 points per
    round) and shrinking (nw/2 points per round) until every walker has accepted.  ``mu`` is tuned
    during the first iterations as zeus does: ``mu *= 2 nexp / (nexp + ncon)`` until the expansion
    fraction stays within ``tolerance`` of 1/2 for ``patience`` iterations.  Third-party algorithm
    restated from the publication (zeus-mcmc is not in the reference tree): parity unpinned; every half step is replayed
    decision by decision against ``oracle.sampling.slice_half_step`` (tests/test_gpu_slice_replay.py) and the posterior is
    checked statistically.  ``mu`` has zeus' meaning (direction ``2 mu (c_a - c_b)``), ``maxsteps`` is zeus' stepping-out
    budget (``J = floor(maxsteps u)`` steps to the left at most, ``maxsteps - 1 - J`` to the right).
    """

    FAST_EXPANSIONS = 12            # at least so many per side and half step on the one-call path (a tuned mu needs about one)
    FAST_TRIALS = 32                # at least so many shrinking trials per walker and half step (each halves the bracket)
    FAST_FIRST = None               # bracket ends per side in the first stepping-out round (None: by ensemble size, below)
    FAST_CAP = (8, 32)              # most ends per side / trials a later round looks ahead
    MAX_ENDS, MAX_TRIALS = 32, 64   # most a round may hold: a wave's lanes in the logic kernels (linna_slice_half_step rejects more)

    def __init__(self, nwalkers, ndim, log_prob, mu=1.0, seed=0, tune=True, tolerance=0.05, patience=5, maxsteps=10000,
                 maxiter=100000, dist_group=None, exchange="none", fast=None):
        EnsembleSampler.__init__(self, nwalkers, ndim, log_prob, seed=seed, dist_group=dist_group, exchange=exchange)
        z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=self.dev)
        ns = self.half
        self.mu = float(mu)
        # zeus' direction is 2 mu (c_a - c_b) (moves.DifferentialMove.get_direction); the kernels multiply by mu_dev[0]
        self.mu_dev = torch.full((1,), 2.0 * self.mu, dtype=torch.float32, device=self.dev)
        self.tune, self.tolerance, self.patience, self.maxsteps, self.maxiter = tune, tolerance, patience, maxsteps, maxiter
        self._tune_count = 0
        self.DIR, self.Q2 = z(ns, self.ld), z(2 * ns, self.ld)
        self.Z0, self.Wacc, self.Zacc = z(ns), z(ns), z(ns)
        self.LR = z(2 * ns)                              # bracket ends, contiguous: both evaluated in one launch
        self.L, self.R = self.LR[:ns], self.LR[ns:]
        self.fused_points = None                         # None: try linna_logprob_eval_slice_points first
        self.ntrial = 2                                  # shrink trials per round (2 x nw/2 points = one full launch)
        self.W = z(self.ntrial * ns)
        self.Z2 = z(2 * ns)
        self.flags = torch.zeros(3 * ns, dtype=torch.int32, device=self.dev)
        self.counters = torch.zeros(4, dtype=torch.int32, device=self.dev)   # expansions, contractions, active (ping-pong)
        self._neval_host = 0
        self._cs, self._pin = None, None
        # One C call per half step (linna_slice_half_step) once mu is tuned: speculative rounds -- `m` bracket ends per side
        # per stepping-out round, `nt` trials per shrinking round -- and a fixed number of rounds, gated off on the device
        # behind the one that finished the last walker.  The host then never waits inside an iteration (with 4-128 walkers
        # the round-by-round loop below was bound by its own launches and count read-backs, not by the GPU).  The first
        # round of each kind evaluates every walker and is sized by the ensemble (a launch of up to ~2000 points costs what
        # one point costs; beyond ~4000 the evaluation is compute bound at 14 ns a point); the later rounds evaluate only
        # the walkers still active, so they look twice as far ahead each time for next to nothing and few rounds cover
        # FAST_EXPANSIONS stepping-out steps per side and FAST_TRIALS shrinking trials.  A walker that needs more is
        # counted (and kept in place), and `run` / `step` then take the sampler back to the state they started from and
        # redo their iterations on the unbounded round loop: the chain is always the round loop's.
        self.fast = fast
        self._fast_ok = None                              # None: try the entry on the first tuned iteration
        first = self.FAST_FIRST or (8 if ns <= 64 else 4 if ns <= 256 else 2 if ns <= 2048 else 1)   # measured: tools/slice_probe.py
        if self.FAST_FIRST is None and ns <= 64:
            # small ensembles (the reference's 128 walkers): every round costs ~30 us of launches whatever it evaluates, and the
            # usage counters (linna_slice_half_step, `round_usage`) show nothing left behind 8 bracket ends per side or behind 16
            # trials in 58 000 walker half steps (R5, tools/slice_probe.py): ONE stepping-out round of 8, the second shrinking
            # round kept as the rescue (16 + 16 trials); a walker beyond that sends the run to the round loop as before
            self.set_schedule([8], [16, 16])
        else:
            self.set_schedule(self._schedule(first, self.FAST_EXPANSIONS, self.FAST_CAP[0]),
                              self._schedule(2 * first, self.FAST_TRIALS, self.FAST_CAP[1]))
        self._last_nexp = None                            # expansions of the last tuning iteration (whole ensemble)
        self._fast_after = 0                              # no one-call steps before this iteration (set after an overflow)
        self._guarded = False
        self.noverflow = 0                                # runs redone on the round loop
        # test hook: called behind every half step with (half index, S, dict of the device arrays Z0 / L / R / Wacc / Zacc of the
        # half ensemble) -- tests/test_gpu_slice_replay.py replays each half step against oracle.sampling.slice_half_step
        self.probe = None

    def set_schedule(self, m_sched, nt_sched):
        """Bracket ends per side of each stepping-out round and trials of each shrinking round of the one-call path."""
        self.m_sched, self.nt_sched = self.check_schedule(m_sched, nt_sched)
        self.m, self.nt_fast = max(self.m_sched), max(self.nt_sched)         # (scratch sizes)
        self._expect, self._expect_base, self._expect_seen, self.expected_rows = None, (0.0, np.zeros(0)), -1, None
        self.nexp_rounds, self.nshr_rounds = len(self.m_sched), len(self.nt_sched)
        self._m_arr = (C.c_int * self.nexp_rounds)(*self.m_sched)
        self._nt_arr = (C.c_int * self.nshr_rounds)(*self.nt_sched)
        if getattr(self, "_fast_bufs", None) is not None:              # (a schedule change mid-run: keep the evaluation count)
            self._neval_host += int(self._fast_bufs["counters"][3].item())
        self._fast_bufs = None

    @staticmethod
    def check_schedule(m_sched, nt_sched):
        """The two schedules as lists of ints; ValueError for a round linna_slice_half_step would reject."""
        m_sched, nt_sched = [int(v) for v in m_sched], [int(v) for v in nt_sched]
        for name, sched, cap in (("m_sched", m_sched, SliceEnsembleSampler.MAX_ENDS), ("nt_sched", nt_sched, SliceEnsembleSampler.MAX_TRIALS)):
            if not sched or min(sched) < 1 or max(sched) > cap:
                raise ValueError("%s = %s: every round needs 1 to %d" % (name, sched, cap))
        return m_sched, nt_sched

    @staticmethod
    def _schedule(first, total, cap):
        """first, 2 first, 4 first ... (at most `cap` each) until at least `total` are covered; two rounds at least."""
        out = [min(first, cap)]
        while sum(out) < total or len(out) < 2:
            out.append(min(2 * out[-1], cap))
        return out

    # -- data-dependent rounds with one round of lookahead ------------------------------------------
    # A round = a few small kernels + one evaluation + a kernel that counts the walkers still active.
    # Reading that count on the host every round left the GPU idle while the host came back and queued
    # the next round (~35 us of every ~110 us).  Instead round r+1 is queued BEFORE the count of round r
    # is known: its evaluation is gated on the device-side count (linna_logprob_eval_if), so when round
    # r turns out to have been the last, round r+1 costs a few empty launches.  The count travels over
    # a second stream into pinned memory, so waiting for it does not wait for round r+1.
    def _run_rounds(self, enqueue, maxrounds, what="expansions"):
        if self._cs is None:
            self._cs = torch.cuda.Stream(device=self.dev)
            self._pin = torch.zeros(2, dtype=torch.int32).pin_memory()
        main = torch.cuda.current_stream(self.dev)
        pending = None
        for r in range(maxrounds):
            slot = 2 + (r & 1)
            self.counters[slot:slot + 1].zero_()
            gate = C.c_void_p(self.counters.data_ptr() + 4 * (2 + ((r - 1) & 1))) if r > 0 else None
            enqueue(r, slot, gate)
            done = torch.cuda.Event()
            done.record(main)
            with torch.cuda.stream(self._cs):
                self._cs.wait_event(done)
                self._pin[r & 1:(r & 1) + 1].copy_(self.counters[slot:slot + 1], non_blocking=True)
                landed = torch.cuda.Event()
                landed.record(self._cs)
            if pending is not None:
                pending[0].synchronize()
                if int(self._pin[pending[1]]) == 0:
                    return                              # round r-1 finished every walker; round r (queued) is gated off
            pending = (landed, r & 1)
        pending[0].synchronize()
        if int(self._pin[pending[1]]) != 0:              # zeus: RuntimeError behind `maxiter` passes (sampler.py:728: maxiter=1E5)
            raise RuntimeError("Number of %s exceeded maximum limit! Make sure that the pdf is well-defined." % what)

    def _eval_if(self, Q, Z, gate):
        if self.host_lp:                                # host callbacks: evaluated whatever the gate says (results of a
            Z.copy_(self.lp.evaluate_any(Q))            # gated-off round are never used)
            return
        p = self.lp._ensure()
        B = Q.shape[0]
        _lib.call("linna_logprob_eval_if", p["handle"], _lib.ptr(Q), Q.stride(0), B, _lib.ptr(self.lp._workspace(B, False)),
                  _lib.ptr(Z), None, 0, gate, _lib.stream())

    def _eval_points(self, S, w, nrep, gate):
        """lnP at coords[S[k]] + w[j*ns + k] DIR[k] into Z2[:nrep*ns]: one launch that never writes the points when
        the whole-network kernel serves this log-probability, else linna_slice_points + the gated evaluation."""
        ns, st, P = self.half, _lib.stream(), _lib.ptr
        if self.host_lp:
            self.fused_points = False
        if self.fused_points is not False:
            rc = _lib.load().linna_logprob_eval_slice_points(
                self.lp._ensure()["handle"], P(self.coords), self.ld, self.ndim, _lib.iptr(S), ns, P(self.DIR), self.ld,
                P(w), nrep, P(self.Z2), gate, st)
            if rc == 0:
                self.fused_points = True
                return
            if rc != _lib.ERR_UNSUPPORTED or self.fused_points is True:
                _lib.check(rc)
            self.fused_points = False
        _lib.call("linna_slice_points", self.ctx, P(self.coords), self.ld, self.ndim, _lib.iptr(S), ns, P(self.DIR), self.ld,
                  P(w), P(self.Q2), self.ld, nrep, st)
        self._eval_if(self.Q2[:nrep * ns], self.Z2[:nrep * ns], gate)

    @property
    def neval(self):
        """Log-probability evaluations so far (points, both paths; reads a device counter)."""
        dev = int(self._fast_bufs["counters"][3].item()) if self._fast_bufs is not None else 0
        return self._neval_host + dev

    def round_usage(self):
        """How much of the one-call path's look-ahead the run has used: for every stepping-out and shrinking round, the mean
        fraction of a half ensemble's walkers still active BEHIND it (device counters of linna_slice_half_step; one read)."""
        if self._fast_bufs is None:
            return None
        nr = self.nexp_rounds + self.nshr_rounds
        c = self._fast_bufs["counters"].cpu().numpy().astype(np.float64)
        calls = c[4 + 2 * nr] - 1                       # (the counts of the latest call are added by the next one)
        if calls < 1:
            return None
        frac = c[4 + nr:4 + 2 * nr] / (calls * self.half)
        return {"half_steps": int(calls), "active_after_expand_round": frac[:self.nexp_rounds].tolist(),
                "active_after_shrink_round": frac[self.nexp_rounds:].tolist()}

    def _use_fast(self):
        """The one-call half step serves every ensemble size (measured: 4.8x the round loop at 128 walkers, 1.3x at 4096).
        While mu is still being tuned it is used only once an iteration has needed few expansions: the walkers of a run
        start in a 1e-3 ball (util.py:937) and the first iterations step out hundreds of times per side, which the
        unbounded round loop handles and the fixed rounds of the one-call path would not."""
        if self.fast is False or self.host_lp or self._fast_ok is False or self.iteration < self._fast_after:
            return False
        # (_last_nexp counts the WHOLE ensemble's expansions when the walkers are sharded over ranks, see _tune_mu)
        if self.tune and not (self._last_nexp is not None and self._last_nexp < 2.0 * self.nw * (self.world if self._shared() else 1)):
            return False
        return True

    def _step_fast(self, halves, seed):
        """Both half steps through linna_slice_half_step; False when the entry does not serve this log-probability."""
        ns, P, I = self.half, _lib.ptr, _lib.iptr
        if self._fast_bufs is None:
            z = lambda *sh: torch.zeros(sh, dtype=torch.float32, device=self.dev)
            nrep = max(2 * self.m, self.nt_fast)
            self._fast_bufs = dict(state=z(5 * ns), W=z(2 * self.m * ns), Wd=z(self.nt_fast * ns), Zt=z(nrep * ns),
                                   list=torch.zeros(nrep * ns, dtype=torch.int32, device=self.dev),
                                   counters=torch.zeros(5 + 2 * (self.nexp_rounds + self.nshr_rounds), dtype=torch.int32, device=self.dev))
        b, st = self._fast_bufs, _lib.stream()
        self._refresh_expectation()
        for h in (0, 1):
            S, Cc = halves[h], halves[1 - h]
            comp, ldc, cidx, nc = self._complement(Cc)
            rc = _lib.load().linna_slice_half_step(
                self.lp._ensure()["handle"], P(self.coords), self.ld, self.ndim, P(self.logp), I(S), ns, P(comp), ldc, I(cidx), nc,
                P(self.mu_dev), seed, I(self.step_dev), h, self._m_arr, self.nexp_rounds, self._nt_arr, self.nshr_rounds, P(self.DIR), self.ld,
                P(b["state"]), I(self.flags), P(b["W"]), P(b["Wd"]), P(b["Zt"]), I(b["list"]), I(b["counters"]), 1 if h == 0 else 0,
                1 if h == 1 else 0, self._expect, int(self.maxsteps), st)    # (the second half step's last kernel advances the device step counter)
            if rc != 0:
                if rc == _lib.ERR_UNSUPPORTED and h == 0 and self._fast_ok is None:
                    self._fast_ok = False
                    return False
                _lib.check(rc)
            if self.probe is not None:
                s5 = b["state"]
                self.probe(h, S, dict(Z0=s5[:ns], L=s5[ns:2 * ns], R=s5[2 * ns:3 * ns], Wacc=s5[3 * ns:4 * ns], Zacc=s5[4 * ns:],
                                      counters=b["counters"], fast=True))
        self._fast_ok = True
        self.iteration += 1
        self._fast_steps = getattr(self, "_fast_steps", 0) + 1
        if self.tune:
            c = b["counters"][:3].cpu().numpy()          # one read per iteration while mu is tuned, as the round loop
            if c[2]:
                if self._shared():
                    self._overflow_seen = True       # (ranks exchange walkers every half step: no rank may leave the loop alone)
                else:
                    raise _FastOverflow()
            self._tune_mu(int(c[0]), int(c[1]))
        return True

    EXPECT_AT = (16, 64, 256)       # one-call iterations after which the usage counters are read (then every 1024)
    USE_EXPECT = True               # (False: the later rounds' engines by the fixed rule, a quarter of the previous round's -- A/B)

    def _refresh_expectation(self):
        """The rounds after the first evaluate only the walkers still active; their launch is sized for all but runs the
        engine (4 / 8 / 16 rows per workgroup) that suits the EXPECTED number of trial points -- 60 points cost 56 us on the
        16-row engine and 29 on the 4-row one.  The expectation is what the usage counters have shown since the last look
        (mean active fraction behind each round x the next round's points per walker x 1.25 + 8; a round that has
        practically never run gets the 16-row engine, whose launch has the fewest workgroups to dismiss), read at fixed iteration
        counts so that a run is reproducible: 16, 64, 256, then every 1024 one-call iterations (one small device read each)."""
        n = getattr(self, "_fast_steps", 0)
        if not self.USE_EXPECT:
            return
        if not (n in self.EXPECT_AT or (n and n % 1024 == 0)) or n == getattr(self, "_expect_seen", -1):
            return
        self._expect_seen = n
        nr = self.nexp_rounds + self.nshr_rounds
        rows, base = self.expected_points(self._fast_bufs["counters"].cpu().numpy(), self.m_sched, self.nt_sched, self.half, self._expect_base)
        if rows is None:
            return
        self._expect_base = base
        self._expect = (C.c_int * nr)(*rows)
        self.expected_rows = rows

    @staticmethod
    def expected_points(counters, m_sched, nt_sched, half, base=None):
        """From the usage counters of linna_slice_half_step (include/linna_hip.h: ``[4 + nr + r]`` walkers still active behind
        round r summed over the earlier calls, ``[4 + 2 nr]`` the calls) and the counters' state at the last look
        (``base`` = (calls, sums)): the trial points each round is expected to evaluate -- entry r of the stepping-out rounds,
        ``len(m_sched) + r`` of the shrinking ones; 1 for the first round of each kind (it evaluates every walker), 2^20 for a
        round whose mean is below half a point -- and the new ``base``.  (None, base) when fewer than 8 calls are new."""
        nexp, nr = len(m_sched), len(m_sched) + len(nt_sched)
        c = np.asarray(counters, np.float64)
        calls, cum = c[4 + 2 * nr] - 1, c[4 + nr:4 + 2 * nr]
        last_calls, last_cum = base if base is not None and len(base[1]) == nr else (0.0, np.zeros(nr))
        if calls - last_calls < 8:
            return None, base
        frac = (cum - last_cum) / ((calls - last_calls) * half)
        pts = [2 * m for m in m_sched] + list(nt_sched)
        rows = [1] * nr
        for i in range(nr):
            if i and i != nexp:
                mean = pts[i] * frac[i - 1] * half
                # (a round that practically never runs: the engine with the fewest workgroups to launch and dismiss)
                rows[i] = int(mean * 1.25) + 8 if mean >= 0.5 else 1 << 20
        return rows, (calls, cum.copy())

    def _tune_mu(self, nexp, ncon):
        """zeus: mu *= 2 nexp / (nexp + ncon) until the expansion fraction stays within ``tolerance`` of 1/2 for
        ``patience`` iterations.  One ensemble sharded over ranks tunes ONE mu from the WHOLE ensemble's counts (zeus and
        the reference do: sampler.py:728-735): the two counts are summed over the ranks first, so every rank carries the
        same mu, leaves tuning at the same iteration and the chain is comparable to the single-rank one."""
        if self._shared():
            t = torch.tensor([float(nexp), float(ncon)], dtype=torch.float32, device=self.mu_dev.device)
            ldist.allreduce_grads(t, None, self.group)
            nexp, ncon = (int(round(v)) for v in t.tolist())
        self._last_nexp = nexp
        nexp = max(1, nexp)
        self.mu *= 2.0 * nexp / (nexp + ncon)
        self.mu_dev.fill_(2.0 * self.mu)
        self._tune_count = self._tune_count + 1 if abs(nexp / (nexp + ncon) - 0.5) < self.tolerance else 0
        if self._tune_count > self.patience:
            self.tune = False
            self.tune_off_iteration = self.iteration

    def _shared(self):
        return self.world > 1 and self.exchange == "allgather"

    def _overflowed(self):
        """A walker needed more stepping-out steps or shrinking trials than the one-call path's rounds hold (one device
        read); with walkers exchanged between ranks: on ANY rank -- every rank then redoes the run."""
        mine = bool(self._fast_bufs is not None and getattr(self, "_fast_steps", 0)
                    and int(self._fast_bufs["counters"][2].item()) > 0) or getattr(self, "_overflow_seen", False)
        self._overflow_seen = False
        if self._shared():
            return ldist.any_rank(mine, self.group)
        return mine

    def _snapshot(self):
        return dict(coords=self.coords.clone(), logp=self.logp.clone(), naccept=self.naccept.clone(), step_dev=self.step_dev.clone(),
                    mu=self.mu, tune=self.tune, tune_count=self._tune_count, last_nexp=self._last_nexp, iteration=self.iteration,
                    dev_steps=self._dev_steps, rs=self._rs.get_state(), split_pos=self._split_pos, split_dev=self._split_dev,
                    split_idx=self._split_idx.copy(), neval=self._neval_host)      # (a drawn chunk of splits is never written again)

    def _restore(self, k):
        torch.cuda.current_stream(self.dev).synchronize()
        self.coords.copy_(k["coords"]); self.logp.copy_(k["logp"]); self.naccept.copy_(k["naccept"]); self.step_dev.copy_(k["step_dev"])
        self.mu, self.tune, self._tune_count, self._last_nexp = k["mu"], k["tune"], k["tune_count"], k["last_nexp"]
        self.mu_dev.fill_(2.0 * self.mu)
        self.iteration, self._dev_steps, self._neval_host = k["iteration"], k["dev_steps"], k["neval"]
        self._rs.set_state(k["rs"]); self._split_pos, self._split_dev = k["split_pos"], k["split_dev"]
        self._split_idx[:] = k["split_idx"]
        if self._fast_bufs is not None:
            self._fast_bufs["counters"][2:3].zero_()

    def _guard(self, body):
        """Run ``body`` (iterations that may take the one-call path); if a walker overflowed its rounds, go back to the state
        at entry and run ``body`` again on the round loop -- what comes out is the round loop's chain either way."""
        if self._guarded or not self._use_fast_possible():
            return body()
        snap = self._snapshot()
        self._guarded = True
        try:
            try:
                out = body()
                redo = self._overflowed()
            except _FastOverflow:
                redo = True
            if redo:
                self._restore(snap)
                self.noverflow += 1
                self._fast_after = snap["iteration"] + 1 << 30       # (this attempt: round loop only)
                out = body()
                # a posterior whose brackets have a heavy tail (few walkers, directions between near neighbours: the 2-D
                # notebook problem at 4 walkers overflowed every few iterations) would otherwise spend its run on the round
                # loop: the schedule looks further ahead from now on -- the added rounds evaluate only the walkers still
                # active and cost a few gated-off launches -- and the one-call path stays in use; at the deepest level the
                # old rule applies (200 quiet iterations on the round loop)
                self._fast_after = self.iteration if self._escalate() else self.iteration + 200
            return out
        finally:
            self._guarded = False

    ESCALATIONS = 2                 # times an overflow may deepen the schedule (x4 stepping-out steps, x2 trials each time)

    def _escalate(self):
        """Deepen the one-call path's look-ahead after an overflow: four times the stepping-out steps per side, twice the
        trials, in rounds that double (at most 32 bracket ends per side / 64 trials per round: a wave's lanes in the logic
        kernels).  False at the deepest level."""
        lvl = getattr(self, "_esc_level", 0)
        if lvl >= self.ESCALATIONS:
            return False
        self._esc_level = lvl + 1
        self.set_schedule(self._schedule(self.m_sched[0], 4 * sum(self.m_sched), 32),
                          self._schedule(self.nt_sched[0], 2 * sum(self.nt_sched), 64))
        return True

    def _use_fast_possible(self):
        return not (self.fast is False or self.host_lp or self._fast_ok is False)

    def run(self, nsteps, store=True):
        return self._guard(lambda: EnsembleSampler.run(self, nsteps, store))

    def step(self):
        if not self._guarded:
            return self._guard(self._step)
        return self._step()

    def _step(self):
        st, ns, ndim = _lib.stream(), self.half, self.ndim
        halves = self._splits()
        seed = self.lib_seed
        if self._use_fast() and self._step_fast(halves, seed):
            return
        self.counters.zero_()
        P = _lib.ptr
        nt = self.ntrial
        for h in (0, 1):
            S, Cc = halves[h], halves[1 - h]
            comp, ldc, cidx, nc = self._complement(Cc)
            _lib.call("linna_slice_init", self.ctx, P(self.logp), _lib.iptr(S), ns, P(comp), ldc, _lib.iptr(cidx), nc, ndim,
                      P(self.mu_dev), seed, _lib.iptr(self.step_dev), h, P(self.DIR), self.ld, P(self.Z0), P(self.L),
                      P(self.R), _lib.iptr(self.flags), int(self.maxsteps), st)

            def expand_round(r, slot, gate):            # stepping out, both ends per round
                self._eval_points(S, self.LR, 2, gate)
                self._neval_host += 2 * ns
                _lib.call("linna_slice_expand", self.ctx, P(self.Z0), P(self.Z2), C.c_void_p(self.Z2.data_ptr() + 4 * ns),
                          P(self.L), P(self.R), _lib.iptr(self.flags), ns, _lib.iptr(self.counters), slot, st)

            # shrinking, TWO trials per round: the second is placed as if the first were rejected (the bracket
            # after a rejection depends on where the trial fell, not on its density), so one launch evaluates
            # 2 x nw/2 points -- the whole GPU instead of half of it -- and the rounds halve; the accepted
            # point is the one the one-trial-per-round procedure accepts (same Philox sub-counters).
            def shrink_round(r, slot, gate):
                _lib.call("linna_slice_draw", self.ctx, P(self.L), P(self.R), _lib.iptr(S), P(self.W), _lib.iptr(self.flags),
                          ns, seed, _lib.iptr(self.step_dev), 2 + h, r * nt, nt, st)
                self._eval_points(S, self.W, nt, gate)
                self._neval_host += nt * ns
                _lib.call("linna_slice_shrink", self.ctx, P(self.Z0), P(self.Z2), P(self.L), P(self.R), P(self.W),
                          _lib.iptr(self.flags), P(self.Wacc), P(self.Zacc), ns, _lib.iptr(self.counters), slot, nt, st)

            # (a side steps out at most maxsteps - 1 times: its budget; shrinking is bounded by zeus' `maxiter` passes only)
            self._run_rounds(expand_round, min(int(self.maxsteps), int(self.maxiter)) + 1)
            self._run_rounds(shrink_round, (int(self.maxiter) + nt - 1) // nt, "contractions")
            _lib.call("linna_slice_commit", self.ctx, P(self.coords), self.ld, ndim, P(self.logp), _lib.iptr(S), ns,
                      P(self.DIR), self.ld, P(self.Wacc), P(self.Zacc), st)
            if self.probe is not None:
                self.probe(h, S, dict(Z0=self.Z0, L=self.L, R=self.R, Wacc=self.Wacc, Zacc=self.Zacc, counters=self.counters, fast=False))
        _lib.call("linna_step_increment", self.ctx, _lib.iptr(self.step_dev), st)
        self.iteration += 1
        if self.tune:                                   # zeus: mu *= 2 nexp / (nexp + ncon)
            c = self.counters.cpu().numpy()
            self._tune_mu(int(c[0]), int(c[1]))
