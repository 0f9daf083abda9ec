#!/usr/bin/env python
"""What the trajectory-length adaptation of ``method="hmc"`` (``BatchedHMC.adapt_traj``) costs and buys.

1. The cost of a warm-up transition's two extra launches (linna_hmc_chees_begin / linna_hmc_chees_end) and of the read of the
   12 state words, on ChtoModelv2(33,33) at 128 and 4096 chains with 5 leapfrog steps: three loops alternate in one process
   -- the transition alone (``run(1, 5)``'s C call), with the two launches, with the launches and the read -- `--repeats`
   windows of `--trans` transitions each, host clock around a window that ends in a device synchronise; and each of the two
   launches alone, back to back.  Microseconds per transition, median and spread.
2. Effective samples of the widest parameter per second and per gradient launch on the two Gaussian targets of
   tests/test_gpu_hmc_chees.py behind the identity-exact emulator (widths 0.02 ... 0.6 at unit mass; widths 0.003 ... 0.3 with
   ``adapt_mass=True``), 256 chains, `--warmup` adaptive and `--stored` stored transitions: the adapted length against 5
   fixed steps with the per-chain step sizes of ``adapt()``.  Effective samples = chains x stored / the integrated
   autocorrelation time (``sampler.integrated_time``, emcee's estimator; a chain of 5 fixed steps moves so slowly in the wide
   direction that the estimate is a lower bound of its time there).

Prints ONE JSON line.

  python tools/hmc_chees_bench.py [--repeats N] [--trans N] [--warmup N] [--stored N]
"""
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPEATS, TRANS, WARMUP, STORED = _arg("--repeats", 7), _arg("--trans", 200), _arg("--warmup", 300), _arg("--stored", 1000)
NLEAP, EPS = 5, 1e-3


def _stats(v):
    v = sorted(v)
    return {"us": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}


def overhead():
    import numpy as np
    import torch
    import bf16_bench
    from linna_amd import _lib, sampler
    lp = bf16_bench.v2_problem(torch.device("cuda", 0))
    out = {}
    for B in (128, 4096):
        x0 = (0.2 * np.random.RandomState(B).standard_normal((B, 33))).astype(np.float32)
        h = sampler.BatchedHMC(lp, x0, seed=5)
        head = np.zeros(int(_lib.load().linna_hmc_chees_doubles(h.ndim)))
        head[0], head[1], head[5], head[7] = 1.0, math.log(EPS), math.log(10 * EPS), math.log(EPS)
        state = torch.as_tensor(head, device=h.dev)
        r0 = torch.empty(B, dtype=torch.float64, device=h.dev)
        eps_out = torch.empty(B, device=h.dev)                 # (the chains keep EPS: every window does the same work)
        D = lambda t: _lib.ptr(t, torch.float64)

        def begin():
            _lib.call("linna_hmc_chees_begin", h.ctx, B, h.ndim, _lib.ptr(h.x), h.ld, D(state), D(r0), _lib.stream())

        def end():
            _lib.call("linna_hmc_chees_end", h.ctx, B, h.ndim, _lib.ptr(h.mass), None, 0, _lib.ptr(h.q), h.ld, _lib.ptr(h.p), h.ld,
                      _lib.ptr(h.alpha), D(r0), D(state), _lib.ptr(eps_out), 2 ** 30, 0.65, 64, _lib.stream())

        def plain():
            h._enqueue(1, NLEAP, None, None, 0, 0.65, False)

        def launches():
            begin(); plain(); end()

        def whole():
            state[:12].tolist()
            launches()
        loops = {"transition": plain, "with_launches": launches, "with_launches_and_read": whole, "begin_alone": begin, "end_alone": end}
        times = {k: [] for k in loops}
        for rep in range(REPEATS + 1):                         # (the first round warms up)
            for k, f in loops.items():
                h.eps.fill_(EPS)
                state.copy_(torch.as_tensor(head))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(TRANS):
                    f()
                torch.cuda.synchronize()
                if rep:
                    times[k].append(1e6 * (time.perf_counter() - t0) / TRANS)
        res = {k: _stats(v) for k, v in times.items()}
        res["launches_add_us"] = round(res["with_launches"]["us"] - res["transition"]["us"], 2)
        res["read_adds_us"] = round(res["with_launches_and_read"]["us"] - res["with_launches"]["us"], 2)
        out["chains_%d" % B] = res
    return out


def effective_samples():
    import numpy as np
    import torch
    import hmc_chees_emul as chees
    import test_gpu_hmc_chees as tc
    import test_gpu_hmc_mass as tm
    from linna_amd import sampler
    B, out = 256, {}
    targets = {"widths_0.02_0.6_unit_mass": (tc.target(), chees.start(B, 1), chees.WIDTHS, False),
               "widths_0.003_0.3_adapt_mass": (tm.target(), tm.start(B), tm.target()["sz"], True)}
    for name, (t, z0, widths, mass) in targets.items():
        res = {}
        for what in ("adapted", "fixed_5"):
            h = sampler.BatchedHMC(t["lp"], z0, seed=1)
            h.num_steps = 5
            h.adapt(WARMUP, 0.65, adapt_mass=mass, adapt_traj=what == "adapted")
            steps = [h.steps_for(i) for i in range(h.iteration, h.iteration + STORED)] if h.traj is not None else [5] * STORED
            n0 = h.naccept.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            chain, _ = h.run(STORED)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            c = chain.cpu().numpy().astype(np.float64)
            wide = int(np.argmax(widths))
            tau = float(sampler.integrated_time(c[:, :, wide])[0])
            ess = B * STORED / tau
            res[what] = {"seconds": round(dt, 4), "gradient_launches": int(sum(steps)), "mean_steps": round(float(np.mean(steps)), 2),
                         "tau_widest": round(tau, 2), "ess_widest": round(ess, 1), "ess_per_s": round(ess / dt, 1),
                         "ess_per_gradient_launch": round(ess / sum(steps), 3),
                         "acceptance": round(float((h.naccept - n0).float().mean()) / STORED, 4),
                         "std_over_truth_widest": round(float(c[:, :, wide].std() / widths[wide]), 4),
                         "step_size_median": float(h.eps.median()), "traj": h.traj}
        res["ess_per_s_ratio"] = round(res["adapted"]["ess_per_s"] / res["fixed_5"]["ess_per_s"], 2)
        res["ess_per_gradient_launch_ratio"] = round(res["adapted"]["ess_per_gradient_launch"] / res["fixed_5"]["ess_per_gradient_launch"], 2)
        out[name] = res
    return out


if __name__ == "__main__":
    print(json.dumps({"tool": "hmc_chees_bench", "repeats": REPEATS, "trans": TRANS, "warmup": WARMUP, "stored": STORED, "leapfrog_steps": NLEAP,
                      "warmup_transition": overhead(), "effective_samples": effective_samples()}))
