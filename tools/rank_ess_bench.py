"""Device time of one rank-normalised bulk-ESS / tail-ESS check (csrc/chain_rank.hip: ``linna_chain_rank_ess``) beside one
rank-normalised, folded split-R-hat check (``linna_chain_rank_rhat``) of the same chains: 33 parameters, 128 walkers x
1 000 / 10 000 / 100 000 rows and 4096 walkers x 1 000 / 10 000 rows.  HIP events around windows of ITERS calls, the two
checks alternating inside one process, the median of WINDOWS windows per check.  The scratch is what ``DeviceChain`` gives
them (``RANK_SCRATCH`` bytes: the parameters of a round share the launches); the lags are those ``DeviceChain.rank_ess`` ended
with on these chains.

``--driver``: the rate of the driver test's problem (8 parameters, 64 chains, 4 leapfrog steps, ``Madapt = 50``, checks of 50,
4000 iterations, thresholds the plain rule cannot meet) with ``ess_rank`` False and True alternating in one process, the
first pair dropped, and the wall time of one confirmation (``DeviceChain.rank_ess`` with its wait) on such a chain.
usage: rank_ess_bench.py [--walkers 128,4096] [--rows 1000,10000,100000] [--json profiles/rank_ess_bench.json] [--driver]"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for sub in ("tests", os.path.join("tests", "golden")):       # (--driver borrows the driver test's problem)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), sub))
import numpy as np
import torch
from linna_amd import _lib
from linna_amd.sampler import DeviceChain
from rhat_bench import ND, ITERS, WINDOWS, fill, window_ms
from rank_rhat_bench import sizes


def checks(a):
    out = []
    for nw, rows in sizes(a):
        gen = torch.Generator(device="cuda")
        gen.manual_seed(nw + rows)
        dc = DeviceChain()
        fill(dc, nw, rows, gen)
        n = dc.n
        dc.rank_rhat()
        tok = dc.rank_ess_begin()
        bulk, tail = dc.rank_ess_end(tok)                     # (the scratch has grown to the larger need of the two)
        kuse = int(tok["kuse"])
        scratch = dc._rank_scratch
        one = int(_lib.load().linna_chain_rank_ess_scratch_bytes(ND, nw, n // 2 * 2, kuse, 1))
        npar = min(ND, scratch.numel() // one)
        res = torch.empty((ND, 8), dtype=torch.float64, device="cuda")

        def rank_rhat():
            _lib.call("linna_chain_rank_rhat", dc.ctx, _lib.ptr(dc.ct), ND, dc.nwp, nw, 0, n, _lib.ptr(scratch, torch.uint8),
                      int(scratch.numel()), None, dc._dptr(res), _lib.stream())

        def rank_ess():
            _lib.call("linna_chain_rank_ess", dc.ctx, _lib.ptr(dc.ct), ND, dc.nwp, nw, 0, n, kuse, _lib.ptr(scratch, torch.uint8),
                      int(scratch.numel()), dc._dptr(res), _lib.stream())

        routes = dict(rank_rhat=rank_rhat, rank_ess=rank_ess)
        iters = 1 if nw * rows >= 128 * 100000 else ITERS
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(WINDOWS):
            for k, fn in routes.items():
                times[k].append(window_ms(fn, iters))
        row = dict(nw=nw, rows=n, pooled=n // 2 * 2 * nw, lags=kuse + 1, parameters_per_round=npar, scratch_bytes=int(scratch.numel()),
                   min_bulk_ess=float(np.min(bulk)), min_tail_ess=float(np.min(tail)),
                   max_last_pair=float(np.max(dc.last_rank_ess[:, 4:7])),
                   **{k + "_us": 1e3 * float(np.median(v)) for k, v in times.items()},
                   **{k + "_spread_us": [1e3 * float(np.min(v)), 1e3 * float(np.max(v))] for k, v in times.items()})
        out.append(row)
        print("nw %5d rows %6d (S %9d, %2d parameters a round, %4d lags): rank R-hat %11.1f us | bulk- and tail-ESS %11.1f us"
              " | min bulk %.0f tail %.0f" % (nw, n, row["pooled"], npar, kuse + 1, row["rank_rhat_us"], row["rank_ess_us"],
                                              row["min_bulk_ess"], row["min_tail_ess"]), flush=True)
        del dc, scratch
        torch.cuda.empty_cache()
    return out


def driver():
    from linna_amd import sampler, util
    from test_gpu_rhat import _problem
    t, x0, mass = _problem()
    wall = {False: [], True: []}
    for rep in range(4):
        for flag in (False, True):
            with tempfile.TemporaryDirectory() as out:
                np.random.seed(1)
                drv = sampler.HMCSampler(t["lp"], None, None, t["nd"], 64, x0=x0, m=mass, transform=util.Transform(t["priors"]), seed=5)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    drv.sample(None, 4000, samp_steps=4, samp_eps=0, Madapt=50, outdir=out, method="hmc", criterion="rhat", ncheck=50,
                               rhat_tol=1.0 + 1e-9, ess_min=1e9, ess_rank=flag)
                torch.cuda.synchronize()
                if rep:
                    wall[flag].append(time.perf_counter() - t0)
                z = sampler.ChainStore.load(os.path.join(out, "chhmc.h5"))["chain"]
    dc = sampler.DeviceChain()
    dc.append(torch.as_tensor(np.asarray(z, np.float32), device="cuda"))
    dc.rank_ess()
    one = []
    for _ in range(7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dc.rank_ess()
        one.append(time.perf_counter() - t0)
    row = dict(iterations=len(z), wall_s_ess_rank_false=wall[False], wall_s_ess_rank_true=wall[True],
               confirmation_wall_ms=1e3 * float(np.median(one)), confirmation_wall_spread_ms=[1e3 * min(one), 1e3 * max(one)])
    print("driver, %d iterations: ess_rank=False %s s | ess_rank=True %s s | one confirmation (64 chains x %d rows x 8, with its wait) %.3f ms"
          % (len(z), ["%.3f" % v for v in wall[False]], ["%.3f" % v for v in wall[True]], len(z), row["confirmation_wall_ms"]), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", default="128,4096")
    ap.add_argument("--rows", default="1000,10000,100000")
    ap.add_argument("--json", default=None)
    ap.add_argument("--driver", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rank_ess_bench: no GPU")
    out = dict(checks=checks(a))
    if a.driver:
        out["driver"] = driver()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
