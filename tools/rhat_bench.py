"""Device time of one split-R-hat check and one multi-chain ESS check (csrc/autocorr.hip), beside the tau check of the same
chain: 128 and 4096 walkers, 33 parameters, chains of 1 000, 10 000 and 100 000 rows.  R-hat is timed with the block-moment
records (the 100 rows of a new block already folded into them, as in a run) and with M = NULL (every row read from the
chain); ESS and tau from the running sums after 100 new rows.  HIP events around windows of ITERS calls, the routes
alternating inside one process, the median of WINDOWS windows per route; also the one-off cost of filling all records.
usage: rhat_bench.py [--walkers 128,4096] [--rows 1000,10000,100000] [--json PATH]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from linna_amd import _lib
from linna_amd.sampler import DeviceChain

ND, ITERS, WINDOWS = 33, 5, 7


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def fill(dc, nw, rows, gen):
    """AR(1)-like rows (rho = 0.9) appended in blocks of at most 5000."""
    state = torch.randn(nw, ND, device="cuda", generator=gen)
    done = 0
    while done < rows:
        nb = min(5000, rows - done)
        e = torch.randn(nb, nw, ND, device="cuda", generator=gen)
        blk = torch.empty_like(e)
        for lo in range(0, nb, 100):                      # the recursion in chunks: a scan over 100 rows by cumulative weights
            hi = min(nb, lo + 100)
            w = 0.9 ** torch.arange(1, hi - lo + 1, device="cuda", dtype=torch.float32)
            seg = torch.cumsum(e[lo:hi] / w[:, None, None], 0) * w[:, None, None] + state[None] * w[:, None, None]
            blk[lo:hi] = seg
            state = seg[-1]
        dc.append(blk)
        done += nb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", default="128,4096")
    ap.add_argument("--rows", default="1000,10000,100000")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rhat_bench: no GPU")
    out = []
    for nw in [int(v) for v in a.walkers.split(",")]:
        for rows in [int(v) for v in a.rows.split(",")]:
            gen = torch.Generator(device="cuda")
            gen.manual_seed(nw + rows)
            dc = DeviceChain()
            fill(dc, nw, rows, gen)
            n = dc.n
            t0 = torch.cuda.Event(enable_timing=True); t1 = torch.cuda.Event(enable_timing=True)
            t0.record()
            dc._records()
            t1.record(); t1.synchronize()
            fill_ms = t0.elapsed_time(t1)
            r_rec, r_raw = dc.rhat(), dc.rhat(records=False)
            assert np.allclose(r_rec, r_raw, rtol=1e-9, atol=0, equal_nan=True), (r_rec, r_raw)
            dc.integrated_time(); ess = dc.ess(); tau = dc.integrated_time()
            S, T = dc._S, dc._T

            def tau_check():                              # what a check enqueues for 100 new rows: the update and the estimate
                dc._update(S, T, n - 100, n, 0, n, 0, len(S), False)
                dc._estimate(S, T, 0, n, 5.0, dc.nws)

            def ess_check():
                dc._update(S, T, n - 100, n, 0, n, 0, len(S), False)
                dc._estimate_ess(S, T, 0, n, dc.nws)

            res = torch.empty((ND, 4), dtype=torch.float64, device="cuda")
            nb = n // _lib.RHAT_BLOCK

            def rhat_records():                           # the newest record filled again (a run fills at most one per 100 rows)
                _lib.call("linna_chain_block_moments", dc.ctx, _lib.ptr(dc.ct), ND, dc.nwp, nb - 1, nb, dc._dptr(dc._M), _lib.stream())
                _lib.call("linna_chain_rhat", dc.ctx, _lib.ptr(dc.ct), ND, dc.nwp, nw, 0, n, dc._dptr(dc._M), nb, dc._dptr(res), _lib.stream())

            def rhat_chain():
                _lib.call("linna_chain_rhat", dc.ctx, _lib.ptr(dc.ct), ND, dc.nwp, nw, 0, n, None, 0, dc._dptr(res), _lib.stream())

            routes = dict(tau=tau_check, ess=ess_check, rhat_records=rhat_records, rhat_chain=rhat_chain)
            iters = 1 if nw * rows >= 4096 * 100000 else ITERS
            for fn in routes.values():
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in routes}
            for _ in range(WINDOWS):
                for k, fn in routes.items():
                    times[k].append(window_ms(fn, iters))
            row = dict(nw=nw, rows=n, lags=len(S), sum_lanes=dc.nwc, records_fill_ms=fill_ms, max_rhat=float(np.max(r_rec)), min_ess=float(np.min(ess)),
                       max_tau=float(np.max(tau)), **{k + "_us": 1e3 * float(np.median(v)) for k, v in times.items()},
                       **{k + "_spread_us": [1e3 * float(np.min(v)), 1e3 * float(np.max(v))] for k, v in times.items()})
            out.append(row)
            print("nw %5d rows %6d (lags %d): tau check %9.1f us | ess check %9.1f us | R-hat with records %9.1f us | R-hat from the chain %11.1f us"
                  " | filling all records once %9.2f ms" % (nw, n, len(S), row["tau_us"], row["ess_us"], row["rhat_records_us"], row["rhat_chain_us"],
                                                             fill_ms), flush=True)
            del dc, S, T
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
