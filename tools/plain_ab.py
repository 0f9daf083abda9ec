#!/usr/bin/env python
"""A/B of the four instantiations of the serving kernel a plain launch can take on the bench's headline (33 -> 512 x 4 -> 33,
4096 walkers, fp32): the hand-placed one without the MFMAs on zero padding ("trim", the default), the hand-placed one
("hand", linna_serve_plain_trim(0)), the plain one with the compiler-scheduled step ("plain", linna_serve_plain_sched(0))
and the generic one ("generic", linna_serve_plain(0)),
INTERLEAVED IN ONE PROCESS -- the first configuration timed in a process reads slow (NOTES), so they alternate, the order
rotating from round to round: sample = HIP events around N back-to-back launches, after a 0.5 s clock ramp.
Usage: python tools/plain_ab.py [samples=9] [launches=2000] [out.json]
Prints the samples, medians, p10-p90 spreads and the verdict of the project's criterion for each step: the faster median
must beat the baseline's median by more than twice the baseline samples' p10-p90 spread (trim against hand, hand against
plain, plain against generic)."""
import json, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from linna_amd import _lib

nsamp = int(sys.argv[1]) if len(sys.argv) > 1 else 9
nl = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
lp, model, consts = bench.build_problem(torch.device("cuda", 0))
z = torch.as_tensor(np.random.RandomState(100).standard_normal((bench.NWALKERS, bench.NIN)).astype(np.float32), device="cuda")
out = torch.empty(bench.NWALKERS, dtype=torch.float32, device="cuda")
# (linna_serve_plain, linna_serve_plain_sched, linna_serve_plain_trim)
VARIANTS = {"trim": (1, 1, 1), "hand": (1, 1, 0), "plain": (1, 0, 0), "generic": (0, 1, 0)}


def select(v):
    _lib.serve_plain(VARIANTS[v][0])
    _lib.serve_plain_sched(VARIANTS[v][1])
    _lib.serve_plain_trim(VARIANTS[v][2])


res = {}
for v in VARIANTS:                              # every instantiation launched once, results compared
    select(v)
    assert lp.serves_plain(bench.NWALKERS) == bool(VARIANTS[v][0])
    lp.evaluate(z, out=out)
    res[v] = out.cpu().numpy().copy()
assert all(np.array_equal(res["trim"], res[v]) for v in VARIANTS), "lnP differs between the instantiations"
t_ramp = time.perf_counter() + 0.5
while time.perf_counter() < t_ramp:
    for _ in range(64):
        lp.evaluate(z, out=out)
    torch.cuda.synchronize()


def sample(v):
    select(v)
    for _ in range(50):
        lp.evaluate(z, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(nl):
        lp.evaluate(z, out=out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / nl      # us per launch


names = list(VARIANTS)
for v in names:                                 # one untimed round of each
    sample(v)
us = {v: [] for v in names}
for i in range(nsamp):
    for v in names[i % len(names):] + names[:i % len(names)]:
        us[v].append(sample(v))
select("trim")
med = {k: float(np.median(v)) for k, v in us.items()}
spread = {k: float(np.percentile(v, 90) - np.percentile(v, 10)) for k, v in us.items()}
r = {"launches_per_sample": nl, "bit_identical": True}
for v in names:
    r[v + "_us"] = us[v]; r[v + "_median_us"] = med[v]; r[v + "_p10_p90_us"] = spread[v]
    print("%-7s us/launch: " % v + " ".join("%.2f" % x for x in us[v]))
for new, base in (("trim", "hand"), ("hand", "plain"), ("plain", "generic")):
    gain = med[base] - med[new]
    ok = bool(gain > 2 * spread[base])
    r["%s_vs_%s" % (new, base)] = {"gain_us": gain, "gain_percent": 100 * gain / med[base], "clearly_faster": ok}
    print("%s %.2f (p10-p90 %.2f) against %s %.2f (p10-p90 %.2f): gain %.2f us = %.2f %%  clearly faster: %s" % (
        new, med[new], spread[new], base, med[base], spread[base], gain, 100 * gain / med[base], ok))
if len(sys.argv) > 3:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])), exist_ok=True)
    json.dump(r, open(sys.argv[3], "w"), indent=1)
