#!/usr/bin/env python
"""A/B of the plain against the generic instantiation of the serving kernel on the bench's headline (33 -> 512 x 4 -> 33,
4096 walkers, fp32), INTERLEAVED IN ONE PROCESS through linna_serve_plain -- the first configuration timed in a process
reads slow (NOTES), so the two alternate: sample = HIP events around N back-to-back launches, after a 0.5 s clock ramp.
Usage: python tools/plain_ab.py [samples=9] [launches=2000] [out.json]
Prints the samples, medians, p10-p90 spreads and the verdict of the project's criterion: the plain median must beat the
generic median by more than twice the generic samples' p10-p90 spread."""
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
res = {}
for on in (1, 0):                               # both instantiations launched once, results compared
    _lib.serve_plain(on)
    assert lp.serves_plain(bench.NWALKERS) == bool(on)
    lp.evaluate(z, out=out)
    res[on] = out.cpu().numpy().copy()
assert np.array_equal(res[0], res[1]), "plain and generic lnP differ"
t_ramp = time.perf_counter() + 0.5
while time.perf_counter() < t_ramp:
    for _ in range(64):
        lp.evaluate(z, out=out)
    torch.cuda.synchronize()


def sample(on):
    _lib.serve_plain(on)
    for _ in range(50):
        lp.evaluate(z, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(nl):
        lp.evaluate(z, out=out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / nl      # us per launch


sample(1); sample(0)                            # one untimed round of each
us = {1: [], 0: []}
for i in range(nsamp):
    for on in ((1, 0) if i % 2 == 0 else (0, 1)):
        us[on].append(sample(on))
_lib.serve_plain(1)
med = {k: float(np.median(v)) for k, v in us.items()}
spread = {k: float(np.percentile(v, 90) - np.percentile(v, 10)) for k, v in us.items()}
gain = med[0] - med[1]
r = {"launches_per_sample": nl, "plain_us": us[1], "generic_us": us[0], "plain_median_us": med[1], "generic_median_us": med[0],
     "plain_p10_p90_us": spread[1], "generic_p10_p90_us": spread[0], "gain_us": gain, "gain_percent": 100 * gain / med[0],
     "clearly_faster": bool(gain > 2 * spread[0]), "bit_identical": True}
print("generic us/launch: " + " ".join("%.2f" % v for v in us[0]))
print("plain   us/launch: " + " ".join("%.2f" % v for v in us[1]))
print("median generic %.2f (p10-p90 %.2f)  plain %.2f (p10-p90 %.2f)  gain %.2f us = %.2f %%  clearly faster: %s" % (
    med[0], spread[0], med[1], spread[1], gain, r["gain_percent"], r["clearly_faster"]))
if len(sys.argv) > 3:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[3])), exist_ok=True)
    json.dump(r, open(sys.argv[3], "w"), indent=1)
