#!/usr/bin/env python
"""lnP and d lnP / d z under a DENSE inverse covariance: the opt-in one-launch gradient (Log_prob(dense_grad="fused")) against
the layered route of the same build (the default object: prior map, layer GEMMs, row-dot GEMM, D Ssym, linna_net_backward,
prior map's derivative, kick and drift as launches of their own), ChtoModelv2(26,457) and ChtoModelv2(40,1000) with a dense
covariance, at 128, 1024, 2048 and 4096 rows.  Both objects live in ONE process, share the emulator and alternate sample by
sample; inputs are resident.

  per launch    `--repeats` samples of `--launches` linna_logprob_grad calls each, device events around a sample
  transitions   `--repeats` samples of `--trans` BatchedHMC.run transitions of 5 leapfrog steps at 128 and 1024 chains, host
                clock around work that ends in a device synchronise

Median and p10-p90 of the samples; `grad_launches` says what Log_prob.grad_launches reports for the batch (0 for "fused": the
batch's engine does not fit the program and the call IS the layered route).  Prints ONE JSON line
(profiles/grad_dense_bench.json).

  python tools/grad_dense_bench.py [--repeats N] [--launches N] [--trans N]
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPEATS, LAUNCHES, TRANS = _arg("--repeats", 9), _arg("--launches", 200), _arg("--trans", 40)
NLEAP, EPS = 5, 1e-4
BATCHES = (128, 1024, 2048, 4096)
HMC_BATCHES = (128, 1024)
NETS = ((26, 457), (40, 1000))


def _stats(v, digits=1):
    v = sorted(v)
    n = len(v)
    return {"median": round(v[n // 2], digits), "p10": round(v[int(0.1 * (n - 1) + 0.5)], digits), "p90": round(v[int(0.9 * (n - 1) + 0.5)], digits)}


def problem(nin, nout, dev):
    """ChtoModelv2(nin, nout) with its default initialisation, unit-scale transforms, a dense covariance (correlated errors of
    condition ~1e2), Gaussian priors: the fused and the layered object on ONE emulator."""
    import numpy as np
    import torch
    from linna_amd import nn, predictor_gpu, util
    rs = np.random.RandomState(nin + nout)
    torch.manual_seed(1000 + nout)
    model = nn.ChtoModelv2(nin, nout, None)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    sigma = rs.uniform(0.5, 2.0, nout)
    A = rs.standard_normal((nout, nout)) / np.sqrt(nout)
    corr = 0.5 * (A @ A.T) + 0.5 * np.eye(nout)
    cov = corr * np.outer(sigma, sigma)
    sig = np.sqrt(np.diag(cov))
    pred = predictor_gpu.Predictor(nin, nout, model=model, device=dev,
                                   X_transform=util.X_transform_class(t(rs.standard_normal(nin)), t(rs.uniform(0.5, 2.0, nin)), "cpu", None),
                                   y_transform=util.Y_transform_class(t(rs.standard_normal(nout)), t(rs.uniform(0.5, 2.0, nout)), "cpu"))
    priors = [{"param": "p%d" % i, "dist": "gauss", "arg1": 0.0, "arg2": 1.0} for i in range(nin)]
    data, inv = t(rs.standard_normal(nout) * sig), t(np.linalg.inv(cov))
    make = lambda how: util.Log_prob(data, inv, pred, util.Y_invtransform_data(sig, "cpu"), util.Transform(priors), 1.0,
                                     util.gaussianlogliklihood, nograd=True, dense_grad=how)
    fused, lay = make("fused"), make("layered")
    fused._ensure(); lay._ensure()
    return fused, lay


def measure():
    import numpy as np
    import torch
    from linna_amd import sampler
    dev = torch.device("cuda", 0)
    out = {}
    for nin, nout in NETS:
        fused, lay = problem(nin, nout, dev)
        for B in BATCHES:
            z = torch.as_tensor((0.3 * np.random.RandomState(B).standard_normal((B, nin))).astype(np.float32), device=dev)
            lnp, g = torch.empty(B, device=dev), torch.empty((B, nin), device=dev)
            objs = {"fused": fused, "layered": lay}
            r = {"grad_launches": {k: lp.grad_launches(B) for k, lp in objs.items()}}
            for lp in objs.values():                          # warm-up: streams laid out, workspaces allocated
                for _ in range(5):
                    lp.evaluate_with_grad(z, out=lnp, grad=g)
            torch.cuda.synchronize()
            us = {k: [] for k in objs}
            for _ in range(REPEATS):
                for k, lp in objs.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(LAUNCHES):
                        lp.evaluate_with_grad(z, out=lnp, grad=g)
                    b.record()
                    torch.cuda.synchronize()
                    us[k].append(1e3 * a.elapsed_time(b) / LAUNCHES)
            r["grad_us"] = {k: _stats(v, 2) for k, v in us.items()}
            gu = r["grad_us"]
            r["fused_over_layered"] = round(gu["fused"]["median"] / gu["layered"]["median"], 4)
            if B in HMC_BATCHES:
                x0 = (0.2 * np.random.RandomState(B + 1).standard_normal((B, nin))).astype(np.float32)
                hs = {k: sampler.BatchedHMC(lp, x0, seed=5) for k, lp in objs.items()}
                for h in hs.values():
                    h.eps.fill_(EPS)
                    h.run(3, NLEAP, store=False)
                torch.cuda.synchronize()
                tps = {k: [] for k in hs}
                for _ in range(REPEATS):
                    for k, h in hs.items():
                        t0 = time.perf_counter()
                        h.run(TRANS, NLEAP, store=False)
                        torch.cuda.synchronize()
                        tps[k].append(TRANS / (time.perf_counter() - t0))
                r["transitions_per_s"] = {k: _stats(v) for k, v in tps.items()}
                del hs
            out["ChtoModelv2_%d_%d_B%d" % (nin, nout, B)] = r
    return out


def main():
    print(json.dumps({"tool": "grad_dense_bench", "repeats": REPEATS, "launches": LAUNCHES, "trans": TRANS, "leapfrog_steps": NLEAP,
                      "results": measure()}))


if __name__ == "__main__":
    main()
