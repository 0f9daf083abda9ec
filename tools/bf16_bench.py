#!/usr/bin/env python
"""fp32 against the opt-in bf16 serving engine (linna_logprob_set_precision), device events, resident inputs, after warm-up:
  headline  the 4x4 512 MLP (bench.py's problem) at 4096 walkers, one linna_logprob_eval
  v2_64     one 64-row ChtoModelv2(33,33) evaluation
  stretch   one 2048-proposal stretch half step (linna_stretch_half_step, the 4096-walker ensemble, MLP)
  emcee128  emcee iterations per second at 128 walkers on ChtoModelv2(33,33) (linna_stretch_run blocks)
  slice128 / slice4096   zeus iterations per second (SliceEnsembleSampler.run) on ChtoModelv2(33,33) at 128 walkers and
            on the MLP at 4096: fp32 one-call, bf16 one-call, bf16 round loop, alternating, mu fixed (slice_rates)
  grad4096  one gradient launch (Log_prob.evaluate_with_grad) at 4096 rows, the MLP and ChtoModelv2(33,33): the fp32 one-launch
            gradient against the bf16 one (grad_precision="bf16"), alternating in one process, five runs each
  hmc       one BatchedHMC.step(5, eps) at 1024 and 4096 chains on both networks, the same way (grad_rates)
Prints ONE JSON line.  --only-slice / --no-slice: the slice objects alone / left out; --slice-trace: the bf16 one-call
route at 128 walkers alone (the process to put under a kernel trace); --grad: grad4096 and hmc alone; --grad-trace: a
short run of both forms of both (the process to put under a kernel trace).  FLOP/s count 2 x multiply-adds of the network per walker, against the bf16 dense peak (2.5 PF spec);
bytes = the weight stream each workgroup reads per launch (padded fragment layout) x workgroups.
usage: python tools/bf16_bench.py [--reps N] [--only-slice | --no-slice | --slice-trace | --grad | --grad-trace]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from linna_amd import _lib, nn, predictor_gpu, sampler, util  # noqa: E402
from oracle import emulator  # noqa: E402

BF16_PEAK = 2.5e15
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 200


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def with_precision(lp, precision):
    return util.Log_prob(lp.data_new, lp.invcov_new, lp.model, lp.y_invtransform_data, lp.transform, lp.T, lp.loglikelihoodfunc,
                         nograd=True, precision=precision)


def v2_problem(dev):
    """ChtoModelv2(33,33), bench.py's transforms and likelihood (diagonal)."""
    lp0, _, c = bench.build_problem(dev)
    torch.manual_seed(4321)
    model = nn.ChtoModelv2(33, 33, None)
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    pred = predictor_gpu.Predictor(33, 33, model=model, device=dev,
                                   X_transform=util.X_transform_class(t(c["X_mean"]), t(c["X_std"]), "cpu", None),
                                   y_transform=util.Y_transform_class(t(c["y_mean"]), t(c["y_std"]), "cpu"))
    return util.Log_prob(lp0.data_new, lp0.invcov_new, pred, lp0.y_invtransform_data, lp0.transform, 1.0,
                         util.gaussianlogliklihood, nograd=True)


def stream_bytes(kind, bf, **kw):
    """Weight bytes one workgroup streams per launch: every matrix product, K padded to the step (16 fp32 / 32 bf16, the
    first layer twice as wide in bf16: [W | W] over [x_hi ; x_lo]), N to 64 columns."""
    ks, bpe = (32, 2) if bf else (16, 4)
    tot = 0
    for i, op in enumerate(emulator.topology(kind, 33, 33, **kw)):
        if op[0] == "linear":
            _, _, K, N, _ = op
            K = 2 * K if (bf and i == 0) else K
            tot += -(-K // ks) * ks * -(-N // 64) * 64
        elif op[0] == "resblock":
            _, _, K, C, N = op
            tot += -(-K // ks) * ks * 64 + -(-(K + C) // ks) * ks * -(-N // 64) * 64
    return tot * bpe


def slice_rates(lp32, nw, iters, repeats, only=None):
    """zeus iterations per second through SliceEnsembleSampler.run at `nw` walkers: fp32 one-call, bf16 one-call and bf16 round
    loop (fast=False: what a bf16 Log_prob ran before the bf16 slice evaluation existed), alternating in one process,
    `repeats` timed runs of `iters` iterations each.  mu is tuned once (fp32) and then FIXED (tune=False) and every route
    starts from the tuned run's ensemble, so the three do the same work; the evaluations per walker and iteration are
    printed beside each rate, and the spread over the repeats beside the median."""
    import time
    t = sampler.SliceEnsembleSampler(nw, 33, lp32, seed=1)
    t.set_state(0.05 * np.random.RandomState(7).standard_normal((nw, 33)))
    t.run(150, store=False)
    torch.cuda.synchronize()
    mu, x0 = float(t.mu), t.coords[:, :33].cpu().numpy().copy()
    lpb = with_precision(lp32, "bf16")
    routes = {"fp32_one_call": (lp32, True), "bf16_one_call": (lpb, True), "bf16_round_loop": (lpb, False)}
    if only:
        routes = {only: routes[only]}
    ens, rates, evals = {}, {k: [] for k in routes}, {}
    for k, (lp, fast) in routes.items():
        e = sampler.SliceEnsembleSampler(nw, 33, lp, seed=3, tune=False, mu=mu, fast=fast)
        e.set_state(x0)
        e.run(80, store=False)                               # warm-up; the later rounds' engines settle (iteration 64)
        torch.cuda.synchronize()
        ens[k] = e
    for _ in range(repeats):
        for k, e in ens.items():
            n0, i0 = e.neval, e.iteration
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.run(iters, store=False)
            torch.cuda.synchronize()
            rates[k].append(iters / (time.perf_counter() - t0))
            evals[k] = (e.neval - n0) / max(1, e.iteration - i0) / nw
    out = {"walkers": nw, "mu": round(mu, 4), "iterations_per_run": iters, "repeats": repeats}
    for k, e in ens.items():
        r = np.asarray(rates[k])
        out[k] = {"it_per_s": round(float(np.median(r)), 1), "it_per_s_min": round(float(r.min()), 1), "it_per_s_max": round(float(r.max()), 1),
                  "spread_pct": round(100.0 * float(r.max() - r.min()) / float(np.median(r)), 2),
                  "evals_per_walker_per_iteration": round(evals[k], 2), "one_call": e._fast_ok is True, "overflows": e.noverflow}
    if not only:
        assert out["fp32_one_call"]["one_call"] and out["bf16_one_call"]["one_call"] and not out["bf16_round_loop"]["one_call"]
        out["bf16_one_call_over_round_loop"] = round(out["bf16_one_call"]["it_per_s"] / out["bf16_round_loop"]["it_per_s"], 3)
        out["bf16_over_fp32_one_call"] = round(out["bf16_one_call"]["it_per_s"] / out["fp32_one_call"]["it_per_s"], 3)
    return out


def _stats(us):
    us = np.asarray(us)
    return {"us": round(float(np.median(us)), 2), "us_min": round(float(us.min()), 2), "us_max": round(float(us.max()), 2),
            "spread_pct": round(100.0 * float(us.max() - us.min()) / float(np.median(us)), 2)}


def grad_rates(lps, reps, repeats=5):
    """grad4096 and hmc: the fp32 object against the bf16 one with the bf16 gradient, alternating in one process, `repeats`
    timed runs of `reps` calls each; median and spread, and the ratio fp32 / bf16 of the medians."""
    out = {"grad4096": {}, "hmc": {}, "repeats": repeats}
    for net, lp32 in lps.items():
        forms = {"fp32": lp32, "bf16": util.Log_prob(lp32.data_new, lp32.invcov_new, lp32.model, lp32.y_invtransform_data, lp32.transform,
                                                      lp32.T, lp32.loglikelihoodfunc, nograd=True, precision="bf16", grad_precision="bf16")}
        z = torch.randn(4096, 33, device="cuda") * 0.5
        lnp, g = torch.empty(4096, device="cuda"), torch.empty(4096, 33, device="cuda")
        t = {k: [] for k in forms}
        for _ in range(repeats):
            for k, lp in forms.items():
                t[k].append(timed(lambda: lp.evaluate_with_grad(z, out=lnp, grad=g), reps))
        r = {k: _stats(v) for k, v in t.items()}
        r["fp32_over_bf16"] = round(r["fp32"]["us"] / r["bf16"]["us"], 3)
        out["grad4096"][net] = r
        for B in (1024, 4096):
            x0 = (0.2 * np.random.RandomState(B).standard_normal((B, 33))).astype(np.float32)
            hm = {k: sampler.BatchedHMC(lp, x0, seed=5) for k, lp in forms.items()}
            t = {k: [] for k in forms}
            for _ in range(repeats):
                for k, h in hm.items():
                    t[k].append(timed(lambda: h.step(5, 1e-3), max(1, reps // 5)))
            r = {k: dict(_stats(v), acceptance=round(float(hm[k].naccept.float().mean()) / max(1, int(hm[k].step_dev.item())), 4)) for k, v in t.items()}
            r["fp32_over_bf16"] = round(r["fp32"]["us"] / r["bf16"]["us"], 3)
            out["hmc"]["%s_%d" % (net, B)] = r
    return out


def main():
    dev = torch.device("cuda", 0)
    res = {"tool": "bf16_bench", "reps": REPS, "bf16_peak_flops": BF16_PEAK}
    lp_mlp, _, _ = bench.build_problem(dev)
    lp_v2 = v2_problem(dev)
    if "--grad" in sys.argv or "--grad-trace" in sys.argv:
        trace = "--grad-trace" in sys.argv
        res.update(grad_rates({"mlp_4x512": lp_mlp, "ChtoModelv2_33_33": lp_v2}, 20 if trace else REPS, 1 if trace else 5))
        print(json.dumps(res))
        return
    if "--slice-trace" in sys.argv:                          # the bf16 one-call route at 128 walkers alone (for a kernel trace)
        print(json.dumps({"tool": "bf16_bench", "slice128": slice_rates(lp_v2, 128, 600, 3, only="bf16_one_call")}))
        return
    if "--no-slice" not in sys.argv:
        res["slice128"] = dict(slice_rates(lp_v2, 128, 600, 5), workload="ChtoModelv2(33,33)")
        res["slice4096"] = dict(slice_rates(lp_mlp, 4096, 100, 5), workload="4x512 MLP")
    if "--only-slice" in sys.argv:
        print(json.dumps(res))
        return
    macs = {"MLP": emulator.macs_per_eval("MLP", 33, 33, width=512, depth=4), "ChtoModelv2": emulator.macs_per_eval("ChtoModelv2", 33, 33)}
    for prec in ("fp32", "bf16"):
        bf = prec == "bf16"
        m = with_precision(lp_mlp, prec)
        v = with_precision(lp_v2, prec)
        for tag, lp, kind, B in (("headline", m, "MLP", 4096), ("v2_64", v, "ChtoModelv2", 64)):
            z = torch.randn(B, 33, device=dev) * 0.5
            out = torch.empty(B, device=dev)
            us = timed(lambda: lp.evaluate(z, out=out), REPS)
            kw = dict(width=512, depth=4) if kind == "MLP" else {}
            rows = 16 if B >= 2048 else 4
            wg = -(-B // rows)
            res["%s_%s_us" % (tag, prec)] = round(us, 2)
            res["%s_%s_tflops" % (tag, prec)] = round(2.0 * macs[kind] * B / (us * 1e-6) / 1e12, 2)
            res["%s_%s_pct_bf16_peak" % (tag, prec)] = round(100.0 * 2.0 * macs[kind] * B / (us * 1e-6) / BF16_PEAK, 3)
            res["%s_%s_stream_bytes_per_wg" % (tag, prec)] = stream_bytes(kind, bf, **kw)
            res["%s_%s_stream_bytes_per_launch" % (tag, prec)] = stream_bytes(kind, bf, **kw) * wg
        # 2048-proposal stretch half step: the fused half steps of a 4096-walker ensemble (one step = two half steps)
        ens = sampler.EnsembleSampler(4096, 33, m, seed=1)
        ens.set_state(0.3 * np.random.RandomState(0).standard_normal((4096, 33)).astype(np.float32))
        us = timed(ens.step, REPS // 4)
        assert ens.fused is True, "stretch half step did not run fused"
        res["stretch_half_step_%s_us" % prec] = round(us / 2, 2)
        # emcee at 128 walkers, ChtoModelv2(33,33): iterations per second of blocks of linna_stretch_run
        e128 = sampler.EnsembleSampler(128, 33, v, seed=2)
        e128.set_state(0.3 * np.random.RandomState(1).standard_normal((128, 33)).astype(np.float32))
        e128.run(50, store=False)
        torch.cuda.synchronize()
        us = timed(lambda: e128.run(100, store=False), 3)
        res["emcee128_%s_it_per_s" % prec] = round(100.0 / (us * 1e-6), 1)
    res["headline_speedup"] = round(res["headline_fp32_us"] / res["headline_bf16_us"], 3)
    res["v2_64_speedup"] = round(res["v2_64_fp32_us"] / res["v2_64_bf16_us"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
