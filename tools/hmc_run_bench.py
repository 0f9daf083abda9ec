#!/usr/bin/env python
"""HMC transitions per second: ``BatchedHMC.run`` (linna_hmc_run_energy with everything optional null, which is linna_hmc_run:
one C call per block of transitions, the step sizes in a device array) against a loop of ``BatchedHMC.step`` (3 + num_steps ctypes calls per transition, the step size a scalar), at 128 and
4096 chains, on ChtoModelv2(33,33) and the 4x512 MLP (bench.py's problem), fp32 and bf16 gradient engine, 5 leapfrog steps.
Host clock around work that ends in a device synchronise (the host's share is what differs), the two routes alternating
in one process, `--repeats` timed windows each; median and spread.  Prints ONE JSON line.

  python tools/hmc_run_bench.py [--repeats N] [--trans N]
  python tools/hmc_run_bench.py --scalar-only          only the step() loop (what the A/B below runs in its children)
  python tools/hmc_run_bench.py --ab OTHER_LIB.so      the scalar step() loop and ``run()`` under this tree's library and under
        another build of it (the parent commit's: what a change adds to the existing routes must cost nothing), alternating,
        each in a fresh process (LINNA_LIB_PATH), `--rounds` of both; prints the medians and ratios.  With `--scalar-only`
        the children time the step() loop alone (a library older than linna_hmc_run); `--this THIRD_LIB.so` puts a third
        build in this tree's place (two copies of one build against each other: the spread of the comparison itself)
  python tools/hmc_run_bench.py --moments              ``run(moments=True)`` (linna_hmc_run_moments' launches: one more per transition,
        the positions of all chains merged into running float64 moments -- what the mass adaptation's windows enqueue) against
        ``run()``, alternating in one process, ChtoModelv2(33,33) only; prints both rates and their ratio
  python tools/hmc_run_bench.py --dense                ``run()`` under a dense mass with C = I (linna_hmc_run_dense's launches: the kick and the
        drift as a launch of their own behind every gradient launch, 2 + num_steps launches more per transition) against
        ``run()`` at unit mass -- the same chains --, with and without the (co-)moments launch, alternating in one process,
        ChtoModelv2(33,33) only; and the duration of one linna_hmc_chol_from_comoments launch at 33 and 128 parameters
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPEATS, TRANS, ROUNDS = _arg("--repeats", 5), _arg("--trans", 200), _arg("--rounds", 3)
NLEAP, EPS = 5, 1e-3


def _stats(v):
    v = sorted(v)
    return {"per_s": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1)}


def measure(scalar_only):
    import numpy as np
    import torch
    import bench
    import bf16_bench
    from linna_amd import _lib, sampler, util
    if os.environ.get("LINNA_LIB_PATH"):                      # another build of the library: bind what it exports
        _lib.load(missing_ok=True)
    dev = torch.device("cuda", 0)
    nets = {"ChtoModelv2_33_33": bf16_bench.v2_problem(dev), "mlp_4x512": bench.build_problem(dev)[0]}
    out = {}
    for net, lp32 in nets.items():
        forms = {"fp32": lp32, "bf16": util.Log_prob(lp32.data_new, lp32.invcov_new, lp32.model, lp32.y_invtransform_data, lp32.transform,
                                                      lp32.T, lp32.loglikelihoodfunc, nograd=True, precision="bf16", grad_precision="bf16")}
        for prec, lp in forms.items():
            for B in (128, 4096):
                x0 = (0.2 * np.random.RandomState(B).standard_normal((B, 33))).astype(np.float32)
                h = sampler.BatchedHMC(lp, x0, seed=5)
                h.eps.fill_(EPS)

                def loop():
                    for _ in range(TRANS):
                        h.step(NLEAP, EPS)

                def block():
                    h.run(TRANS, NLEAP, store=False)
                routes = {"step_loop": loop} if scalar_only else {"step_loop": loop, "run": block}
                for fn in routes.values():                    # warm-up: every shape, both routes
                    fn()
                torch.cuda.synchronize()
                t = {k: [] for k in routes}
                for _ in range(REPEATS):
                    for k, fn in routes.items():
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        t[k].append(TRANS / (time.perf_counter() - t0))
                r = {k: _stats(v) for k, v in t.items()}
                if not scalar_only:
                    r["run_over_step_loop"] = round(r["run"]["per_s"] / r["step_loop"]["per_s"], 3)
                out["%s_%s_%d" % (net, prec, B)] = r
    return out


def measure_moments():
    import numpy as np
    import torch
    import bf16_bench
    from linna_amd import sampler, util
    dev = torch.device("cuda", 0)
    lp32 = bf16_bench.v2_problem(dev)
    forms = {"fp32": lp32, "bf16": util.Log_prob(lp32.data_new, lp32.invcov_new, lp32.model, lp32.y_invtransform_data, lp32.transform,
                                                  lp32.T, lp32.loglikelihoodfunc, nograd=True, precision="bf16", grad_precision="bf16")}
    out = {}
    for prec, lp in forms.items():
        for B in (128, 4096):
            x0 = (0.2 * np.random.RandomState(B).standard_normal((B, 33))).astype(np.float32)
            h = sampler.BatchedHMC(lp, x0, seed=5)
            h.eps.fill_(EPS)
            routes = {"run": lambda: h.run(TRANS, NLEAP, store=False),
                      "run_moments": lambda: h.run(TRANS, NLEAP, store=False, moments=True)}
            for fn in routes.values():
                fn()
            torch.cuda.synchronize()
            t = {k: [] for k in routes}
            for _ in range(REPEATS):
                for k, fn in routes.items():
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    t[k].append(TRANS / (time.perf_counter() - t0))
            r = {k: _stats(v) for k, v in t.items()}
            r["run_moments_over_run"] = round(r["run_moments"]["per_s"] / r["run"]["per_s"], 4)
            r["moments_us_per_transition"] = round(1e6 / r["run_moments"]["per_s"] - 1e6 / r["run"]["per_s"], 2)
            out["ChtoModelv2_33_33_%s_%d" % (prec, B)] = r
    return out


def measure_dense():
    import numpy as np
    import torch
    import bf16_bench
    from linna_amd import _lib, sampler, util
    dev = torch.device("cuda", 0)
    lp32 = bf16_bench.v2_problem(dev)
    forms = {"fp32": lp32, "bf16": util.Log_prob(lp32.data_new, lp32.invcov_new, lp32.model, lp32.y_invtransform_data, lp32.transform,
                                                  lp32.T, lp32.loglikelihoodfunc, nograd=True, precision="bf16", grad_precision="bf16")}
    out = {}
    for prec, lp in forms.items():
        for B in (128, 4096):
            x0 = (0.2 * np.random.RandomState(B).standard_normal((B, 33))).astype(np.float32)
            h, d = sampler.BatchedHMC(lp, x0, seed=5), sampler.BatchedHMC(lp, x0, mass=np.eye(33), seed=5)
            h.eps.fill_(EPS); d.eps.fill_(EPS)
            routes = {"run": lambda: h.run(TRANS, NLEAP, store=False), "run_dense": lambda: d.run(TRANS, NLEAP, store=False),
                      "run_moments": lambda: h.run(TRANS, NLEAP, store=False, moments=True),
                      "run_dense_comoments": lambda: d.run(TRANS, NLEAP, store=False, moments=True)}
            for fn in routes.values():
                fn()
            torch.cuda.synchronize()
            t = {k: [] for k in routes}
            for _ in range(REPEATS):
                for k, fn in routes.items():
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    t[k].append(TRANS / (time.perf_counter() - t0))
            r = {k: _stats(v) for k, v in t.items()}
            us = lambda k: 1e6 / r[k]["per_s"]
            r["run_dense_over_run"] = round(r["run_dense"]["per_s"] / r["run"]["per_s"], 4)
            r["dense_us_per_transition"] = round(us("run_dense") - us("run"), 2)
            r["moments_us_per_transition"] = round(us("run_moments") - us("run"), 2)
            r["comoments_us_per_transition"] = round(us("run_dense_comoments") - us("run_dense"), 2)
            r["same_chains"] = bool(torch.equal(h.x, d.x))
            out["ChtoModelv2_33_33_%s_%d" % (prec, B)] = r
    chol = {}
    for nd in (33, 128):                                       # one factorisation of a well-conditioned covariance, device clock
        ld = _lib.ld4(nd)
        nw = int(_lib.load().linna_hmc_comoments_doubles(nd))
        rows = np.random.RandomState(nd).standard_normal((4096, nd)).astype(np.float32)
        X = torch.zeros((4096, ld), device=dev)
        X[:, :nd].copy_(torch.as_tensor(rows))
        mom = torch.zeros(nw, dtype=torch.float64, device=dev)
        Cm = torch.zeros((2, nd, ld), device=dev)
        info = torch.zeros(1, dtype=torch.int32, device=dev)
        ctx, st = _lib.ctx(0), _lib.stream()
        _lib.call("linna_hmc_comoments", ctx, 4096, nd, _lib.ptr(X), ld, _lib.ptr(mom, torch.float64), st)
        call = lambda: _lib.call("linna_hmc_chol_from_comoments", ctx, nd, _lib.ptr(mom, torch.float64), _lib.ptr(Cm), ld,
                                 _lib.iptr(info), 0, st)
        call()
        torch.cuda.synchronize()
        us = []
        for _ in range(20):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); call(); b.record()
            torch.cuda.synchronize()
            us.append(1e3 * a.elapsed_time(b))
        us.sort()
        chol["ndim_%d" % nd] = {"us": round(us[len(us) // 2], 1), "min": round(us[0], 1), "max": round(us[-1], 1), "info": int(info.item())}
    return out, chol


def ab(other):
    scalar = ["--scalar-only"] if "--scalar-only" in sys.argv else []
    runs = {"this": [], "other": []}
    for rnd in range(ROUNDS):
        for tag in (("other", "this") if rnd % 2 == 0 else ("this", "other")):      # (neither build always runs second)
            env = dict(os.environ)
            env.pop("LINNA_LIB_PATH", None)
            if tag == "other":
                env["LINNA_LIB_PATH"] = os.path.abspath(other)
            elif "--this" in sys.argv:
                env["LINNA_LIB_PATH"] = os.path.abspath(sys.argv[sys.argv.index("--this") + 1])
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--repeats", str(REPEATS), "--trans", str(TRANS)] + scalar,
                               env=env, stdout=subprocess.PIPE, universal_newlines=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("child (%s) failed with %d" % (tag, p.returncode))
            runs[tag].append(json.loads(p.stdout.strip().splitlines()[-1])["rates"])
    res = {}
    for route in ("step_loop",) if scalar else ("step_loop", "run"):
        res[route] = {}
        for key in runs["this"][0]:
            a = sorted(r[key][route]["per_s"] for r in runs["this"])
            b = sorted(r[key][route]["per_s"] for r in runs["other"])
            res[route][key] = {"this_per_s": a, "other_per_s": b, "this_over_other": round(a[len(a) // 2] / b[len(b) // 2], 4)}
    return res


def main():
    if "--ab" in sys.argv:
        print(json.dumps({"tool": "hmc_run_bench", "mode": "ab", "other": sys.argv[sys.argv.index("--ab") + 1], "rounds": ROUNDS,
                          "trans": TRANS, "repeats": REPEATS, "routes": ab(sys.argv[sys.argv.index("--ab") + 1])}))
        return
    if "--dense" in sys.argv:
        rates, chol = measure_dense()
        print(json.dumps({"tool": "hmc_run_bench", "mode": "dense", "leapfrog_steps": NLEAP, "trans": TRANS, "repeats": REPEATS,
                          "rates": rates, "chol_from_comoments": chol}))
        return
    if "--moments" in sys.argv:
        print(json.dumps({"tool": "hmc_run_bench", "mode": "moments", "leapfrog_steps": NLEAP, "trans": TRANS, "repeats": REPEATS,
                          "rates": measure_moments()}))
        return
    scalar_only ="--scalar-only" in sys.argv
    print(json.dumps({"tool": "hmc_run_bench", "leapfrog_steps": NLEAP, "trans": TRANS, "repeats": REPEATS,
                      "scalar_only": scalar_only, "rates": measure(scalar_only)}))


if __name__ == "__main__":
    main()
