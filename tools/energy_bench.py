#!/usr/bin/env python
"""What the energy diagnostics of ``method="hmc"`` cost: transitions per second of ``BatchedHMC.run`` (5 leapfrog steps,
ChtoModelv2(33,33), fp32 and the bf16 gradient engine, 128 and 4096 chains) with the diagnostics off (linna_hmc_run) and on
(linna_hmc_run_energy: the accumulators and the divergence counts, and with the E / dH rows written as the driver asks for
them), the routes alternating in one process, `--repeats` timed windows each; and the device time of one
linna_hmc_energy_finish launch.  Host clock around work that ends in a device synchronise.  Prints ONE JSON line.

  python tools/energy_bench.py [--repeats N] [--trans N]
  python tools/energy_bench.py --off-only            only ``run()`` with the diagnostics off (what the A/B below runs in its children)
  python tools/energy_bench.py --ab OTHER_LIB.so     the "off" rate under this tree's library and under another build of it (the
        parent commit's: the Metropolis kernel has gained arguments, which must cost the existing route nothing), alternating,
        each in a fresh process (LINNA_LIB_PATH), `--rounds` of both; `--this THIRD_LIB.so` puts a third build in this tree's
        place (two copies of one build against each other: the spread of the comparison itself)
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


REPEATS, TRANS, ROUNDS = _arg("--repeats", 7), _arg("--trans", 200), _arg("--rounds", 3)
NLEAP, EPS = 5, 1e-3


def _stats(v):
    v = sorted(v)
    return {"per_s": round(v[len(v) // 2], 1), "min": round(v[0], 1), "max": round(v[-1], 1)}


def measure(off_only):
    import numpy as np
    import torch
    import bf16_bench
    from linna_amd import _lib, sampler, util
    if os.environ.get("LINNA_LIB_PATH"):                      # another build of the library: bind what it exports
        _lib.load(missing_ok=True)
    dev = torch.device("cuda", 0)
    lp32 = bf16_bench.v2_problem(dev)
    forms = {"fp32": lp32, "bf16": util.Log_prob(lp32.data_new, lp32.invcov_new, lp32.model, lp32.y_invtransform_data, lp32.transform,
                                                  lp32.T, lp32.loglikelihoodfunc, nograd=True, precision="bf16", grad_precision="bf16")}
    out = {}
    for prec, lp in forms.items():
        for B in (128, 4096):
            x0 = (0.2 * np.random.RandomState(B).standard_normal((B, 33))).astype(np.float32)
            off = sampler.BatchedHMC(lp, x0, seed=5)
            off.eps.fill_(EPS)
            routes = {"off": lambda: off.run(TRANS, NLEAP, store=False)}
            if not off_only:
                on = sampler.BatchedHMC(lp, x0, seed=5)
                on.eps.fill_(EPS)
                on.energy_stats(True)
                routes["on"] = lambda: on.run(TRANS, NLEAP, store=False)
                routes["on_rows"] = lambda: on.run(TRANS, NLEAP, store=False, energy=True)
            for fn in routes.values():                        # warm-up: every route
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
            if not off_only:
                us = lambda k: 1e6 / r[k]["per_s"]
                r["on_over_off"] = round(r["on"]["per_s"] / r["off"]["per_s"], 4)
                r["on_us_per_transition"] = round(us("on") - us("off"), 3)
                r["on_rows_us_per_transition"] = round(us("on_rows") - us("off"), 3)
                fin = []
                for _ in range(20):                           # one finish launch, device clock
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); on.energy_finish(); b.record()
                    torch.cuda.synchronize()
                    fin.append(1e3 * a.elapsed_time(b))
                fin.sort()
                r["finish_us"] = {"us": round(fin[len(fin) // 2], 1), "min": round(fin[0], 1), "max": round(fin[-1], 1)}
            out["ChtoModelv2_33_33_%s_%d" % (prec, B)] = r
    return out


def ab(other):
    runs = {"this": [], "other": []}
    for rnd in range(ROUNDS):
        for tag in (("other", "this") if rnd % 2 == 0 else ("this", "other")):      # (neither build always runs second)
            env = dict(os.environ)
            env.pop("LINNA_LIB_PATH", None)
            if tag == "other":
                env["LINNA_LIB_PATH"] = os.path.abspath(other)
            elif "--this" in sys.argv:
                env["LINNA_LIB_PATH"] = os.path.abspath(sys.argv[sys.argv.index("--this") + 1])
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--off-only", "--repeats", str(REPEATS), "--trans", str(TRANS)],
                               env=env, stdout=subprocess.PIPE, universal_newlines=True, timeout=300)
            if p.returncode != 0:
                raise SystemExit("child (%s) failed with %d" % (tag, p.returncode))
            runs[tag].append(json.loads(p.stdout.strip().splitlines()[-1])["rates"])
    res = {}
    for key in runs["this"][0]:
        a = sorted(r[key]["off"]["per_s"] for r in runs["this"])
        b = sorted(r[key]["off"]["per_s"] for r in runs["other"])
        res[key] = {"this_per_s": a, "other_per_s": b, "this_over_other": round(a[len(a) // 2] / b[len(b) // 2], 4)}
    return res


def main():
    if "--ab" in sys.argv:
        other = sys.argv[sys.argv.index("--ab") + 1]
        print(json.dumps({"tool": "energy_bench", "mode": "ab", "other": other, "rounds": ROUNDS, "trans": TRANS, "repeats": REPEATS,
                          "off": ab(other)}))
        return
    off_only = "--off-only" in sys.argv
    print(json.dumps({"tool": "energy_bench", "leapfrog_steps": NLEAP, "trans": TRANS, "repeats": REPEATS, "off_only": off_only,
                      "rates": measure(off_only)}))


if __name__ == "__main__":
    main()
