#!/usr/bin/env python
"""fp32 against the opt-in bf16 training step (linna_net_set_train_precision), one process, device events, after warm-up,
the two precisions alternating block by block:
  step_<net>     one optimiser step through linna_net_train_step_update (the merged launch + the grouped parameter-gradient
                 launch with AdamW in its epilogue), batch 500
  grad_<net>     the same without the optimiser (linna_net_train_step: merged launch + grouped gradients)
  epoch_v2_457   one Predictor.train epoch (20 steps of 500 rows, the validation pass, the controller): the wall time of a
                 6-epoch run over 6, mean of two runs after one not counted
for ChtoModelv2(26,457) with its dense loss covariance (BASELINE configs[2]'s shape), ChtoModelv2(33,33) and the 4 x 512 MLP
(33,33).  The merged launch alone is timed by rocprofv3 --kernel-trace --stats in a run of its own (tools/README.md).
Prints ONE JSON line.  usage: python tools/bf16_train_bench.py [--reps N] [--nets v2_457,v2_33,mlp_33] [--no-epoch]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")]
import synth  # noqa: E402
from linna_amd import nn, predictor_gpu, trainer, util  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 200
B = 500
NETS = {"v2_457": ("ChtoModelv2", 26, 457, 205), "v2_33": ("ChtoModelv2", 33, 33, 203), "mlp_33": ("MLP", 33, 33, 207)}
RUN = sys.argv[sys.argv.index("--nets") + 1].split(",") if "--nets" in sys.argv else list(NETS)


def problem(kind, nin, nout, seed, n):
    rs = np.random.RandomState(seed + 31)
    data, cov, _ = synth.gaussian_problem(nin, nout, seed, dense=True, cond=1e2)
    X_mean, X_std, y_mean, y_std = synth.transform_constants(nin, nout, seed)
    X = (X_mean[None, :] + X_std[None, :] * rs.standard_normal((n, nin))).astype(np.float32)
    Y = (data[None, :] + 3 * np.sqrt(np.diag(cov))[None, :] * rs.standard_normal((n, nout))).astype(np.float32)
    return data, cov, X_mean, X_std, y_mean, y_std, X, Y


def engine(name, precision, n=3 * B):
    kind, nin, nout, seed = NETS[name]
    data, cov, X_mean, X_std, y_mean, y_std, X, Y = problem(kind, nin, nout, seed, n)
    model = (nn.MLP if kind == "MLP" else nn.ChtoModelv2)(nin, nout, None)
    model.load_state_dict(synth.weights(kind, nin, nout, seed))
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    pred = predictor_gpu.Predictor(nin, nout, model=model, device="cuda",
                                   X_transform=util.X_transform_class(t(X_mean), t(X_std), "cpu", None),
                                   y_transform=util.Y_transform_class(t(y_mean), t(y_std), "cpu"))
    sigma = np.sqrt(np.diag(cov))
    lf = util.Loss_fn(t(data), torch.tensor(cov, dtype=torch.float64), torch.tensor(np.linalg.inv(cov), dtype=torch.float64),
                      util.Y_transform_data(sigma, "cpu"), util.Y_invtransform_class(t(y_mean), t(y_std), t(data), "cpu"), "cpu")
    vm = util.Val_metric_fn(t(data), torch.tensor(cov, dtype=torch.float64), torch.tensor(np.linalg.inv(cov), dtype=torch.float64),
                            util.Y_transform_data(sigma, "cpu"), util.Y_invtransform_class(t(y_mean), t(y_std), t(data), "cpu"), "cpu")
    loader = predictor_gpu.BatchLoader(util.ArrayDataset(X, Y), B, shuffle=False, drop_last=True)
    if n > 3 * B:
        return pred, lf, vm, loader
    return trainer.TrainEngine(pred, loader, lf, None, use_graph=False, precision=precision)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(reps):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps          # us per call


def main():
    res = {"tool": "bf16_train_bench", "reps": REPS, "batch": B}
    rows = [torch.arange(k * B, (k + 1) * B, dtype=torch.int32, device="cuda") for k in range(3)]
    for name in RUN:
        eng, opt = {}, {}
        for prec in ("fp32", "bf16"):
            e = engine(name, prec)
            eng[prec], opt[prec] = e, predictor_gpu._AdamWState(e.model, 1e-4)
            for i in range(20):                       # warm-up: code objects, stream layouts, the first-step decisions
                e.step(opt[prec], rows[i % 3])
                e._forward_loss_backward(rows[i % 3], None, None, update=False)
        torch.cuda.synchronize()
        step, grad = {"fp32": [], "bf16": []}, {"fp32": [], "bf16": []}
        for _ in range(4):                            # alternating blocks
            for prec in ("fp32", "bf16"):
                e, o = eng[prec], opt[prec]
                step[prec].append(timed(lambda i: e.step(o, rows[i % 3]), REPS))
                grad[prec].append(timed(lambda i: e._forward_loss_backward(rows[i % 3], None, None, update=False), REPS))
        for prec in ("fp32", "bf16"):
            assert eng[prec].one_update is True and eng[prec].one_launch is True, (name, prec)
            res["step_%s_%s_us" % (name, prec)] = round(float(np.median(step[prec])), 2)
            res["grad_%s_%s_us" % (name, prec)] = round(float(np.median(grad[prec])), 2)
        res["step_%s_speedup" % name] = round(res["step_%s_fp32_us" % name] / res["step_%s_bf16_us" % name], 3)
    # one Predictor.train epoch at (26,457): 10000 training rows (20 steps), 500 validation rows
    ep = {"fp32": [], "bf16": []}
    for rep in range(0 if "--no-epoch" in sys.argv else 3):      # (the first pair: one-time set-up, not counted)
        for prec in ("fp32", "bf16"):
            pred, lf, vm, loader = engine("v2_457", prec, n=10000)
            kind, nin, nout, seed = NETS["v2_457"]
            *_, Xv, Yv = problem(kind, nin, nout, seed + 1, 500)
            val = predictor_gpu.BatchLoader(util.ArrayDataset(Xv, Yv), 500, shuffle=False, drop_last=False)
            pred.optim = type("FixedLR", (), {"lr": 1e-4})()      # a fixed learning rate: no range test in the timing
            t0 = time.perf_counter()
            pred.train(loader, 6, lf, val, vm, precision=prec)
            torch.cuda.synchronize()
            if rep:
                ep[prec].append((time.perf_counter() - t0) / 6)
    for prec in ("fp32", "bf16"):
        if ep[prec]:
            res["epoch_v2_457_%s_ms" % prec] = round(1e3 * float(np.median(ep[prec])), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
