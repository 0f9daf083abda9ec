"""Float64 emulation of lnP and d lnP / d z of the bf16 one-launch gradient (linna_logprob_set_grad_precision,
net_stream.hip net_stream_grad_bf16_kernel), built on tests/bf16_emul.py (forward) and the backward stages of
tests/bf16_train_emul.py.

TEST INFRASTRUCTURE ONLY.  It rounds exactly where the kernel rounds and nowhere else:
  * every packed weight, forward and transposed, to bf16 nearest-even AFTER the fp32 folding (a residual block's second K
    part is fp32(0.1f * W2) in both halves: one bf16 value per weight);
  * the network input as x_hi = bf16(x) and x_lo = x - x_hi against [W | W]; every later A operand of the forward half and
    every delta of the backward half, to bf16 where the matrix cores read it;
  * the gates are the signs of the ROUNDED forward's activations (a residual block's hidden t and every op output that
    went through a ReLU).
Not rounded (fp32 on the GPU, float64 here): bias, ReLU, the turnaround d lnP / d out = -(d w) gscale / T from the output
map and the diagonal likelihood, the input transform's and the prior map's derivative, the -z of the Gaussian prior term.
rounded=False: the exact network and its exact gradient on the same fp32 input and fp32 parameters.
"""
import numpy as np

from oracle import emulator, likelihood
from bf16_emul import bf16

f64 = lambda a: np.asarray(a, np.float64)
f32 = lambda a: np.asarray(a, np.float32)


def network_fwd_bwd(params, x32, kind, nin, nout, dout_of, rounded=True, **kw):
    """(h, dx): the network output h [B, nout] on the fp32 input rows x32 and d/dx of the scalar whose derivative with
    respect to h is dout_of(h) (float64, not rounded: the turnaround)."""
    R = bf16 if rounded else (lambda a: f32(a))
    ops = emulator.topology(kind, nin, nout, **kw)
    x32 = f32(x32)
    acts = []                                   # per op: (hidden t or None, output y), float64, unrounded
    h = f64(x32)
    for i, op in enumerate(ops):
        if op[0] == "linear":
            _, key, K, N, relu = op
            W = f64(R(f32(params[key + ".weight"])))
            b = f64(f32(params[key + ".bias"]))
            if i == 0 and rounded:
                hi = bf16(x32)
                y = f64(hi) @ W.T + f64(bf16(x32 - hi)) @ W.T + b
            else:
                y = f64(R(f32(h))) @ W.T + b
            if relu:
                y = np.maximum(y, 0.0)
            acts.append((None, y))
        elif op[0] == "resblock":
            _, key, K, C, N = op
            a = f64(R(f32(h)))
            t = np.maximum(a @ f64(R(f32(params[key + ".layer1.weight"]))).T + f64(f32(params[key + ".layer1.bias"])), 0.0)
            W2 = f64(R(np.float32(0.1) * f32(params[key + ".layer2.weight"])))
            b2 = f64(np.float32(0.1) * f32(params[key + ".layer2.bias"]))
            skip = a @ f64(R(f32(params[key + ".skip_layer.weight"]))).T if K != N else a
            y = np.maximum(skip + f64(R(f32(t))) @ W2.T + b2, 0.0)
            acts.append((t, y))
        else:
            raise ValueError("no one-launch gradient for an input-skip network")
        h = y
    out = h
    dY = f64(dout_of(out))
    for i in range(len(ops) - 1, -1, -1):
        op = ops[i]
        t = acts[i][0]
        dR = f64(R(f32(dY)))
        if op[0] == "linear":
            dX = dR @ f64(R(f32(params[op[1] + ".weight"])))
        else:
            _, key, K, C, N = op
            dT = dR @ f64(R(np.float32(0.1) * f32(params[key + ".layer2.weight"])))
            dT = np.where(t > 0, dT, 0.0)
            skip = dR @ f64(R(f32(params[key + ".skip_layer.weight"]))) if K != N else dR
            dX = skip + f64(R(f32(dT))) @ f64(R(f32(params[key + ".layer1.weight"])))
        if i > 0 and (ops[i - 1][0] == "resblock" or ops[i - 1][4]):
            dX = np.where(acts[i - 1][1] > 0, dX, 0.0)          # the gate: op i's input went through a ReLU
        dY = dX
    return out, dY


def log_prob_grad(z, prob, w, temperature, rounded=True):
    """(lnP[B], G[B, nin]) of the serving problem `prob` (tests/cases.py) with the DIAGONAL inverse covariance w: the
    linear output map only (an exp map has no gradient path)."""
    if prob["ypositive"]:
        raise ValueError("the exp output map has no gradient path")
    z64 = np.atleast_2d(f64(z))
    theta = likelihood.prior_map(z64, prob["priors"])
    x = likelihood.x_transform(theta, f64(prob["X_mean"]), f64(prob["X_std"]), prob["dolog10"])
    ys, ym, sig, data, w = f64(prob["y_std"]), f64(prob["y_mean"]), f64(prob["sigma"]), f64(prob["data"]), f64(w)
    resid = lambda h: (h * ys + ym) * sig - data
    dout = lambda h: -(resid(h) * w) * (ys * sig) / temperature
    h, dx = network_fwd_bwd(prob["weights"], f32(x), prob["kind"], prob["nin"], prob["nout"], dout, rounded=rounded, **prob["kw"])
    d = resid(h)
    lnp = -0.5 * (d * d * w[None, :]).sum(-1) / temperature - 0.5 * (z64 * z64).sum(-1)
    dtheta = dx / f64(prob["X_std"])[None, :]
    if prob["dolog10"] is not None:
        for i in prob["dolog10"]:
            dtheta[:, i] = dtheta[:, i] / (theta[:, i] * np.log(10.0))
    G = dtheta * likelihood.prior_map_grad(z64, prob["priors"]) - z64
    return np.where(np.isnan(lnp), -np.inf, lnp), G
