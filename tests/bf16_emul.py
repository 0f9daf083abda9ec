"""Float64 emulation of the whole-network kernel's bf16 serving engine (linna_logprob_set_precision, net_stream.hip BF).

TEST INFRASTRUCTURE ONLY.  It rounds exactly where the kernel rounds and nowhere else:
  * every packed weight, to bf16 nearest-even, AFTER the fp32 folding the packer does: a residual block's second K part
    is fp32(0.1f * W2), an input skip's is fp32(alpha * Wl); biases are fp32 (0.1f * b2, b8 + alpha bl) and not rounded;
  * every A operand (the fp32 activation the matrix cores read), to bf16 nearest-even;
  * the network input x (fp32) as x_hi = bf16(x) and x_lo = x - x_hi, both read by the first layer [W | W].
Everything else -- sums, bias, ReLU, the output map, the log-likelihood, the prior map -- is float64 here, fp32 on the
GPU: those differences are orders of magnitude below the bf16 roundings this module exists to pin down.
"""
import numpy as np

from oracle import emulator, likelihood


def bf16(a):
    """Round float32 values to the nearest bf16 (ties to even), returned as float32.  (NaN inputs are not expected.)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def _f32(a):
    return np.asarray(a, np.float32)


def network(params, x32, kind, nin, nout, rounded=True, **kw):
    """The network on the fp32 input rows x32 [B, nin], float64 arithmetic.  rounded=False: no rounding at all (the exact
    network on the same fp32 input and fp32 parameters)."""
    R = bf16 if rounded else (lambda a: _f32(a))
    f64 = lambda a: np.asarray(a, np.float64)
    x32 = _f32(x32)
    first = True
    h = None
    ops = emulator.topology(kind, nin, nout, **kw)
    for op in ops:
        if op[0] == "linear":
            _, key, K, N, relu = op
            W = R(_f32(params[key + ".weight"]))
            b = f64(_f32(params[key + ".bias"]))
            if first:
                if rounded:
                    hi = bf16(x32)
                    lo = bf16(x32 - hi)                    # x - x_hi is exact in fp32; rounded again where it is read
                    y = f64(hi) @ f64(W).T + f64(lo) @ f64(W).T + b
                else:
                    y = f64(x32) @ f64(W).T + b
            else:
                y = f64(R(_f32(h))) @ f64(W).T + b
            if relu:
                y = np.maximum(y, 0.0)
        elif op[0] == "resblock":
            _, key, K, C, N = op
            a = f64(R(_f32(h)))
            W1 = R(_f32(params[key + ".layer1.weight"]))
            t = np.maximum(a @ f64(W1).T + f64(_f32(params[key + ".layer1.bias"])), 0.0)
            W2 = R(np.float32(0.1) * _f32(params[key + ".layer2.weight"]))                  # alpha folded in fp32, then rounded
            b2 = f64(np.float32(0.1) * _f32(params[key + ".layer2.bias"]))
            skip = a @ f64(R(_f32(params[key + ".skip_layer.weight"]))).T if K != N else a
            y = np.maximum(skip + f64(R(_f32(t))) @ f64(W2).T + b2, 0.0)
        else:                                          # input skip: ONE GEMM over [h ; x0] with [W8 | alpha Wl] (see above)
            _, key, K, N, scale = op
            al = np.float32(scale)
            Wl = R(al * _f32(params[key + ".weight"]))
            bl = f64(al * _f32(params[key + ".bias"]))
            y = h + f64(R(x32)) @ f64(Wl).T + bl       # h: layer8's output (its own bias included); x0 read as bf16
        first = False
        h = y
    return h


def log_prob(z, prob, w, temperature, rounded=True):
    """lnP[B] of the serving problem `prob` (tests/cases.py) with the DIAGONAL inverse covariance w, in float64 from the
    fp32 network input the kernel's prologue forms."""
    z64 = np.atleast_2d(np.asarray(z, np.float64))
    theta = likelihood.prior_map(z64, prob["priors"])
    x = likelihood.x_transform(theta, np.asarray(prob["X_mean"], np.float64), np.asarray(prob["X_std"], np.float64), prob["dolog10"])
    h = network(prob["weights"], _f32(x), prob["kind"], prob["nin"], prob["nout"], rounded=rounded, **prob["kw"])
    y = likelihood.y_transform(h, np.asarray(prob["y_mean"], np.float64), np.asarray(prob["y_std"], np.float64), prob["ypositive"])
    d = y * np.asarray(prob["sigma"], np.float64)[None, :] - np.asarray(prob["data"], np.float64)[None, :]
    out = -0.5 * (d * d * np.asarray(w, np.float64)[None, :]).sum(-1) / temperature - 0.5 * (z64 * z64).sum(-1)
    return np.where(np.isnan(out), -np.inf, out)


def abs_network(params, x, kind, nin, nout, **kw):
    """A_L of the absolute-value network: A_0 = |x|, each op with |W| and |b| (ReLU dropped): the first-order bound of what
    rounding every operand of every matrix product by a relative 2^-9 can move each output, per unit of 2 * 2^-9 per stage."""
    h = np.abs(np.asarray(x, np.float64))
    s0 = h
    for op in emulator.topology(kind, nin, nout, **kw):
        A = lambda k: np.abs(np.asarray(params[k], np.float64))
        if op[0] == "linear":
            _, key, K, N, relu = op
            h = h @ A(key + ".weight").T + A(key + ".bias")
        elif op[0] == "resblock":
            _, key, K, C, N = op
            t = h @ A(key + ".layer1.weight").T + A(key + ".layer1.bias")
            skip = h @ A(key + ".skip_layer.weight").T if K != N else h
            h = skip + 0.1 * (t @ A(key + ".layer2.weight").T + A(key + ".layer2.bias"))
        else:
            _, key, K, N, scale = op
            h = h + scale * (s0 @ A(key + ".weight").T + A(key + ".bias"))
    return h


def stages(kind, nin, nout, **kw):
    """Matrix products on the longest path from the input to the output (each one a rounding stage)."""
    n = 0
    for op in emulator.topology(kind, nin, nout, **kw):
        n += 2 if op[0] == "resblock" else 1 if op[0] == "linear" else 0
    return n
