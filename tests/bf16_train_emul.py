"""Float64 emulation of ONE bf16 training step of the whole-network kernel (linna_net_set_train_precision,
net_stream.hip BF + TRB), extending tests/bf16_emul.py.

TEST INFRASTRUCTURE ONLY.  It rounds exactly where the kernel rounds and nowhere else:
  * the forward as bf16_emul.network: every packed weight to bf16 after the fp32 folding (0.1 W2), every A operand to bf16,
    the input as x_hi = bf16(x) + x_lo = x - x_hi against [W | W]; the activations it keeps are the UNROUNDED ones;
  * the loss segment is fp32 inside the bf16 launch: delta = ynorm - pred, U = delta Cinv, loss_b = delta . U / den,
    d loss / d pred = -2 U inv_batch / den (zero where the target is masked) -- not rounded at all;
  * the dX chain reads bf16(W^T) (a residual block's 0.1 W2 folded first) and bf16(dY) where the matrix cores read them,
    and gates by the stored activation > 0;
  * the parameter gradients dW = A^T dY are fp32 GEMMs on the UNROUNDED stored A and dY.
rounded=False: the same step with no rounding at all.
"""
import numpy as np

from oracle import emulator
from bf16_emul import bf16

f64 = lambda a: np.asarray(a, np.float64)
f32 = lambda a: np.asarray(a, np.float32)


def train_step(params, x32, kind, nin, nout, YN, den, inv_batch, Cinv, rounded=True, acts_out=None, **kw):
    """One step on the fp32 input rows x32 [B, nin] (the transformed batch the kernel stores), normalised targets YN [B, nout]
    (NaN = masked), per-row denominators den [B], Cinv [nout, nout].  Returns (loss_rows, dpred, grads {state-dict key: array})."""
    R = bf16 if rounded else (lambda a: f32(a))
    ops = emulator.topology(kind, nin, nout, **kw)
    x32 = f32(x32)
    acts = []                                   # per op: (input, hidden t or None, output), float64, unrounded
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
            acts.append((h, None, y))
        elif op[0] == "resblock":
            _, key, K, C, N = op
            a = f64(R(f32(h)))
            t = np.maximum(a @ f64(R(f32(params[key + ".layer1.weight"]))).T + f64(f32(params[key + ".layer1.bias"])), 0.0)
            W2 = f64(R(np.float32(0.1) * f32(params[key + ".layer2.weight"])))
            b2 = f64(np.float32(0.1) * f32(params[key + ".layer2.bias"]))
            skip = a @ f64(R(f32(params[key + ".skip_layer.weight"]))).T if K != N else a
            y = np.maximum(skip + f64(R(f32(t))) @ W2.T + b2, 0.0)
            acts.append((h, t, y))
        else:
            raise ValueError("no bf16 training step for an input-skip network")
        h = y
    pred = h
    if acts_out is not None:
        acts_out.extend(acts)
    YN = f64(YN)
    mask = np.isnan(YN)
    delta = np.where(mask, 0.0, YN - pred)
    U = delta @ f64(Cinv).T
    den = f64(den)
    loss_rows = (delta * U).sum(1) / den
    dpred = np.where(mask, 0.0, -2.0 * U * inv_batch / den[:, None])
    grads = {}
    dY = dpred
    for i in range(len(ops) - 1, -1, -1):
        op = ops[i]
        A, t, _ = acts[i]
        gate = (A > 0) if i > 0 and (ops[i - 1][0] == "resblock" or ops[i - 1][4]) else None
        if op[0] == "linear":
            key = op[1]
            grads[key + ".weight"] = dY.T @ A
            grads[key + ".bias"] = dY.sum(0)
            if i > 0:
                dX = f64(R(f32(dY))) @ f64(R(f32(params[key + ".weight"])))
        else:
            _, key, K, C, N = op
            dR = f64(R(f32(dY)))
            dT = dR @ f64(R(np.float32(0.1) * f32(params[key + ".layer2.weight"])))
            dT = np.where(t > 0, dT, 0.0)
            grads[key + ".layer2.weight"] = 0.1 * (dY.T @ t)
            grads[key + ".layer2.bias"] = 0.1 * dY.sum(0)
            grads[key + ".layer1.weight"] = dT.T @ A
            grads[key + ".layer1.bias"] = dT.sum(0)
            if K != N:
                grads[key + ".skip_layer.weight"] = dY.T @ A
            if i > 0:
                skip = dR @ f64(R(f32(params[key + ".skip_layer.weight"]))) if K != N else dR
                dX = skip + f64(R(f32(dT))) @ f64(R(f32(params[key + ".layer1.weight"])))
        if i > 0:
            dY = np.where(gate, dX, 0.0) if gate is not None else dX
    return loss_rows, dpred, grads


def stage_grads(params, kind, nin, nout, acts, dys, dts, dpred, rounded=True, **kw):
    """The parameter gradients ONE rounding stage at a time, from the kernel's own stored tensors: acts[i] = (input, t, output)
    of op i, dys[i] = d loss / d (input of op i) as the launch stored it (gated; i >= 1), dts[i] = d loss / d t of a residual
    block, dpred = d loss / d pred.  Op i's parameter gradient is formed from the dY the emulation derives from the stored
    dY of op i + 1 (one dX stage: bf16(W^T), bf16(dY) where the kernel rounds) and the stored A -- so the fp32 noise of
    earlier stages, which can move an operand across a bf16 rounding boundary and compound over a deep chain, is not
    compared; every stage is.  The last op's gradient has no stage of its own (dpred is fp32) and is left out."""
    R = bf16 if rounded else (lambda a: f32(a))
    ops = emulator.topology(kind, nin, nout, **kw)
    grads = {}
    for i in range(len(ops) - 2, -1, -1):
        op, nx = ops[i], ops[i + 1]
        up = f64(dpred) if i + 1 == len(ops) - 1 else f64(dys[i + 2])      # stored d loss / d (output of op i + 1)
        dR = f64(R(f32(up)))
        if nx[0] == "linear":
            dX = dR @ f64(R(f32(params[nx[1] + ".weight"])))
        else:
            _, key, K, C, N = nx
            skip = dR @ f64(R(f32(params[key + ".skip_layer.weight"]))) if K != N else dR
            dX = skip + f64(R(f32(dts[i + 1]))) @ f64(R(f32(params[key + ".layer1.weight"])))
        A, t, y = acts[i]
        dY = np.where(f64(y) > 0, dX, 0.0)                  # op i's output went through a ReLU (resblock or relu linear)
        A = f64(A)
        if op[0] == "linear":
            grads[op[1] + ".weight"] = dY.T @ A
            grads[op[1] + ".bias"] = dY.sum(0)
        else:
            _, key, K, C, N = op
            dT = f64(R(f32(dys[i + 1]))) @ f64(R(np.float32(0.1) * f32(params[key + ".layer2.weight"])))   # (from the stored dY)
            dT = np.where(f64(t) > 0, dT, 0.0)
            grads[key + ".layer2.weight"] = 0.1 * (dY.T @ f64(t))
            grads[key + ".layer2.bias"] = 0.1 * dY.sum(0)
            grads[key + ".layer1.weight"] = dT.T @ A
            grads[key + ".layer1.bias"] = dT.sum(0)
            if K != N:
                grads[key + ".skip_layer.weight"] = dY.T @ A
    return grads
