"""Exact integer tables and integer references for the whole-network kernel (tests/test_net_exact_host.py pins them on the
CPU, tests/test_gpu_net_exact.py runs net_stream.hip, its planner and its pack kernel against them).  Not a test module.

The technique of tests/entries_ref.py carried to whole networks: every weight, bias, input and constant is a small integer
(or an integer times one power of two), so every fp32 product and every partial sum is exact, the result does not depend on
the engine, the K split or the order of summation, and equals the integer reference BIT FOR BIT.  A residual block's fixed
0.1 is folded into the packed weight by the planner (``alpha * Wb``, ``bscale * b``): ``layer2.weight`` / ``layer2.bias`` are
stored as 10 x an integer, and float32(0.1) * float32(10 m) rounds to exactly m.

A table (network, dense map m, B rows) has ONE dense map -- the map under test: every weight position from {-1, +1}, an
integer bias.  Every other linear map is a sparse routing map:
 * before the dense map a row sums a few columns with +1 (bias 0); the network input is zero but for a few columns per row
   (column j is live in row b iff j = b mod P), so that the dense map's input is sparse in every row -- its outputs stay small --
   and every one of its input columns is non-zero in some row;
 * behind the dense map a row has +1 and -1 entries in alternation and a bias from {-1, 0, 1}: the layers whose ReLU gates get
   exercised (zero is exact here: no kink exemption).
The dense map rotates over every linear map of the network (three per residual block: W1, W2, Ws).
The bf16 engines (linna_logprob_set_precision, linna_logprob_set_grad_precision, linna_net_set_train_precision) are tested
on the same tables: every fp32 partial sum is exact, so every value a bf16 engine rounds is known exactly, round-to-nearest-
even of it is deterministic, and a reference that rounds where include/linna_hip.h says the engine rounds equals the GPU bit
for bit.  ``forward_ref``, ``backward_ref`` and ``serving_ref`` take that rounding as a hook (``Bf16Hook``; default: none).
Every table is a pure function of its key.  The references are written from the definitions (y = relu(W x + b); the residual
block of nn.py:45-56 with 0.1 as an integer division of the stored weight; the chain rule) in float64 on integers.
"""
import numpy as np

from entries_ref import F, T_EXACT, f64, rng
from linna_amd import _lib, nn

L, R = _lib.OP_LINEAR, _lib.OP_RESBLOCK


# ----------------------------------------------------------------------------------------------- networks
class ExactNet(nn._Emulator):
    """A network from an arbitrary op list: ("L", K, N, relu) and ("R", K, C, N) (K == N: the identity skip)."""

    def __init__(self, spec):
        self._spec = tuple(spec)
        nn._Emulator.__init__(self, spec[0][1], spec[-1][3] if spec[-1][0] == "R" else spec[-1][2], None)

    def _build_ops(self):
        ops = []
        for i, s in enumerate(self._spec):
            if s[0] == "L":
                ops.append(nn._Op(L, "op%d" % i, s[1], s[2], relu=int(s[3])))
            else:
                ops.append(nn._Op(R, "op%d" % i, s[1], s[3], C=s[2]))
        return ops


def mlp(nin, widths, nout):
    spec, k = [], nin
    for w in widths:
        spec.append(("L", k, w, 1))
        k = w
    return spec + [("L", k, nout, 0)]


# name -> ("v2" | "simple", nin, nout) or ("custom", spec)
NETS = {
    # ---- plain MLPs: K tail, first-layer padding, column groups, the SPLIT / WIDE choice, passes
    "in1_n1": ("custom", mlp(1, [1], 1)),
    "in15_n16": ("custom", mlp(15, [16], 17)),
    "in16_n17": ("custom", mlp(16, [17], 16)),
    "in17_n32": ("custom", mlp(17, [32, 33], 3)),
    "in64_n64": ("custom", mlp(64, [64, 65], 64)),
    "in65_n128": ("custom", mlp(65, [128, 129], 5)),
    "in256_n256": ("custom", mlp(256, [256, 257], 9)),
    "n512_513": ("custom", mlp(9, [512, 513], 33)),
    "n1000_1024": ("custom", mlp(5, [1000, 1024], 40)),
    "split_4k": ("custom", mlp(8, [64, 128], 4)),               # 128 <- 64: 4 k steps, split_steps + 3 <= 4: SPLIT
    "wide_3k": ("custom", mlp(8, [48, 128], 4)),                # 128 <- 48: 3 k steps: WIDE
    # ---- SIDE segments on the 16-row engine: kc 4 / 2 / 1 (<= 16 / 32 / 64 columns), one step, two steps, one past (SPLIT)
    "side16_1": ("custom", mlp(7, [500, 16], 3)),
    "side16_2": ("custom", mlp(7, [1000, 16], 3)),
    "side32_1": ("custom", mlp(7, [250, 32], 3)),
    "side32_2": ("custom", mlp(7, [500, 32], 3)),
    "side32_3": ("custom", mlp(7, [600, 32], 3)),
    "side64_1": ("custom", mlp(7, [128, 64], 3)),
    "side64_2": ("custom", mlp(7, [250, 64], 3)),
    "side64_3": ("custom", mlp(7, [300, 64], 3)),
    # ---- gradient gates: fused MLP gradient (hidden N > 256), one and two mask slots, nin = nout = 64
    "grad257": ("custom", mlp(64, [257, 257], 64)),
    "grad513": ("custom", mlp(5, [513, 513], 3)),
    # ---- residual networks
    "v2_33_33": ("v2", 33, 33),
    "v2_5_1": ("v2", 5, 1),
    "v2_6_30": ("v2", 6, 30),
    "v2_6_31": ("v2", 6, 31),
    "v2_26_457": ("v2", 26, 457),
    "simple_6_4": ("simple", 6, 4),
    "simple_6_31": ("simple", 6, 31),
    "blk_c1": ("custom", [("L", 5, 17, 1), ("R", 17, 1, 40), ("L", 40, 3, 0)]),
    "blk_c16": ("custom", [("L", 5, 17, 1), ("R", 17, 16, 33), ("L", 33, 3, 0)]),
    "blk_c17": ("custom", [("L", 5, 40, 1), ("R", 40, 17, 20), ("L", 20, 3, 0)]),
    "blk_c64": ("custom", [("L", 5, 100, 1), ("R", 100, 64, 50), ("L", 50, 3, 0)]),
    "blk_id17": ("custom", [("L", 5, 17, 1), ("R", 17, 4, 17), ("L", 17, 3, 0)]),
    "blk_id64": ("custom", [("L", 9, 64, 1), ("R", 64, 16, 64), ("R", 64, 8, 64), ("L", 64, 5, 0)]),
    # ---- edges of the bf16 planner (32 k per step, no SIDE segments: tests/test_net_exact_host.py pins each from the planner)
    "k31_63": ("custom", mlp(6, [31, 63], 5)),                              # hidden K of 31 and 63: one slot short of 1 and 2 steps
    "bf_split_wide": ("custom", mlp(8, [128, 128, 96, 128], 4)),            # 128 <- 128: 4 steps of 32 k, SPLIT; 128 <- 96: 3, WIDE
    "bf_n64_k256_257": ("custom", mlp(7, [256, 64, 257, 64], 3)),           # 64 columns: one SPLIT step up to K = 256, two from 257
    "bf_n64_k512_513": ("custom", mlp(7, [512, 64, 513, 64], 3)),           # ... two up to 512, three from 513
    "bf_n32_k512_513": ("custom", mlp(7, [512, 32, 513, 32], 3)),           # 32 columns
    "bf_n16_k1024": ("custom", mlp(7, [1024, 16], 3)),                      # 16 columns behind K = 1024: four SPLIT steps
    "blk_k20_c31": ("custom", [("L", 5, 20, 1), ("R", 20, 31, 24), ("L", 24, 3, 0)]),   # [x (32) ; h (C)]: 63 k, two steps
    "blk_k20_c32": ("custom", [("L", 5, 20, 1), ("R", 20, 32, 24), ("L", 24, 3, 0)]),   # 64 k: two steps, the second one full
    "blk_k20_c33": ("custom", [("L", 5, 20, 1), ("R", 20, 33, 24), ("L", 24, 3, 0)]),   # 65 k: three
    "blk_k40_c15": ("custom", [("L", 5, 40, 1), ("R", 40, 15, 20), ("L", 20, 3, 0)]),   # [x (48) ; h (15)]: 63 k (blk_c17: 65)
    # ---- dense likelihood widths (one hidden layer in front)
    "dense16": ("custom", mlp(6, [64], 16)),
    "dense33": ("custom", mlp(8, [64, 64], 33)),                # the direct form's covariance segment is a SIDE one
    "dense64": ("custom", mlp(6, [64], 64)),
    "dense65": ("custom", mlp(6, [64], 65)),
    "dense256": ("custom", mlp(6, [64], 256)),
    "dense257": ("custom", mlp(6, [64], 257)),
    "dense512": ("custom", mlp(6, [64], 512)),
    "dense513": ("custom", mlp(6, [64], 513)),
    "dense960": ("custom", mlp(6, [64], 960)),
    "dense961": ("custom", mlp(6, [64], 961)),
    "dense1000": ("custom", mlp(6, [64], 1000)),
    "dense1024": ("custom", mlp(6, [64], 1024)),
}
DENSE_NETS = tuple(n for n in NETS if n.startswith("dense"))
BATCH_ROWS = (1, 3, 5, 9, 17, 33)
ENGINES = (4, 8, 16)

_models = {}


def model(name):
    """The network on the CPU (shapes, planner); ``fresh_model`` for one to move to the GPU."""
    if name not in _models:
        _models[name] = fresh_model(name)
    return _models[name]


def fresh_model(name):
    s = NETS[name]
    if s[0] == "v2":
        return nn.ChtoModelv2(s[1], s[2], None)
    if s[0] == "simple":
        return nn.ChtoModelsimple(s[1], s[2], None)
    return ExactNet(s[1])


def net_maps(ops):
    """Every linear map in forward order: (op index, role, weight key, bias key or None, N, K)."""
    out = []
    for i, op in enumerate(ops):
        if op.op == R:
            out.append((i, "W1", op.key + ".layer1.weight", op.key + ".layer1.bias", op.C, op.K))
            out.append((i, "W2", op.key + ".layer2.weight", op.key + ".layer2.bias", op.N, op.C))
            if op.K != op.N:
                out.append((i, "Ws", op.key + ".skip_layer.weight", None, op.N, op.K))
        else:
            out.append((i, "W", op.key + ".weight", op.key + ".bias", op.N, op.K))
    return out


ROWS = 20            # rows of a table where a test does not sweep them: two workgroups of the 16-row engine, the second ragged


# ----------------------------------------------------------------------------------------------- tables
def _route_pre(N, K, r, role):
    """Before the dense map: ONE +1 per row, at column n mod K (N >= K) or at columns spread over the K (N < K) -- a unit
    is the copy of one network input, small and live in the rows that input is live in.  A residual block's W2 has its
    +1 in one row of three only (the block's output is the skip's copy, plus h there)."""
    W = np.zeros((N, K))
    n = np.arange(N)
    col = n % K if N >= K else (n * (K // N) + (n % (K // N))) % K
    if role == "W2":
        n, col = n[::3], col[::3]
    W[n, col] = 1
    return W


def _route_post(N, K, r, role):
    """Behind the dense map: +1 at one column and, in two rows of three, -1 at another (inputs are >= 0 behind a ReLU: the
    difference is no larger than they are).  A residual block's W2: one entry per row, its sign alternating by row."""
    W = np.zeros((N, K))
    n = np.arange(N)
    col = n % K if N >= K else (n * (K // N) + (n % (K // N))) % K
    if role == "W2":
        W[n, col] = 1 - 2 * (n % 2)
        return W
    W[n, col] = 1
    other = (col + 1 + (n * 7) % max(K - 1, 1)) % K
    use = (other != col) & (r.randint(0, 3, N) > 0)
    W[n[use], other[use]] = -1
    return W


def gated_both_ways(ops, P, x, dense):
    """The coverage condition on the dense map's output: zero (gated) and positive entries behind a ReLU, more than one value
    without one."""
    i, role = net_maps(ops)[dense][:2]
    c = forward_ref(ops, P, x)[i]
    y = c["h"] if role == "W1" else c["y"]
    if role == "W1" or ops[i].op == R or ops[i].relu:
        return bool((y == 0).any() and (y > 0).any())
    return len(np.unique(y)) > 1


def weights(name, dense):
    """state_dict of the table (network ``name``, dense map ``dense``) as float32 arrays: the first of the draws salt = 0, 1, ...
    whose dense map meets ``gated_both_ways`` on the table's ROWS-row input (a map of one or two units can miss it)."""
    ops = model(name).ops
    for salt in range(32):
        P = _weights(name, dense, salt)
        if gated_both_ways(ops, P, inputs(name, dense, ROWS), dense):
            return P
    raise ValueError("no draw of %s / dense map %d meets the coverage condition" % (name, dense))


def _weights(name, dense, salt):
    ops = model(name).ops
    r = rng("netW", name, dense, salt)
    P = {}
    for j, (i, role, kw, kb, N, K) in enumerate(net_maps(ops)):
        ten = 10.0 if role == "W2" else 1.0
        if j == dense:
            W, b = r.choice([-1.0, 1.0], size=(N, K)), r.randint(-1, 2, N).astype(float)
        elif j < dense:
            W, b = _route_pre(N, K, r, role), np.zeros(N)
        else:
            W, b = _route_post(N, K, r, role), r.randint(-1, 2, N).astype(float)
        P[kw] = (ten * W).astype(F)
        if kb is not None:
            P[kb] = (ten * b).astype(F)
    return P


def inputs(name, dense, B):
    """x[B, nin]: integers; column j is live in row b iff j = b (mod P), P = min(16, max(1, nin // 2)) -- the rows of the dense map's
    input are sparse, every column is live in some row of a batch of ROWS.  Live values are from {1, 2} (from {-2, -1, 1, 2} where the first map is
    the dense one, positive in the first P rows)."""
    nin = model(name).in_size
    r = rng("netX", name, dense, B)
    P = min(16, max(1, nin // 2))
    live = (np.arange(nin)[None, :] % P) == (np.arange(B)[:, None] % P)
    v = r.randint(1, 3, (B, nin)).astype(float)
    if dense == 0:
        v = v * r.choice([-1.0, 1.0], size=(B, nin))
        v[: min(B, P)] = np.abs(v[: min(B, P)])            # (every column positive in some row)
    return np.where(live, v, 0.0).astype(F)


def dout_table(name, dense, B):
    """d loss / d output: 10 x an integer from {-1, 0, 1} (a multiple of 10 keeps the 0.1 of a residual block's layer2
    gradients exact); about half the entries are zero."""
    nout = model(name).out_size
    r = rng("netdY", name, dense, B)
    return (10.0 * r.randint(-1, 2, (B, nout)) * (r.randint(0, 2, (B, nout)) > 0)).astype(F)


# ----------------------------------------------------------------------------------------------- references
def _ten(a):
    q = f64(a) / 10.0
    assert np.array_equal(q, np.round(q)), "a residual layer2 tensor is not 10 x an integer"
    return q


class Bf16Hook(object):
    """The rounding hook of the references: round-to-nearest-even to bf16 (tests/bf16_emul.bf16) of a value that must be an
    fp32 number -- if it is not, the sums before it were not exact and the table is no exact table.  Counts what it did:
    ``changed`` values that were no bf16 number, ``ties`` of them exactly half way between two (where nearest-even and
    truncation, or round-half-away, part)."""

    def __init__(self):
        self.changed = self.ties = 0

    def __call__(self, a):
        from bf16_emul import bf16
        a = f64(a)
        a32 = a.astype(F)
        assert np.array_equal(a32.astype(np.float64), a), "a value a bf16 engine rounds is not an fp32 number: the sums before it were not exact"
        r = bf16(a32)
        self.changed += int(np.count_nonzero(r != a32))
        self.ties += int(np.count_nonzero((np.ascontiguousarray(a32).view(np.uint32) & 0xFFFF) == 0x8000))
        return r.astype(np.float64)


def _prod_quantum(*pairs):
    """The quantum of a sum of matrix products (and plain addends: a pair with None): every term is a multiple of it."""
    return min(quantum(a) * (quantum(b) if b is not None else 1.0) for a, b in pairs)


def _fold(a, rnd):
    """A residual block's layer2 tensor as the packer folds it: fp32(0.1f * a), an integer here (asserted)."""
    q = _ten(a)
    assert rnd is None or np.array_equal((F(0.1) * np.asarray(a, F)).astype(np.float64), q)
    return q


def forward_ref(ops, P, x, rnd=None):
    """Per op {"x", "h" (residual blocks), "y", "terms", "exact"}: float64 arrays of integers; terms = sum of |terms| per
    output of each of the op's maps (a list); exact = [(that sum, the quantum of its terms)] (``bf16_exact_sum``).
    ``rnd`` (None: nothing is rounded, the fp32 kernel) is applied where a bf16 engine rounds and nowhere else: to every packed
    weight after the fp32 folding, to every A operand -- the network input as rnd(x) + rnd(x - rnd(x)) against the first layer
    twice -- and NOT to bias, ReLU or the activations that are kept ("x", "h", "y" are the unrounded ones of the rounded forward)."""
    Rd = rnd if rnd is not None else (lambda a: a)
    x = f64(x)
    out = []
    for n, op in enumerate(ops):
        k = op.key
        if n == 0 and rnd is not None:
            assert op.op == L, "a bf16 program's first op is a linear layer"
            hi = Rd(x)
            parts = [hi, Rd(x - hi)]
        else:
            parts = [Rd(x)]
        a = sum(parts)                                       # (the operand's value: x itself where nothing is lost)
        if op.op == R:
            W1, b1, W2, b2 = Rd(f64(P[k + ".layer1.weight"])), f64(P[k + ".layer1.bias"]), Rd(_fold(P[k + ".layer2.weight"], rnd)), _fold(P[k + ".layer2.bias"], rnd)
            Ws = Rd(f64(P[k + ".skip_layer.weight"])) if op.K != op.N else np.eye(op.N)
            h = np.maximum(a @ W1.T + b1, 0.0)
            hr = Rd(h)
            y = np.maximum(hr @ W2.T + b2 + a @ Ws.T, 0.0)
            terms = [np.abs(a) @ np.abs(W1).T + np.abs(b1), np.abs(hr) @ np.abs(W2).T + np.abs(b2) + np.abs(a) @ np.abs(Ws).T]
            exact = [(terms[0], _prod_quantum((a, W1), (b1, None))), (terms[1], _prod_quantum((hr, W2), (b2, None), (a, Ws)))]
            out.append(dict(x=x, h=h, y=y, terms=terms, exact=exact))
        else:
            W, b = Rd(f64(P[k + ".weight"])), f64(P[k + ".bias"])
            y = sum(p @ W.T for p in parts) + b
            if op.relu:
                y = np.maximum(y, 0.0)
            terms = [sum(np.abs(p) for p in parts) @ np.abs(W).T + np.abs(b)]
            out.append(dict(x=x, y=y, terms=terms, exact=[(terms[0], _prod_quantum(*([(p, W) for p in parts] + [(b, None)])))]))
        x = out[-1]["y"]
    return out


def backward_ref(ops, P, fwd, dout, param_grads=True, rnd=None, exact=None, tens=True):
    """(dX, {key: gradient}, per op {"dprev", "dt"}, terms): the chain rule on the stored forward.  ``dout`` is the
    gradient w.r.t. the (un-gated) network output; with ``param_grads`` and ``tens`` it must be a multiple of 10
    (``dout_table``), as every delta behind it.  ``rnd`` as in ``forward_ref``: applied to every packed weight (the same value
    as forward) and to every delta where a matrix product of the dX chain reads it (d before d W2, dt and d before dt W1 +
    d Ws); the gates are the signs of ``fwd``'s activations (the rounded forward's, when ``fwd`` is one); the deltas that are
    kept ("dprev", "dt") and the parameter gradients A^T dY, taken on the kept values, are not rounded.  ``tens`` False (deltas
    that are no multiples of 10: a loss's, a rounded chain's): a residual block's layer2 gradients are fp32(0.1f * sum), ONE
    rounding of the exact sum -- the gradient launch scales its accumulator -- which is sum / 10 where that is an integer.
    ``exact``: a list that receives (sum of |terms|, quantum) of every sum (``bf16_exact_sum``)."""
    Rd = rnd if rnd is not None else (lambda a: a)
    tenth = lambda s: (f64(F(0.1)) * s).astype(F).astype(np.float64)          # (24 x 24 bits: the float64 product is exact)
    d = f64(dout)
    G, bufs, terms = {}, [None] * len(ops), []
    ex = exact if exact is not None else []
    for i in range(len(ops) - 1, -1, -1):
        op, c, k = ops[i], fwd[i], ops[i].key
        gate_in = i > 0                                     # the producer of this op's input went through a ReLU (checked below)
        if i > 0:
            assert ops[i - 1].op == R or ops[i - 1].relu
        dr = Rd(d)
        if op.op == R:
            W1, W2 = Rd(f64(P[k + ".layer1.weight"])), Rd(_fold(P[k + ".layer2.weight"], rnd))
            Ws = Rd(f64(P[k + ".skip_layer.weight"])) if op.K != op.N else np.eye(op.N)
            dt = (dr @ W2) * (c["h"] > 0)
            dtr = Rd(dt)
            s2, s2b = d.T @ c["h"], d.sum(0)
            q, qb = s2 / 10.0, s2b / 10.0
            if param_grads and not tens:
                q, qb = tenth(s2), tenth(s2b)
            assert not param_grads or not tens or (np.array_equal(q, np.round(q)) and np.array_equal(qb, np.round(qb)))
            G[k + ".layer2.weight"], G[k + ".layer2.bias"] = q, qb
            G[k + ".layer1.weight"], G[k + ".layer1.bias"] = dt.T @ c["x"], dt.sum(0)
            if op.K != op.N:
                G[k + ".skip_layer.weight"] = d.T @ c["x"]
            dprev = dtr @ W1 + dr @ Ws
            t5 = [np.abs(dr) @ np.abs(W2), np.abs(dtr) @ np.abs(W1) + np.abs(dr) @ np.abs(Ws),
                  np.abs(d).T @ np.abs(c["h"]), np.abs(dt).T @ np.abs(c["x"]), np.abs(d).T @ np.abs(c["x"])]
            terms += t5
            ex += [(t5[0], _prod_quantum((dr, W2))), (t5[1], _prod_quantum((dtr, W1), (dr, Ws)))]
            if param_grads:
                ex += [(t5[2], _prod_quantum((d, c["h"]))), (t5[3], _prod_quantum((dt, c["x"]))), (t5[4], _prod_quantum((d, c["x"]))),
                       (np.abs(d).sum(0), quantum(d)), (np.abs(dt).sum(0), quantum(dt))]
            bufs[i] = dict(dt=dt)
        else:
            W = Rd(f64(P[k + ".weight"]))
            G[k + ".weight"], G[k + ".bias"] = d.T @ c["x"], d.sum(0)
            dprev = dr @ W
            t2 = [np.abs(dr) @ np.abs(W), np.abs(d).T @ np.abs(c["x"])]
            terms += t2
            ex += [(t2[0], _prod_quantum((dr, W)))]
            if param_grads:
                ex += [(t2[1], _prod_quantum((d, c["x"]))), (np.abs(d).sum(0), quantum(d))]
            bufs[i] = dict()
        if gate_in:
            dprev = dprev * (c["x"] > 0)
        bufs[i]["dprev"] = dprev
        d = dprev
    return d, G, bufs, terms


def quantum(*arrays):
    """The largest power of two every element of the arrays is an integer multiple of."""
    q = np.inf
    for a in arrays:
        a = np.abs(np.asarray(a, np.float64)).ravel()
        a = a[a > 0]
        if a.size:
            m, e = np.frexp(a)
            low = np.ldexp(1.0, e - 53) * ((m * 2.0 ** 53).astype(np.int64) & -(m * 2.0 ** 53).astype(np.int64))
            q = min(q, float(low.min()))
    return 1.0 if q == np.inf else q


def exact_sum(terms, axis=-1):
    """The exact-table condition for sums whose terms are multiples of one quantum: sum |terms| < 2^24 quantum."""
    t = np.abs(np.asarray(terms, np.float64))
    return float(t.sum(axis=axis).max()) < 2.0 ** 24 * quantum(t)


def bf16_exact_sum(pairs):
    """``exact_sum``'s condition on the ROUNDED operands of every matrix product of a reference run with a rounding hook:
    ``pairs`` are the (sum of |terms| per output, quantum of the terms) the references record -- the quantum taken
    conservatively, as the product of the smallest quanta over the two whole operand arrays (and the bias).  Every partial sum,
    in any order and any K split, is then a multiple of the quantum below 2^24 of them: an fp32 number."""
    return all(float(np.max(s)) < 2.0 ** 24 * q for s, q in pairs if np.size(s))


def bf16_margin(pairs):
    """log2 of the worst sum |terms| / quantum over ``pairs`` (24 is the limit)."""
    return max([np.log2(max(float(np.max(s)), 1e-300) / q) for s, q in pairs if np.size(s)] or [0.0])


# ----------------------------------------------------------------------------------------------- serving
def serving_consts(name, kind="diag"):
    """Priors (all Gaussian), transforms, data and the inverse covariance of the serving problem on network ``name``, chosen so
    that x = z 2^e + s (e from {0, 1}, s from {-2, 0, 2}) and d = h cscale + cshift (cscale a power of two, cshift an integer):
      a2 = X_std 2^e, a1 = X_mean + X_std s;  cscale = y_std sigma, cshift = y_mean sigma - data.
    kind "diag": the weights of the columns are from {0.5, 1, 2}; "dense": S = L L^T with L lower triangular (``dense_factor``)."""
    m = model(name)
    nin, nout = m.in_size, m.out_size
    j, o = np.arange(nin), np.arange(nout)
    e, s = j % 2, 2 * ((j % 3) - 1)
    X_std = 2.0 ** ((j % 3) - 1)
    X_mean = ((j % 5) - 2).astype(float)
    a2, a1 = X_std * 2.0 ** e, X_mean + X_std * s
    y_std, sigma = 2.0 ** (o % 2), 2.0 ** (-((o // 2) % 2))           # cscale from {0.5, 1, 2}
    y_mean = ((o % 3) - 1).astype(float) * 2.0
    data = y_mean * sigma - np.array([1.0, -1.0, 2.0, -2.0])[o % 4]           # cshift from {-2, -1, 1, 2}: d is rarely zero
    c = dict(nin=nin, nout=nout, e=e, s=s, X_std=X_std, X_mean=X_mean, a1=a1, a2=a2, y_std=y_std, y_mean=y_mean, sigma=sigma,
             data=data, cscale=y_std * sigma, cshift=y_mean * sigma - data, T=T_EXACT,
             priors=[{"param": "p%d" % i, "dist": "gauss", "arg1": float(a1[i]), "arg2": float(a2[i])} for i in range(nin)])
    if kind == "diag":
        c["w"] = 2.0 ** ((o % 3) - 1)
        c["invcov"] = np.diag(c["w"])
    else:
        c["L"] = dense_factor(nout)
        c["invcov"] = c["L"] @ c["L"].T
    return c


def dense_factor(nout):
    """L: lower triangular, diagonal from {1, 2}, and in column n the entries L[n + 1][n], L[n + 17][n], L[n + 64][n] and
    L[n + 513][n] from {-1, +1} (where those rows exist) -- a non-zero at the first row of every 16-row step behind the diagonal
    block, one past the 64-column block and one in the second 512-row pass."""
    r = rng("denseL", nout)
    Lm = np.diag(2.0 ** r.randint(0, 2, nout))
    n = np.arange(nout)
    for dlt in (1, 16, 17, 64, 513):
        m = n[n + dlt < nout]
        Lm[m + dlt, m] = r.choice([-1.0, 1.0], size=len(m))
    return Lm


def z_of(c, x):
    """The latent rows that the prior map and the input transform turn into the integer rows ``x``."""
    return ((f64(x) - c["s"][None, :]) / 2.0 ** c["e"][None, :]).astype(F)


def serving_ref(ops, P, c, z, grad=False, rnd=None):
    """theta, lnP (and d lnP / d z) in float64 from the definitions; also the likelihood's terms per row.  ``rnd``: the
    network's two halves round as ``forward_ref`` / ``backward_ref`` say; the prior map, the input transform, the output map,
    the likelihood, the turnaround -(d w) gscale / T, the prior map's derivative and -z do not ("exact": every recorded sum)."""
    z = f64(z)
    theta = z * c["a2"][None, :] + c["a1"][None, :]
    x = (theta - c["X_mean"][None, :]) / c["X_std"][None, :]
    fwd = forward_ref(ops, P, x, rnd)
    d = fwd[-1]["y"] * c["cscale"][None, :] + c["cshift"][None, :]
    T = float(c["T"])
    if "w" in c:
        like_terms = d * d * c["w"][None, :] / (2.0 * T)
        dd = -(d * c["w"][None, :]) / T
        mid_terms = []
    else:
        U = d @ c["L"]
        like_terms = U * U / (2.0 * T)
        dd = -(U @ c["L"].T) / T
        mid_terms = [np.abs(d) @ np.abs(c["L"])]
    lnP = -like_terms.sum(-1) - 0.5 * (z * z).sum(-1)
    out = dict(theta=theta, x=x, fwd=fwd, d=d, lnP=lnP, terms=np.concatenate([like_terms, 0.5 * z * z], axis=1), mid_terms=mid_terms,
               exact=[e for f in fwd for e in f["exact"]])
    if grad:
        dh = dd * c["cscale"][None, :]
        dx, _, _, bterms = backward_ref(ops, P, fwd, dh, param_grads=False, rnd=rnd, exact=out["exact"])
        out["G"] = dx / c["X_std"][None, :] * c["a2"][None, :] - z
        out["bterms"] = bterms + ([np.abs(U) @ np.abs(c["L"]).T] if "L" in c else [])
    return out


def lnp_bound(ref):
    """The derived bound where lnP cannot be exact (entries_ref.loglike_diag_bound's form): terms x 2^-24 x sum |terms|."""
    t = np.abs(ref["terms"])
    return (t.shape[1] + 4) * 2.0 ** -24 * t.sum(-1)


def leapfrog_ref(G, Q, Pm, mass, ek, ed):
    """P += eps_kick G; Q += eps_drift P / mass."""
    Pn = f64(Pm) + ek * f64(G)
    return Pn, f64(Q) + ed * Pn / f64(mass)[None, :]


# ----------------------------------------------------------------------------------------------- what the tests run
GRAD_NETS = tuple(n for n, s in NETS.items() if not n.startswith("dense") and max(model(n).in_size, model(n).out_size) <= 64)
# The bf16 one-launch gradient (linna_logprob_set_grad_precision): the networks with such a program on every engine, and the
# ones the setter refuses (more than 64 inputs or outputs).  Literal: tests/test_net_exact_host.py holds them against the planner.
BF16_GRAD_NETS = ("in1_n1", "in15_n16", "in16_n17", "in17_n32", "in64_n64", "n512_513", "n1000_1024", "split_4k", "wide_3k", "side16_1",
                  "side16_2", "side32_1", "side32_2", "side32_3", "side64_1", "side64_2", "side64_3", "grad257", "grad513", "v2_33_33", "v2_5_1",
                  "v2_6_30", "v2_6_31", "simple_6_4", "simple_6_31", "blk_c1", "blk_c16", "blk_c17", "blk_c64", "blk_id17", "blk_id64", "k31_63",
                  "bf_split_wide", "bf_n64_k256_257", "bf_n64_k512_513", "bf_n32_k512_513", "bf_n16_k1024", "blk_k20_c31", "blk_k20_c32",
                  "blk_k20_c33", "blk_k40_c15")
BF16_GRAD_REFUSED = ("in65_n128", "in256_n256", "v2_26_457")
# The merged training step is driven on a subset that covers each family: the K-tail MLPs, one network per column class of the
# narrow layers behind a long K (16 / 32 / 64 columns), the SPLIT / WIDE pair, residual blocks of each kind.  Every network
# of NETS has a bf16 training step on the 4-row engine, the only one that runs it (pinned by the host test).
TRAIN_STEP_NETS = ("in1_n1", "in15_n16", "in16_n17", "in17_n32", "k31_63", "side16_2", "side32_2", "side64_2", "bf_split_wide", "bf_n64_k256_257",
                   "blk_c17", "blk_id17", "blk_c64", "v2_6_31", "simple_6_4", "v2_33_33", "blk_k20_c31", "blk_k20_c32", "blk_k20_c33", "blk_k40_c15")
_tables = {}


def n_maps(name):
    return len(net_maps(model(name).ops))


def table(name, dense, B=ROWS):
    """The training table: weights, x, the stored forward, dout and the backward (computed once, shared, never written)."""
    key = (name, dense, B)
    if key not in _tables:
        ops = model(name).ops
        P, x, dY = weights(name, dense), inputs(name, dense, B), dout_table(name, dense, B)
        fwd = forward_ref(ops, P, x)
        dX, G, bufs, bterms = backward_ref(ops, P, fwd, dY)
        _tables[key] = dict(ops=ops, P=P, x=x, dY=dY, fwd=fwd, dX=dX, G=G, bufs=bufs, bterms=bterms)
    return _tables[key]


def serving_table(name, dense, B=ROWS, kind="diag", grad=False):
    key = (name, dense, B, kind, grad)
    if key not in _tables:
        c = serving_consts(name, kind)
        P, z = weights(name, dense), z_of(c, inputs(name, dense, B))
        _tables[key] = dict(c=c, P=P, z=z, ref=serving_ref(model(name).ops, P, c, z, grad=grad))
    return _tables[key]


def bf16_table(name, dense, B=ROWS):
    """``table`` through the rounding references (the dX chain of a bf16 training step on the table's dout): the same fields,
    "hook" (what was rounded) and "exact" (``bf16_exact_sum``'s pairs)."""
    key = ("bf16", name, dense, B)
    if key not in _tables:
        ops = model(name).ops
        P, x, dY = weights(name, dense), inputs(name, dense, B), dout_table(name, dense, B)
        hook = Bf16Hook()
        fwd = forward_ref(ops, P, x, hook)
        exact = [e for f in fwd for e in f["exact"]]
        dX, G, bufs, bterms = backward_ref(ops, P, fwd, dY, rnd=hook, exact=exact, tens=False)
        _tables[key] = dict(ops=ops, P=P, x=x, dY=dY, fwd=fwd, dX=dX, G=G, bufs=bufs, bterms=bterms, hook=hook, exact=exact)
    return _tables[key]


def bf16_serving_table(name, dense, B=ROWS, grad=False):
    """``serving_table`` (diagonal likelihood) through the rounding references, with "hook"."""
    key = ("bf16", name, dense, B, "diag", grad)
    if key not in _tables:
        c = serving_consts(name)
        P, z = weights(name, dense), z_of(c, inputs(name, dense, B))
        hook = Bf16Hook()
        _tables[key] = dict(c=c, P=P, z=z, ref=serving_ref(model(name).ops, P, c, z, grad=grad, rnd=hook), hook=hook)
    return _tables[key]


# ---- the merged training step's loss (api.hip linna_net_train_step; util.py:1072-1088): exact tables
#   ynorm integers with some entries NaN (masked), den a power of two per row, inv_batch a power of two, Cinv with the sparse
#   integer structure of dense_factor (diagonal from {1, 2}, a few off-diagonal entries +-1), symmetric:
#   delta = ynorm - pred (0 where masked), U = delta Cinv, loss_b = delta . U / den, mean = inv_batch sum_b loss_b,
#   dpred = -2 U inv_batch / den (0 where masked) are exact in fp32.
LOSS_ROWS = (1, 3, 4, 5, 9, 20)
INV_BATCH = 2.0 ** -3


def loss_cinv(nout):
    """Symmetric, integer: diag from {1, 2}; +-1 at (n, n + dlt) and (n + dlt, n) for dlt of 1, 17, 64 in one column of three."""
    r = rng("lossC", nout)
    Cm = np.diag(2.0 ** r.randint(0, 2, nout))
    n = np.arange(nout)
    for dlt in (1, 17, 64):
        m = n[(n + dlt < nout) & (n % 3 == dlt % 3)]
        v = r.choice([-1.0, 1.0], size=len(m))
        Cm[m + dlt, m] = v
        Cm[m, m + dlt] = v
    return Cm


def loss_consts(name, dense, B):
    """(YN [B, nout], den [B] from {1, 2, 4}, Cinv).  YN: integers from {-3 .. 3} with about one entry in eight NaN, and in
    every fourth row (0, 4, ...) ONE entry of nine significant bits, an odd integer of magnitude 257 ... 511: the deltas there
    (delta, U, d loss / d pred and what the dX chain makes of them) are no bf16 numbers -- half of them ties -- so the bf16
    training step has something to round on every network; one row in four keeps the batch mean's sum (delta^2 terms of 2^18)
    within the exactness condition at 20 rows."""
    nout = model(name).out_size
    r = rng("lossY", name, dense, B)
    YN = r.randint(-3, 4, (B, nout)).astype(np.float64)
    YN[r.randint(0, 8, (B, nout)) == 0] = np.nan
    den = 2.0 ** r.randint(0, 3, B)
    rows = np.arange(0, B, 4)
    YN[rows, r.randint(0, nout, len(rows))] = r.choice([-1.0, 1.0], size=len(rows)) * (257.0 + 2.0 * r.randint(0, 128, len(rows)))
    return YN.astype(F), den.astype(F), loss_cinv(nout)


def loss_ref(pred, YN, den, Cinv, inv_batch=INV_BATCH):
    """(loss rows, batch mean, dpred, [(sum |terms|, quantum)]) in float64 from the definitions; nothing here is rounded,
    on a bf16 handle neither (the loss segment is an fp32 run on the unrounded prediction)."""
    YN, den, pred = f64(YN), f64(den), f64(pred)
    mask = np.isnan(YN)
    delta = np.where(mask, 0.0, YN - pred)
    U = delta @ f64(Cinv).T
    rows = (delta * U).sum(1) / den
    dpred = np.where(mask, 0.0, -2.0 * U * inv_batch / den[:, None])
    pairs = [(np.abs(delta) @ np.abs(f64(Cinv)).T, _prod_quantum((delta, Cinv))), (np.abs(delta * U).sum(1), _prod_quantum((delta, U))),
             (np.abs(rows).sum(keepdims=True) * inv_batch, quantum(rows) * inv_batch)]
    return rows, rows.sum() * inv_batch, dpred, pairs


def loss_table(name, dense, B, bf=False):
    """One merged training step on the table's weights and input: forward, loss, the dX chain from dpred, every parameter
    gradient.  ``bf``: through the rounding references (the loss itself never rounds)."""
    key = ("loss", name, dense, B, bf)
    if key not in _tables:
        ops = model(name).ops
        P, x = weights(name, dense), inputs(name, dense, B)
        YN, den, Cinv = loss_consts(name, dense, B)
        hook = Bf16Hook() if bf else None
        fwd = forward_ref(ops, P, x, hook)
        rows, mean, dpred, exact = loss_ref(fwd[-1]["y"], YN, den, Cinv)
        exact = [e for f in fwd for e in f["exact"]] + exact
        dX, G, bufs, _ = backward_ref(ops, P, fwd, dpred, rnd=hook, exact=exact, tens=False)
        _tables[key] = dict(ops=ops, P=P, x=x, YN=YN, den=den, Cinv=Cinv, fwd=fwd, rows=rows, mean=mean, dpred=dpred, G=G, bufs=bufs,
                            hook=hook, exact=exact)
    return _tables[key]


def sweep_tables(name):
    """(dense map, rows) of every table the GPU tests run on network ``name``: every dense map at ROWS rows, and the first and
    the last map at every batch size of BATCH_ROWS."""
    n = n_maps(name)
    return [(m, ROWS) for m in range(n)] + [(m, B) for m in sorted({0, n - 1}) for B in BATCH_ROWS]


def fwd_layout(ops, B):
    """[(op index, "h" | "y", offset, ld, columns)] of the forward workspace (api.hip fwd_floats) and its size in floats."""
    out, off = [], 0
    for i, op in enumerate(ops):
        if op.op == R:
            out.append((i, "h", off, _lib.ld4(op.C), op.C))
            off += B * _lib.ld4(op.C)
        if i + 1 < len(ops):
            out.append((i, "y", off, _lib.ld4(op.N), op.N))
            off += B * _lib.ld4(op.N)
    return out, off


def bwd_layout(ops, B):
    """[(op index, "dprev" | "dt", offset, ld, columns)] of the backward workspace (api.hip net_bufs: walked from the last op
    down; d/d(input) of every op but the first, d/dh behind it for a residual block) and its size in floats."""
    out, off = [], 0
    for i in range(len(ops) - 1, -1, -1):
        op = ops[i]
        if i > 0:
            out.append((i, "dprev", off, _lib.ld4(op.K), op.K))
            off += B * _lib.ld4(op.K)
        if op.op == R:
            out.append((i, "dt", off, _lib.ld4(op.C), op.C))
            off += B * _lib.ld4(op.C)
    return out, off


# ---- the leapfrog: eps a power of two, masses from {1, 2}, momenta halves
EPS = 0.125


def MASS(nin):
    return 2.0 ** (np.arange(nin) % 2)


def momenta(name, dense, B):
    nin = model(name).in_size
    return (0.5 * rng("netP", name, dense, B).randint(-4, 5, (B, nin))).astype(F)


# ---- dense likelihoods: the network's last layer is the dense map (d is non-zero almost everywhere); the direct form
#      (chi^2 = d S d^T, LINNA_DENSE_FACTORED=0) where the whole sum over i, j stays exact
DIRECT_NETS = ("dense16", "dense33", "dense64")


def dense_sweep(name):
    n = n_maps(name)
    return [(n - 1, ROWS), (0, ROWS)] + [(n - 1, B) for B in (1, 17)]


# serving tables whose lnP cannot meet the exactness condition and is compared within lnp_bound instead: none
LNP_FALLBACK = ()
# networks whose 16-row serving program is plain (WIDE and SPLIT segments only): pinned by tests/test_net_exact_host.py
PLAIN_NETS = ("grad257", "grad513", "in15_n16", "in1_n1", "n1000_1024", "n512_513")
