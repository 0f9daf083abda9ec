"""CPU: the exact tables of tests/net_exact.py meet the conditions tests/test_gpu_net_exact.py relies on, the integer
references agree with the project's float64 oracle, and every shape still lands on the planner edge it is named for.

Conditions (asserted for EVERY table a GPU test runs -- net_exact.sweep_tables, the serving and the dense tables):
 * exactness: for every map, row and output the sum of |terms| is below 2^24 quanta (entries_ref.exact_ok's rule) -- forward,
   the dX chain, dW over the batch, the likelihood and the leapfrog;
 * coverage: every weight position of the dense map is non-zero, every one of its input columns is non-zero in some row, its
   output has zero (gated) and positive entries (more than one value where it has no ReLU);
 * folding: float32(0.1) * w and float32(0.1) * b are integers for every residual layer2 weight and bias (numpy float32).
No table needed the derived-bound fallback for lnP: ``test_lnp_is_exact_everywhere`` asserts that."""
import numpy as np
import pytest

import entries_ref as er
import net_exact as ne
from linna_amd import _lib, nn
from oracle import emulator, likelihood

F = np.float32


def small(*sums):
    """exact_ok on sums of |terms| that are already taken."""
    return er.exact_ok(*[np.asarray(s)[..., None] for s in sums])


def dense_io(name, dense, t):
    i, role = ne.net_maps(t["ops"])[dense][:2]
    c = t["fwd"][i]
    return (c["h"] if role == "W2" else c["x"]), (c["h"] if role == "W1" else c["y"]), bool(role == "W1" or t["ops"][i].op == ne.R or t["ops"][i].relu)


@pytest.mark.parametrize("name", list(ne.NETS))
def test_training_tables_meet_the_conditions(name):
    maps = ne.net_maps(ne.model(name).ops)
    for dense, B in ne.sweep_tables(name):
        t = ne.table(name, dense, B)
        tag = "%s dense map %d rows %d" % (name, dense, B)
        # exactness: forward, dX chain, dW
        assert small(*[s for c in t["fwd"] for s in c["terms"]]), tag
        assert small(*t["bterms"]), tag
        # the values themselves are integers (dout, and with it every gradient, a multiple of 10)
        for c in t["fwd"]:
            assert np.array_equal(c["y"], np.round(c["y"])), tag
        assert np.array_equal(t["dY"] / 10, np.round(t["dY"] / 10)) and np.array_equal(t["dX"] / 10, np.round(t["dX"] / 10)), tag
        for k, g in t["G"].items():
            assert np.array_equal(g, np.round(g)), (tag, k)
        # coverage
        W = t["P"][maps[dense][2]]
        assert np.all(W != 0), tag
        if B == ne.ROWS:
            xin, yout, relu = dense_io(name, dense, t)
            assert (np.abs(xin) > 0).any(axis=0).all(), tag
            if relu:
                assert (yout == 0).any() and (yout > 0).any(), tag
            else:
                assert len(np.unique(yout)) > 1, tag
            assert ne.gated_both_ways(t["ops"], t["P"], t["x"], dense), tag
        # folding, in numpy float32
        for (i, role, kw, kb, N, K) in maps:
            if role == "W2":
                for a in (t["P"][kw], t["P"][kb]):
                    folded = F(0.1) * a.astype(F)
                    assert folded.dtype == F and np.array_equal(folded, np.round(folded)) and np.array_equal(folded, ne._ten(a).astype(F)), tag


@pytest.mark.parametrize("name", [n for n in ne.NETS if n not in ne.DENSE_NETS])
def test_serving_tables_meet_the_conditions(name):
    grad = name in ne.GRAD_NETS
    for dense, B in ne.sweep_tables(name):
        s = ne.serving_table(name, dense, B, grad=grad)
        c, ref, tag = s["c"], s["ref"], "%s dense map %d rows %d" % (name, dense, B)
        assert np.array_equal(ref["x"], ne.inputs(name, dense, B).astype(np.float64)), tag        # the prior map + input transform give the table's x
        assert np.array_equal(ref["theta"].astype(F).astype(np.float64), ref["theta"]), tag
        assert ne.exact_sum(ref["terms"]), tag                                                     # lnP: no fallback
        assert np.array_equal(ref["lnP"].astype(F).astype(np.float64), ref["lnP"]), tag
        for v in (c["cscale"], c["X_std"], c["a2"], c["w"]):
            m, _ = np.frexp(v)
            assert np.all(m == 0.5), tag                                                           # powers of two
        for v in (c["cshift"], c["a1"], c["X_mean"], c["data"]):
            assert np.array_equal(v, np.round(v)), tag
        if grad:
            assert small(*ref["bterms"]), tag
            assert np.array_equal(ref["G"].astype(F).astype(np.float64), ref["G"]), tag
            # leapfrog with eps = 2^-3, mass from {1, 2}: P and Q keep few bits
            Pn, Qn = ne.leapfrog_ref(ref["G"], s["z"], ne.momenta(name, dense, B), ne.MASS(c["nin"]), ne.EPS, ne.EPS)
            assert np.array_equal(Pn.astype(F).astype(np.float64), Pn) and np.array_equal(Qn.astype(F).astype(np.float64), Qn), tag


@pytest.mark.parametrize("name", ne.DENSE_NETS)
def test_dense_tables_meet_the_conditions(name):
    c = ne.serving_consts(name, "dense")
    Lm, S = c["L"], c["invcov"]
    assert np.array_equal(np.tril(Lm), Lm) and np.all(np.diag(Lm) > 0)
    assert np.array_equal(S.astype(F).astype(np.float64), S) and np.count_nonzero(S - np.diag(np.diagonal(S))) > 0
    # what util.Log_prob._build does with the float32 matrix: the float64 Cholesky factor IS L
    S32 = S.astype(F).astype(np.float64)
    assert np.array_equal(np.linalg.cholesky(0.5 * (S32 + S32.T)), Lm)
    nout = c["nout"]
    for dlt in (1, 16, 17, 64, 513):                        # the bands are there
        if dlt < nout:
            assert np.all(np.diagonal(Lm, -dlt) != 0)
    for dense, B in ne.dense_sweep(name):
        s = ne.serving_table(name, dense, B, kind="dense")
        ref, tag = s["ref"], "%s dense map %d rows %d" % (name, dense, B)
        assert small(*ref["mid_terms"]), tag                                         # U = d L
        assert (np.abs(ref["d"]) > 0).any(axis=0).all() or B < ne.ROWS, tag          # every row of L meets a non-zero d
        assert ne.exact_sum(ref["terms"]), tag                                       # |U|^2 / 2T + |z|^2 / 2: no fallback
        # the direct form d S d^T (nout <= 64 here): its terms d_i S_ij d_j
        if name in ne.DIRECT_NETS:
            d = ref["d"]
            t = np.abs(d)[:, :, None] * np.abs(S)[None] * np.abs(d)[:, None, :]
            assert ne.exact_sum(np.concatenate([t.reshape(len(d), -1) / (2 * c["T"]), 0.5 * s["z"].astype(np.float64) ** 2], axis=1)), tag
            assert np.allclose(-(d @ S * d).sum(-1) / (2 * c["T"]) - 0.5 * (s["z"].astype(np.float64) ** 2).sum(-1), ref["lnP"], rtol=0, atol=0), tag


def test_lnp_is_exact_everywhere():
    """The derived-bound fallback (net_exact.lnp_bound) exists and is unused: every serving table's lnP meets the exactness
    condition, so the GPU tests compare lnP bit for bit on every table."""
    assert ne.LNP_FALLBACK == ()


# ----------------------------------------------------------------------------------------------- the oracle
def _kind(name):
    return {"v2": "ChtoModelv2", "simple": "ChtoModelsimple"}[ne.NETS[name][0]]


@pytest.mark.parametrize("name", [n for n, s in ne.NETS.items() if s[0] in ("v2", "simple")])
def test_references_agree_with_the_oracle(name):
    """oracle.emulator / oracle.likelihood in float64 on the same tables (the real network classes): 1e-9 relative."""
    m = ne.model(name)
    n = ne.n_maps(name)
    for dense in sorted({0, 1, 2, 3, n // 2, n - 1}):
        t = ne.table(name, dense)
        P64 = {k: v.astype(np.float64) for k, v in t["P"].items()}
        out, caches = emulator.forward(P64, t["x"].astype(np.float64), _kind(name), m.in_size, m.out_size, keep=True)
        close = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9 * max(1.0, float(np.abs(b).max())))
        close(out, t["fwd"][-1]["y"])
        for c, r in zip(caches, t["fwd"]):
            close(c[-1], r["y"])
            if len(c) == 3:
                close(c[1], r["h"])
        dx, grads = emulator.backward(P64, caches, t["dY"].astype(np.float64), _kind(name), m.in_size, m.out_size)
        close(dx, t["dX"])
        assert set(grads) == set(t["G"])
        for k in grads:
            close(grads[k], t["G"][k])
        if name in ne.GRAD_NETS:
            s = ne.serving_table(name, dense, grad=True)
            c = s["c"]
            emu = likelihood.Emulator(_kind(name), m.in_size, m.out_size, P64, c["X_mean"], c["X_std"], c["y_mean"], c["y_std"], c["sigma"])
            lnp, g = likelihood.grad_log_prob(s["z"], emu, c["priors"], c["data"], c["invcov"], c["T"], dtype=np.float64)
            close(lnp, s["ref"]["lnP"])
            close(g, s["ref"]["G"])
            close(likelihood.prior_map(s["z"].astype(np.float64), c["priors"]), s["ref"]["theta"])


def test_custom_networks_agree_with_the_oracle_layer_by_layer():
    """The custom op lists have no oracle topology; an MLP of equal widths has (kind "MLP"): the same reference code."""
    spec = ne.mlp(7, [24, 24], 5)
    net = ne.ExactNet(spec)
    r = er.rng("oracle-mlp")
    P = {}
    for (i, role, kw, kb, N, K) in ne.net_maps(net.ops):
        P[kw], P[kb] = r.randint(-2, 3, (N, K)).astype(F), r.randint(-2, 3, N).astype(F)
    x = r.randint(-2, 3, (9, 7)).astype(F)
    fwd = ne.forward_ref(net.ops, P, x)
    P64 = {"layer%d.%s" % (i + 1, k.split(".")[1]): v.astype(np.float64) for i in range(3) for k, v in P.items() if k.startswith("op%d." % i)}
    out, caches = emulator.forward(P64, x.astype(np.float64), "MLP", 7, 5, keep=True, width=24, depth=2)
    np.testing.assert_allclose(out, fwd[-1]["y"], rtol=1e-9)
    dY = 10.0 * r.randint(-1, 2, (9, 5))
    dx, grads = emulator.backward(P64, caches, dY, "MLP", 7, 5, width=24, depth=2)
    dX, G, _, _ = ne.backward_ref(net.ops, P, fwd, dY)
    np.testing.assert_allclose(dx, dX, rtol=1e-9)
    for i in range(3):
        np.testing.assert_allclose(grads["layer%d.weight" % (i + 1)], G["op%d.weight" % i], rtol=1e-9)
        np.testing.assert_allclose(grads["layer%d.bias" % (i + 1)], G["op%d.bias" % i], rtol=1e-9)


# ----------------------------------------------------------------------------------------------- the planner
def segs(name, rows=16, dense_nout=0):
    n, txt = nn.describe_program(ne.model(name), rows, dense_nout)
    lines = txt.strip().splitlines()
    assert lines[0].startswith("ok"), (name, txt)
    return lines[0], lines[1:]


# (network, engine rows, segment index, what its line starts with): the edge each shape is named for
PLAN = [
    ("in1_n1", 16, 0, "WIDE steps 1 passes 1 ncg 1 kc 1 dst 0 zext 0 N 1"),
    ("in64_n64", 16, 0, "SPLIT steps 1 passes 1 ncg 1 "),              # 64 columns: one column group
    ("in64_n64", 16, 1, "SPLIT steps 1 passes 1 ncg 2 "),              # 65: two
    ("in65_n128", 16, 0, "SPLIT steps 2 passes 1 ncg 2 "),             # 128: two
    ("in65_n128", 16, 1, "SPLIT steps 4 passes 1 ncg 4 "),             # 129: four
    ("in256_n256", 16, 0, "SPLIT steps 8 passes 1 ncg 4 "),            # 256 is SPLIT with 4 column groups
    ("in256_n256", 16, 1, "WIDE steps 16 passes 1 "),                  # 257 is WIDE
    ("n512_513", 16, 0, "WIDE steps 1 passes 1 "),                     # 512: one pass
    ("n512_513", 16, 1, "WIDE steps 32 passes 2 "),                    # 513: two
    ("n1000_1024", 16, 0, "WIDE steps 1 passes 2 "),
    ("n1000_1024", 16, 1, "WIDE steps 63 passes 2 "),                  # K = 1000: 63 steps, the last one 8 k
    ("split_4k", 16, 1, "SPLIT steps 1 passes 1 ncg 2 "),              # split_steps + 3 <= ksteps: 1 + 3 <= 4
    ("wide_3k", 16, 1, "WIDE steps 3 passes 1 "),                      # 1 + 3 > 3
    ("side16_1", 16, 1, "SIDE steps 1 passes 1 ncg 1 kc 4 "),          # 16 outputs behind 500: one SIDE step, kc 4
    ("side16_2", 16, 1, "SIDE steps 2 passes 1 ncg 1 kc 4 "),          # 16 outputs behind 1000 is SIDE on the 16-row engine: two steps
    ("side16_2", 4, 1, "SPLIT steps 8 passes 1 ncg 1 "),               # ... and SPLIT on the others
    ("side32_1", 16, 1, "SIDE steps 1 passes 1 ncg 1 kc 2 "),
    ("side32_2", 16, 1, "SIDE steps 2 passes 1 ncg 1 kc 2 "),
    ("side32_3", 16, 1, "SPLIT steps 5 passes 1 ncg 1 "),              # one step past the limit
    ("side64_1", 16, 1, "SIDE steps 1 passes 1 ncg 1 kc 1 "),
    ("side64_2", 16, 1, "SIDE steps 2 passes 1 ncg 1 kc 1 "),
    ("side64_3", 16, 1, "SPLIT steps 3 passes 1 ncg 1 "),
    ("v2_33_33", 16, 9, "SIDE steps 1 passes 1 ncg 1 kc 1 dst 0 zext 64 N 33"),     # the last forward segment as a SIDE one
    ("v2_33_33", 4, 9, "WIDE steps 3 passes 1 "),
    ("v2_33_33", 16, 1, "SIDE steps 2 passes 1 ncg 1 kc 4 dst 1008 "),               # h of the first block behind its 1000-column input
    ("blk_c1", 16, 1, "SIDE steps 1 passes 1 ncg 1 kc 4 dst 32 zext 64 N 1"),
    ("blk_c17", 16, 1, "SIDE steps 1 passes 1 ncg 1 kc 2 dst 48 zext 64 N 17"),
    ("blk_c64", 16, 1, "SIDE steps 1 passes 1 ncg 1 kc 1 dst 112 zext 64 N 64"),
    ("blk_id17", 16, 2, "WIDE steps 3 passes 1 ncg 1 kc 1 dst 0 zext 0 N 17"),        # [I | 0.1 W2] over [x (32) ; h (16)]: 3 steps
    ("blk_id64", 16, 2, "SPLIT steps 1 passes 1 ncg 1 kc 1 dst 0 zext 512 N 64"),
]


@pytest.mark.parametrize("name,rows,i,want", PLAN)
def test_shapes_sit_on_their_planner_edges(name, rows, i, want):
    head, lines = segs(name, rows)
    assert lines[i].startswith(want), "%s on the %d-row engine, segment %d: %s" % (name, rows, i, lines[i])


def test_gradient_programs():
    """The fused MLP gradient where every hidden layer is wider than 256 (one mask slot per pass: 257 one, 513 two); the
    any-network form (NS_BWD_INPUT) for the others; both in one launch for every network of GRAD_NETS."""
    for name, slots in (("grad257", 2), ("grad513", 4)):
        head, lines = segs(name)
        assert head.endswith("grad 1") and len(lines) == 6, head
        assert sum(int(ln.split()[4]) for ln in lines[:2]) == slots
    for name in ne.GRAD_NETS:
        head, lines = segs(name)
        _, g = segs(name, 16, -1)
        assert head.endswith("grad 1") or g[-1].endswith("one launch"), (name, head, g[-1])
    for name in ("v2_33_33", "blk_id64", "in64_n64", "simple_6_4"):
        assert segs(name)[0].endswith("grad 0") and segs(name, 16, -1)[1][-1].endswith("one launch")


def test_dense_programs():
    """U = d L behind d in the same buffer up to 256 columns, in the other buffer from 257; the factored form's second pass
    from 513; the balanced triangular pass for 16 column blocks (960 < nout <= 1024) under linna_dense_tri 2."""
    lib = _lib.load()
    prev = lib.linna_dense_tri(-1)
    want = {  # name: (tri 0, tri 1, tri 2) of the factored program's last segment
        "dense16": ("SPLIT steps 1 passes 1 ncg 1 kc 1 dst 16 ",) * 3, "dense64": ("SPLIT steps 1 passes 1 ncg 1 kc 1 dst 64 ",) * 3,
        "dense65": ("SPLIT steps 2 passes 1 ncg 2 kc 1 dst 80 ",) * 3, "dense256": ("SPLIT steps 8 passes 1 ncg 4 kc 1 dst 256 ",) * 3,
        "dense257": ("WIDE steps 17 passes 1 ncg 1 kc 1 dst 0 zext 0 ",) * 3, "dense512": ("WIDE steps 32 passes 1 ncg 1 kc 1 dst 0 zext 0 ",) * 3,
        "dense513": ("WIDE steps 33 passes 2 ncg 1 kc 1 dst 0 zext 0 ", "WIDE steps 33 passes 2 ncg 1 kc 1 dst 0 zext 1 ", "WIDE steps 33 passes 2 ncg 1 kc 1 dst 0 zext 1 "),
        "dense960": ("WIDE steps 60 passes 2 ncg 1 kc 1 dst 0 zext 0 ", "WIDE steps 60 passes 2 ncg 1 kc 1 dst 0 zext 28 ", "WIDE steps 60 passes 2 ncg 1 kc 1 dst 0 zext 28 "),
        "dense961": ("WIDE steps 61 passes 2 ncg 1 kc 1 dst 0 zext 0 ", "WIDE steps 61 passes 2 ncg 1 kc 1 dst 0 zext 29 ", "WIDE steps 61 passes 2 ncg 1 kc 1 dst 0 zext -1 "),
        "dense1000": ("WIDE steps 63 passes 2 ncg 1 kc 1 dst 0 zext 0 ", "WIDE steps 63 passes 2 ncg 1 kc 1 dst 0 zext 31 ", "WIDE steps 63 passes 2 ncg 1 kc 1 dst 0 zext -1 "),
        "dense1024": ("WIDE steps 64 passes 2 ncg 1 kc 1 dst 0 zext 0 ", "WIDE steps 64 passes 2 ncg 1 kc 1 dst 0 zext 32 ", "WIDE steps 64 passes 2 ncg 1 kc 1 dst 0 zext -1 "),
    }
    try:
        for name, w in want.items():
            nout = ne.model(name).out_size
            for tri in (0, 1, 2):
                lib.linna_dense_tri(tri)
                for rows in (16, 4):
                    last = segs(name, rows, -nout)[1][-1]
                    assert last.startswith(w[tri]) and last.endswith("N %d" % nout), (name, tri, rows, last)
    finally:
        lib.linna_dense_tri(prev)
    # the direct form (S itself): a SIDE segment on the 16-row engine behind a last layer that is not one
    assert segs("dense33", 16, 33)[1][-1].startswith("SIDE steps 1 passes 1 ncg 1 kc 1 dst 48 ")
    assert segs("dense33", 4, 33)[1][-1].startswith("SPLIT steps 1 passes 1 ncg 1 kc 1 dst 48 ")
    assert segs("dense16", 16, 16)[1][-1].startswith("SPLIT steps 1 passes 1 ncg 1 kc 1 dst 16 ")


# ----------------------------------------------------------------------------------------------- the bf16 engines
# tests/test_gpu_net_exact_bf16.py compares the three bf16 forms of the kernel with the references run through net_exact.Bf16Hook.
SERVE_NETS = [n for n in ne.NETS if n not in ne.DENSE_NETS]
ok32 = lambda a: np.array_equal(np.asarray(a, np.float64).astype(F).astype(np.float64), a)


def family(name):
    return "block" if name.startswith("blk") else ne.NETS[name][0] if ne.NETS[name][0] != "custom" else "mlp"


@pytest.mark.parametrize("name", SERVE_NETS)
def test_bf16_serving_tables_round_nothing(name):
    """Every forward A operand, the transformed input and every packed weight of every serving (and slice-point) table is a
    bf16 number: the rounding reference rounds nothing and equals the fp32 integer reference -- lnP, THETA, every activation."""
    for dense, B in ne.sweep_tables(name):
        a, b = ne.serving_table(name, dense, B, grad=name in ne.GRAD_NETS), ne.bf16_serving_table(name, dense, B)
        tag = "%s dense map %d rows %d" % (name, dense, B)
        assert b["hook"].changed == 0 and b["hook"].ties == 0, tag
        assert np.array_equal(a["ref"]["lnP"], b["ref"]["lnP"]) and np.array_equal(a["ref"]["theta"], b["ref"]["theta"]), tag
        for ca, cb in zip(a["ref"]["fwd"], b["ref"]["fwd"]):
            for k in ("x", "h", "y"):
                assert (k not in ca and k not in cb) or np.array_equal(ca[k], cb[k]), (tag, k)
        assert ne.bf16_exact_sum(b["ref"]["exact"]), tag


def test_bf16_serving_table_count():
    """755 of 755 serving tables round nothing (589 of them on the networks the fp32 module already had)."""
    tabs = [(n, d, B) for n in SERVE_NETS for d, B in ne.sweep_tables(n)]
    assert len(tabs) == 755 and sum(ne.bf16_serving_table(*t)["hook"].changed == 0 for t in tabs) == 755


@pytest.mark.parametrize("name", ne.BF16_GRAD_NETS)
def test_bf16_gradient_tables_are_exact(name):
    """With the deltas rounded where the matrix cores read them every sum of every gradient table still meets the exactness
    condition on its ROUNDED operands; lnP, G and both leapfrogs' P and Q are fp32 numbers."""
    nin = ne.model(name).in_size
    for dense, B in ne.sweep_tables(name):
        s = ne.bf16_serving_table(name, dense, B, grad=True)
        ref, tag = s["ref"], "%s dense map %d rows %d" % (name, dense, B)
        assert ne.bf16_exact_sum(ref["exact"]), (tag, ne.bf16_margin(ref["exact"]))
        assert ne.exact_sum(ref["terms"]) and ok32(ref["lnP"]) and ok32(ref["G"]), tag
        eps = 2.0 ** -(1.0 + np.arange(B) % 3)[:, None]
        for ek, ed in ((ne.EPS, ne.EPS), (eps, 0.5 * eps)):
            Pn, Qn = ne.leapfrog_ref(ref["G"], s["z"], ne.momenta(name, dense, B), ne.MASS(nin), ek, ed)
            assert ok32(Pn) and ok32(Qn), tag


@pytest.mark.parametrize("name", SERVE_NETS)
def test_bf16_training_tables_are_exact(name):
    """The dX chain of a bf16 training step on every training table, and the merged training step's loss tables in both
    precisions on the networks the GPU test drives: every sum exact on its rounded operands, every result an fp32 number."""
    n = ne.n_maps(name)
    tabs = [(ne.bf16_table(name, d, B), "%s dense map %d rows %d" % (name, d, B)) for d, B in ne.sweep_tables(name)]
    if name in ne.TRAIN_STEP_NETS:
        tabs += [(ne.loss_table(name, d, B, bf), "%s loss, dense map %d rows %d bf16 %d" % (name, d, B, bf)) for d in range(n)
                 for B in (ne.LOSS_ROWS if d in (0, n - 1) else (ne.ROWS,)) for bf in (False, True)]
    for t, tag in tabs:
        assert ne.bf16_exact_sum(t["exact"]), (tag, ne.bf16_margin(t["exact"]))
        for a in list(t["G"].values()) + [b[w] for b in t["bufs"] for w in b] + [c[k] for c in t["fwd"] for k in ("h", "y") if k in c]:
            assert ok32(a), tag
        if "rows" in t:
            assert ok32(t["rows"]) and ok32(np.array([t["mean"]])) and ok32(t["dpred"]), tag
            assert np.isnan(t["YN"]).any() or t["YN"].size < 64, tag                    # some targets are masked (one in eight)
            m, _ = np.frexp(t["den"])
            assert np.all(m == 0.5) and np.array_equal(t["Cinv"], t["Cinv"].T) and np.array_equal(t["Cinv"], np.round(t["Cinv"])), tag


# gradient tables (of net_exact.sweep_tables) whose deltas round, per network; the networks not listed have none
GRAD_ROUNDS = {"in15_n16": 7, "in16_n17": 6, "in64_n64": 8, "n512_513": 8, "n1000_1024": 8, "grad257": 11, "grad513": 6, "v2_33_33": 25,
               "v2_6_30": 24, "v2_6_31": 25, "simple_6_4": 6, "simple_6_31": 24, "blk_id64": 6, "bf_n64_k512_513": 6, "blk_k20_c32": 1,
               "blk_k40_c15": 2}
# bf16 loss tables of the merged training step, per network: (tables that round, tables with a tie, tables)
LOSS_ROUNDS = {"in1_n1": (9, 9, 12), "in15_n16": (12, 11, 12), "in16_n17": (12, 12, 12), "in17_n32": (10, 8, 13), "k31_63": (11, 8, 13),
               "side16_2": (12, 12, 13), "side32_2": (13, 13, 13), "side64_2": (12, 12, 13), "bf_split_wide": (15, 15, 15),
               "bf_n64_k256_257": (12, 11, 15), "blk_c17": (13, 11, 15), "blk_id17": (11, 9, 14), "blk_c64": (15, 14, 15), "v2_6_31": (23, 23, 23),
               "simple_6_4": (21, 18, 23), "v2_33_33": (23, 23, 23), "blk_k20_c31": (14, 14, 15), "blk_k20_c32": (14, 13, 15),
               "blk_k20_c33": (14, 13, 15), "blk_k40_c15": (13, 11, 15)}


def test_bf16_tables_round_and_tie():
    """The tables can tell nearest-even from truncation, and a delta rounded in the wrong place from one rounded in the right
    one -- where they round.  Gradient: in every family of networks (plain MLP, ChtoModelv2, ChtoModelsimple, custom residual
    block) some table has deltas that are no bf16 numbers, ties among them; GRAD_ROUNDS says, network by network, how many of
    its tables do (none on most of the side*, blk_c* and bf16-edge networks: those check slots and packing on that surface,
    not where the backward rounds).  Training step: the loss tables the GPU test drives round on EVERY network of
    TRAIN_STEP_NETS, with ties (net_exact.loss_consts puts a nine-bit target into every fourth row); LOSS_ROUNDS holds the
    counts.  The dX chain on the fp32 module's dout tables rounds on ChtoModelv2 only (small integer deltas elsewhere)."""
    got = {}
    rounds, ties = {}, {}
    for name in ne.BF16_GRAD_NETS:
        hooks = [ne.bf16_serving_table(name, dense, B, grad=True)["hook"] for dense, B in ne.sweep_tables(name)]
        got[name] = sum(h.changed > 0 for h in hooks)
        rounds[family(name)] = rounds.get(family(name), 0) + got[name]
        ties[family(name)] = ties.get(family(name), 0) + sum(h.ties > 0 for h in hooks)
    assert set(rounds) == {"mlp", "v2", "simple", "block"} and all(v > 0 for v in rounds.values()) and all(v > 0 for v in ties.values()), (rounds, ties)
    assert {k: v for k, v in got.items() if v} == GRAD_ROUNDS, got
    assert sum(got.values()) == 173                         # (164 on the networks the fp32 module already had)
    tr = [ne.bf16_table(n, d, B)["hook"] for n in ("v2_6_31", "v2_26_457") for d, B in ne.sweep_tables(n)]
    assert sum(h.changed > 0 for h in tr) == 18 and sum(h.ties > 0 for h in tr) > 0
    loss = {}
    for name in ne.TRAIN_STEP_NETS:
        n = ne.n_maps(name)
        hooks = [ne.loss_table(name, d, B, True)["hook"] for d in range(n) for B in (ne.LOSS_ROWS if d in (0, n - 1) else (ne.ROWS,))]
        loss[name] = (sum(h.changed > 0 for h in hooks), sum(h.ties > 0 for h in hooks), len(hooks))
    assert loss == LOSS_ROUNDS, loss
    assert all(r >= 9 and t >= 8 for r, t, _ in loss.values())              # every network, most of its tables, ties in them
    # the reference tells the wrong roundings apart on such tables: a plain MLP with a SPLIT backward segment, custom blocks,
    # ChtoModelsimple, ChtoModelv2 -- truncation instead of nearest-even moves a stored delta or a parameter gradient
    trunc = lambda a: (np.ascontiguousarray(a, F).view(np.uint32) & np.uint32(0xFFFF0000)).view(F).astype(np.float64)
    for name in ("bf_split_wide", "side32_2", "blk_c17", "blk_k20_c33", "simple_6_4", "v2_6_31"):
        t = ne.loss_table(name, ne.n_maps(name) - 1, ne.ROWS, True)
        assert t["hook"].ties > 0, name
        _, G, bufs, _ = ne.backward_ref(t["ops"], t["P"], t["fwd"], t["dpred"], rnd=trunc, tens=False)
        assert any(not np.array_equal(G[k], t["G"][k]) for k in G) and any(not np.array_equal(a[w], b[w]) for a, b in zip(bufs, t["bufs"]) for w in a), name
        _, G, _, _ = ne.backward_ref(t["ops"], t["P"], t["fwd"], t["dpred"], rnd=None, tens=False)
        assert any(not np.array_equal(G[k], t["G"][k]) for k in G), name            # (deltas left unrounded)
    # and the reference itself tells the wrong roundings apart on such a table: truncation instead of nearest-even, deltas
    # left unrounded (a hook that rounds nothing), a gate from the unrounded forward (the fp32 reference's G is another one)
    s = ne.bf16_serving_table("v2_6_31", 0, grad=True)
    ops, G = ne.model("v2_6_31").ops, s["ref"]["G"]
    trunc = lambda a: (np.ascontiguousarray(a, F).view(np.uint32) & np.uint32(0xFFFF0000)).view(F).astype(np.float64)
    assert s["hook"].ties > 0
    assert not np.array_equal(ne.serving_ref(ops, s["P"], s["c"], s["z"], grad=True, rnd=trunc)["G"], G)
    assert not np.array_equal(ne.serving_table("v2_6_31", 0, grad=True)["ref"]["G"], G)


@pytest.mark.parametrize("name", ["in17_n32", "v2_6_31", "simple_6_4", "blk_id17", "blk_k20_c33"])
def test_identity_hook_gives_the_unrounded_references(name):
    """Through the hook's code path (the input as hi + lo, the operands passed through ``rnd``) with a hook that rounds
    nothing: the references the fp32 module uses, array for array; and fp32(0.1f * sum) is sum / 10 on multiples of 10."""
    ident = lambda a: np.asarray(a, np.float64)
    ops = ne.model(name).ops
    for dense in sorted({0, ne.n_maps(name) - 1}):
        t = ne.table(name, dense)
        fwd = ne.forward_ref(ops, t["P"], t["x"], ident)
        for ca, cb in zip(t["fwd"], fwd):
            assert all(np.array_equal(ca[k], cb[k]) for k in ("x", "h", "y") if k in ca)
        dX, G, bufs, _ = ne.backward_ref(ops, t["P"], fwd, t["dY"], rnd=ident, tens=False)
        assert np.array_equal(dX, t["dX"]) and all(np.array_equal(G[k], t["G"][k]) for k in t["G"]) and set(G) == set(t["G"])
        assert all(np.array_equal(a[w], b[w]) for a, b in zip(bufs, t["bufs"]) for w in a)
        if name in ne.GRAD_NETS:
            s = ne.serving_table(name, dense, grad=True)
            r = ne.serving_ref(ops, s["P"], s["c"], s["z"], grad=True, rnd=ident)
            assert np.array_equal(r["lnP"], s["ref"]["lnP"]) and np.array_equal(r["G"], s["ref"]["G"]) and np.array_equal(r["theta"], s["ref"]["theta"])


def _prob(name, s):
    c = s["c"]
    kind = {"v2": "ChtoModelv2", "simple": "ChtoModelsimple"}[ne.NETS[name][0]]
    return dict(kind=kind, nin=c["nin"], nout=c["nout"], kw={}, weights=s["P"], priors=c["priors"], X_mean=c["X_mean"], X_std=c["X_std"],
                y_mean=c["y_mean"], y_std=c["y_std"], sigma=c["sigma"], data=c["data"], dolog10=None, ypositive=False)


@pytest.mark.parametrize("name", ["v2_6_31", "v2_33_33", "simple_6_31"])
def test_rounding_references_agree_with_the_bf16_emulations(name):
    """The two descriptions of "where it rounds" are the same one: tests/bf16_emul.py, bf16_grad_emul.py and bf16_train_emul.py
    (what the statistical bf16 tests compare against) on the tables whose deltas DO round, to float64 accuracy."""
    import bf16_emul, bf16_grad_emul, bf16_train_emul
    close = lambda a, b: np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(b).max())))
    m = ne.model(name)
    n = ne.n_maps(name)
    rounded = 0
    for dense in sorted({0, 2, n // 2, n - 1}):
        s = ne.bf16_serving_table(name, dense, grad=True)
        prob, ref = _prob(name, s), s["ref"]
        rounded += s["hook"].changed
        close(bf16_emul.network(s["P"], ref["x"].astype(F), prob["kind"], m.in_size, m.out_size), ref["fwd"][-1]["y"])
        close(bf16_emul.log_prob(s["z"], prob, s["c"]["w"], s["c"]["T"]), ref["lnP"])
        lnp, G = bf16_grad_emul.log_prob_grad(s["z"], prob, s["c"]["w"], s["c"]["T"])
        close(lnp, ref["lnP"])
        close(G, ref["G"])
        for B in (5, 20):
            t = ne.loss_table(name, dense, B, True)
            rows, dpred, grads = bf16_train_emul.train_step(t["P"], t["x"], prob["kind"], m.in_size, m.out_size, t["YN"], t["den"], ne.INV_BATCH, t["Cinv"])
            close(rows, t["rows"])
            close(dpred, t["dpred"])
            assert set(grads) == set(t["G"])
            for k in grads:
                np.testing.assert_allclose(grads[k], t["G"][k], rtol=2.0 ** -23, atol=0)    # (fp32(0.1f * sum) against 0.1 * sum in float64)
    assert rounded > 0


@pytest.fixture(scope="module")
def bf16_plans(tmp_path_factory):
    """{(network, kind, engine rows): (ok, train_ok, ["TYPE steps S passes P ncg G N n K k" per segment])} of the bf16 serving
    program and the bf16 merged training step, from the planner's own dump (tests/net_program_dump.hip, as
    tests/test_net_program_host.py builds it)."""
    import test_net_program_host as tp
    text = []
    for name in ne.NETS:
        lines, _ = tp.layer_lines(ne.model(name))
        for kind, dense in (("SERVE_BF16", 0), ("TRAIN_STEP_BF16", 1)):
            for rows in (16, 8, 4):
                text.append(tp.case_line("%s/%s/%d" % (name, kind, rows), kind, rows, ne.model(name).in_size, dense, 2, len(lines)))
                text.extend(lines)
    summary, full = tp.run_dump(tp.build_dump(tmp_path_factory.mktemp("net_exact_bf16")), "\n".join(text) + "\n")
    plans = {}
    for line in summary:
        case, head = line.split(" | ")[:2]
        segs = ["%s steps %s passes %s ncg %d N %s K %d" % (("WIDE", "SPLIT", "SIDE")[int(sg["type"])], sg["steps"], sg["passes"], 1 << int(sg["ncg_log2"]),
                                                            pk["N"], int(pk["Kapad"]) + int(pk["Kb"]))
                for sg, pk in zip(tp.dump_records(full[case], "seg"), tp.dump_records(full[case], "pack"))]
        train_ok = [int(r["train_ok"]) for r in tp.dump_records(full[case], "nseg")]
        name, kind, rows = case.split("/")
        plans[(name, kind, int(rows))] = (head.startswith("ok") and head.endswith("plan 1"), train_ok[0] if train_ok else 0, segs)
    return plans


# (network, segment index, its line): the bf16 edge each shape is named for -- 32 k per step, ksteps = (Kapad + Kb + 31) / 32, the
# first layer over [x_hi ; x_lo] with no pad between the halves; the same on every engine (asserted), no SIDE segment anywhere
PLAN_BF16 = [
    ("in1_n1", 0, "WIDE steps 1 passes 1 ncg 1 N 1 K 2"),                   # first-layer K of 2 ... 512 (the bf16 limit kpad0 <= 512)
    ("in15_n16", 0, "WIDE steps 1 passes 1 ncg 1 N 16 K 30"),
    ("in16_n17", 0, "WIDE steps 1 passes 1 ncg 1 N 17 K 32"),
    ("in17_n32", 0, "WIDE steps 2 passes 1 ncg 1 N 32 K 34"),
    ("in64_n64", 0, "SPLIT steps 1 passes 1 ncg 1 N 64 K 128"),
    ("in65_n128", 0, "SPLIT steps 2 passes 1 ncg 2 N 128 K 130"),
    ("in256_n256", 0, "SPLIT steps 8 passes 1 ncg 4 N 256 K 512"),
    ("k31_63", 1, "WIDE steps 1 passes 1 ncg 1 N 63 K 32"),                 # hidden K 31: one step with one slot short
    ("k31_63", 2, "WIDE steps 2 passes 1 ncg 1 N 5 K 64"),                  # hidden K 63: two
    ("in17_n32", 2, "WIDE steps 2 passes 1 ncg 1 N 3 K 48"),                # hidden K 33: the second step half empty
    ("n1000_1024", 1, "WIDE steps 32 passes 2 ncg 1 N 1024 K 1008"),        # K = 1000: 32 steps, the last one 8 k + 8 pad + 16 absent
    ("bf_split_wide", 1, "SPLIT steps 1 passes 1 ncg 2 N 128 K 128"),       # split_steps + 3 <= ksteps: 1 + 3 <= 4
    ("bf_split_wide", 3, "WIDE steps 3 passes 1 ncg 1 N 128 K 96"),         # 1 + 3 > 3
    ("split_4k", 1, "WIDE steps 2 passes 1 ncg 1 N 128 K 64"),              # (the fp32 pair is WIDE on both sides in bf16)
    ("bf_n64_k256_257", 1, "SPLIT steps 1 passes 1 ncg 1 N 64 K 256"),      # 64 columns: 8 waves x 32 k = one step up to K = 256
    ("bf_n64_k256_257", 3, "SPLIT steps 2 passes 1 ncg 1 N 64 K 272"),      # 257: two
    ("bf_n64_k512_513", 1, "SPLIT steps 2 passes 1 ncg 1 N 64 K 512"),
    ("bf_n64_k512_513", 3, "SPLIT steps 3 passes 1 ncg 1 N 64 K 528"),      # 513: three
    ("bf_n32_k512_513", 1, "SPLIT steps 2 passes 1 ncg 1 N 32 K 512"),
    ("bf_n32_k512_513", 3, "SPLIT steps 3 passes 1 ncg 1 N 32 K 528"),
    ("bf_n16_k1024", 1, "SPLIT steps 4 passes 1 ncg 1 N 16 K 1024"),
    ("side64_2", 1, "SPLIT steps 1 passes 1 ncg 1 N 64 K 256"),             # K = 250 (the fp32 program's SIDE segments are SPLIT here)
    ("blk_k20_c31", 2, "WIDE steps 2 passes 1 ncg 1 N 24 K 63"),            # [x (32) ; h (31)]: 63 k
    ("blk_k20_c32", 2, "WIDE steps 2 passes 1 ncg 1 N 24 K 64"),
    ("blk_k20_c33", 2, "WIDE steps 3 passes 1 ncg 1 N 24 K 65"),
    ("blk_k40_c15", 2, "WIDE steps 2 passes 1 ncg 1 N 20 K 63"),            # [x (48) ; h (15)]
    ("blk_c17", 2, "WIDE steps 3 passes 1 ncg 1 N 20 K 65"),
]


@pytest.mark.parametrize("name,i,want", PLAN_BF16)
def test_shapes_sit_on_their_bf16_planner_edges(bf16_plans, name, i, want):
    for rows in (16, 8, 4):
        ok, _, segs = bf16_plans[(name, "SERVE_BF16", rows)]
        assert ok and segs[i] == want, "%s on the %d-row engine, segment %d: %s" % (name, rows, i, segs[i])
        ok, train_ok, tsegs = bf16_plans[(name, "TRAIN_STEP_BF16", rows)]
        assert ok and train_ok and tsegs[i] == want, (name, rows, tsegs[i])        # the training step's forward half is the same program


def test_bf16_programs(bf16_plans):
    """Which networks have which bf16 program, as the GPU test relies on it: every network of NETS is served in bf16 and has a
    bf16 merged training step on every engine's plan (the 4-row engine alone runs it); no bf16 program has a SIDE segment; the
    bf16 one-launch gradient exists on every engine for the networks of up to 64 inputs and outputs and for no other."""
    for (name, kind, rows), (ok, train_ok, segs) in bf16_plans.items():
        assert ok and (train_ok or kind == "SERVE_BF16"), (name, kind, rows)
        assert not [s for s in segs if s.startswith("SIDE")], (name, kind, rows)
    for rows in ne.ENGINES:
        have = tuple(n for n in SERVE_NETS if nn.describe_grad_bf16_program(ne.model(n), rows)[0] > 0)
        assert have == ne.BF16_GRAD_NETS, (rows, have)
    assert tuple(n for n in SERVE_NETS if n not in ne.BF16_GRAD_NETS) == ne.BF16_GRAD_REFUSED
    assert all(max(ne.model(n).in_size, ne.model(n).out_size) > 64 for n in ne.BF16_GRAD_REFUSED)
    assert set(ne.TRAIN_STEP_NETS) <= set(SERVE_NETS) and len(set(ne.TRAIN_STEP_NETS)) == len(ne.TRAIN_STEP_NETS)
    n, txt = nn.describe_grad_bf16_program(ne.model("blk_k20_c33"), 4)
    lines = txt.strip().splitlines()
    assert n == 8 and lines[3].startswith("WIDE steps 3 passes 1 ") and not [ln for ln in lines if ln.startswith("SIDE")], txt


def test_plain_programs():
    """Which networks the lean instantiation serves: WIDE and SPLIT segments only."""
    plain = {n for n in ne.NETS if n not in ne.DENSE_NETS and nn.program_is_plain(ne.model(n), 16)}
    assert plain == set(ne.PLAIN_NETS), sorted(plain)
    assert not any(nn.program_is_plain(ne.model(n), 4) for n in ne.NETS)
