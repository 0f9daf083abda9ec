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


def test_plain_programs():
    """Which networks the lean instantiation serves: WIDE and SPLIT segments only."""
    plain = {n for n in ne.NETS if n not in ne.DENSE_NETS and nn.program_is_plain(ne.model(n), 16)}
    assert plain == set(ne.PLAIN_NETS), sorted(plain)
    assert not any(nn.program_is_plain(ne.model(n), 4) for n in ne.NETS)
