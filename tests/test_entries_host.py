"""CPU: the tables and float64 references of tests/entries_ref.py, pinned before a GPU sees them (tests/test_gpu_entries.py
runs the stand-alone ABI entries against them).  The selection reference against torch's reductions, each table against what
its case claims, the exact tables against the 2^24 condition, and the float32 restatement of every non-transcendental
formula against the float64 reference rounded once."""
import numpy as np
import pytest

import entries_ref as R

torch = pytest.importorskip("torch")
F = np.float32


def same(a, b):
    """Value equality; a NaN matches a NaN (-0.0 == 0.0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ----------------------------------------------------------------------------------------------- val_metrics
@pytest.mark.parametrize("n", R.VAL_NS)
def test_val_reference_equals_torch(n):
    for name in R.val_table_names(n):
        loss, frac = R.val_table(n, name)
        ref = R.val_metrics_ref(loss, frac, F(0.75))
        tl, tf = torch.as_tensor(loss), torch.as_tensor(frac)
        want = [0.75, torch.median(tl).item(), torch.max(tf).item(), torch.median(tf).item()]
        assert same(ref, want), (n, name, ref, want)
        assert np.isnan(R.val_metrics_ref(loss, frac, None)[0])


def test_val_tables_hold_what_they_claim():
    assert any(n % 2 == 0 for n in R.VAL_NS) and any(n % 2 == 1 for n in R.VAL_NS) and max(R.VAL_NS) == 65536
    assert {255, 256, 257, 512, 513} <= set(R.VAL_NS)                      # one block, a full block, more than one
    for n in R.VAL_NS:
        names = R.val_table_names(n)
        loss, frac = R.val_table(n, "distinct")
        assert len(np.unique(loss)) == n and len(np.unique(frac)) == n and (n == 1 or not np.array_equal(loss, frac))
        loss, frac = R.val_table(n, "ties")
        assert set(np.unique(loss)) <= {0.0, 1.0, 2.0}
        if n >= 255:
            assert len(np.unique(loss)) < n and np.any(np.signbit(loss) & (loss == 0)) and np.any(~np.signbit(loss) & (loss == 0))
            mid = np.sort(frac)[(n - 1) // 2]
            assert (frac == mid).sum() > 1                                  # the median is a tied value
        if "equal" not in names:
            continue
        loss, frac = R.val_table(n, "equal")
        assert len(np.unique(loss)) == 1 and len(np.unique(frac)) == 1
        loss, frac = R.val_table(n, "inf")
        assert np.isposinf(loss).any() and np.isposinf(frac).any() and not np.isnan(loss).any()
        loss, frac = R.val_table(n, "nan_loss")
        assert np.isnan(loss).sum() == 1 and not np.isnan(frac).any()
        loss, frac = R.val_table(n, "nan_frac")
        assert np.isnan(frac).sum() == 1 and not np.isnan(loss).any()
        assert np.isnan(R.val_table(n, "nan_first")[0][0])
        loss, frac = R.val_table(n, "nan_last")
        assert np.isnan(frac[n - 1]) and np.isnan(frac).sum() == 1
        assert np.isnan(R.val_table(n, "nan_last_loss")[0][n - 1])
    for n in (257, 513):                                                   # the NaN is the ONLY element of the last tile of 256
        assert (n - 1) % 256 == 0


# ----------------------------------------------------------------------------------------------- exact tables: 2^24
def test_exact_layer_tables_stay_below_2_24():
    for B, K, N in R.LAYER_SHAPES:
        t = R.linear_exact_table(B, K, N)
        assert R.exact_ok(R.linear_fwd_terms(t["X"], t["W"], t["b"], t["R"]).reshape(-1, 1))
        t = R.linear_bwd_table(B, K, N)
        a = np.abs
        assert R.exact_ok((a(R.f64(t["dY"])) @ a(R.f64(t["W"]))).reshape(-1, 1), (a(R.f64(t["dY"])).T @ a(R.f64(t["X"]))).reshape(-1, 1))
        assert {-1.0, 0.0, 1.0} <= set(np.unique(t["Xmask"])) or B * K < 8
    for B in R.COLSUM_B:
        for N in R.COLSUM_N:
            assert R.exact_ok(R.colsum_table(B, N).T)


def test_exact_loglike_tables_stay_below_2_24():
    for nout, nin in R.DIAG_SHAPES:
        D, w, Z = R.diag_exact_table(nout, nin, max(R.DIAG_B))
        assert R.exact_ok(R.f64(D) ** 2 * R.f64(w)[None, :], R.f64(Z) ** 2)
    for nout in R.DENSE_NOUT:
        D, S, Z = R.dense_exact_table(nout, 5, max(R.DENSE_B))
        d = np.abs(R.f64(D))
        assert R.exact_ok(((d @ np.abs(R.f64(S))) * d), R.f64(Z) ** 2)


def test_exact_gemm_dot_tables_stay_below_2_24():
    for M, N, K in R.GEMM_EXTRA_SHAPES:
        t = R.gemm_dot_table(M, N, K)
        c = np.abs(R.f64(t["A"])) @ np.abs(R.f64(t["B"])).T + np.abs(R.f64(t["bias"]))[None, :]
        assert R.exact_ok(c * c, c * np.abs(R.f64(t["dw"])))


@pytest.mark.parametrize("nout", (1, 3, 63, 64, 65, 130))
def test_exact_loss_tables_stay_below_2_24(nout):
    for cinv in ("full", "diag"):
        c = R.loss_consts(nout, "exact", cinv)
        assert np.array_equal(c["Cinv"], c["Cinv"].T) and set(np.unique(c["Cinv"])) <= {0.0, 0.5, 1.0, 2.0}
        Y = R.loss_Y(("host", nout), 257, nout)
        pred = R.ints(("hostpred", nout), Y.shape, 2)
        yn = np.nan_to_num(R.loss_targets_ref(c, Y))
        dn = np.where(c["dn"] == F(1e-30), 0, c["dn"]).astype(np.float64)
        for delta in (yn - dn[None, :], yn - R.f64(pred), R.f64(pred) - dn[None, :]):
            assert R.exact_ok(R.chi2_terms(c, delta)[:, None])


# ----------------------------------------------------------------------------------------------- float32 restatements
def test_f32_restatement_layers():
    for B, K, N in R.LAYER_SHAPES:
        t = R.linear_exact_table(B, K, N)
        for alpha in (1.0, 0.5):
            f32 = np.maximum(F(alpha) * (t["X"] @ t["W"].T + t["b"][None, :]) + t["R"], F(0))
            assert np.array_equal(f32, R.round_once(R.linear_fwd_ref(t["X"], t["W"], t["b"], alpha, t["R"], 1)))
        t = R.linear_bwd_table(B, K, N)
        dX, dW, db = R.linear_bwd_ref(t["dY"], t["X"], t["W"], t["Xmask"], 0.5)
        assert np.array_equal(np.where(t["Xmask"] > 0, F(0.5) * (t["dY"] @ t["W"]), F(0)), R.round_once(dX))
        assert np.array_equal(F(0.5) * (t["dY"].T @ t["X"]), R.round_once(dW))
        assert np.array_equal(F(0.5) * t["dY"].sum(0, dtype=F), R.round_once(db))


def test_f32_restatement_loglike():
    for nout, nin in R.DIAG_SHAPES:
        D, w, Z = R.diag_exact_table(nout, nin, 17)
        f32 = (F(-0.5) * ((D * w[None, :]) * D).sum(-1, dtype=F)) / F(R.T_EXACT) + F(-0.5) * (Z * Z).sum(-1, dtype=F)
        assert np.array_equal(f32, R.round_once(R.loglike_diag_ref(D, w, Z, R.T_EXACT)))
    for nout in R.DENSE_NOUT:
        D, S, Z = R.dense_exact_table(nout, 5, 65)
        f32 = (F(-0.5) * ((D @ S) * D).sum(-1, dtype=F)) / F(R.T_EXACT) + F(-0.5) * (Z * Z).sum(-1, dtype=F)
        assert np.array_equal(f32, R.round_once(R.loglike_dense_ref(D, S, Z, R.T_EXACT)))
    D, w, Z = R.diag_exact_table(33, 5, 3)
    D[1, 2] = np.nan
    Z[2, 0] = np.nan
    ref = R.loglike_diag_ref(D, w, Z, R.T_EXACT)
    assert np.isneginf(ref[1]) and np.isneginf(ref[2]) and np.isfinite(ref[0])


def test_loglike_diag_lanes_per_row_cover():
    assert sorted({R.diag_lanes_per_row(a, b) for a, b in R.DIAG_SHAPES}) == [4, 8, 16, 32, 64]
    assert [R.diag_lanes_per_row(a, b) for a, b in R.DIAG_RANDOM] == [4, 8, 16, 32, 64]
    assert [R.diag_lanes_per_row(a, b) for a, b in ((3, 17), (3, 65), (5, 129))] == [8, 32, 64]    # the prior row picks it


def test_f32_restatement_prior_map():
    for nin in R.PRIOR_NIN:
        t = R.prior_table(nin, 300)
        alg = t["algebra"]
        assert alg.any() and set(np.unique(t["Z"])) == set(R.Z_GRID.tolist()) or nin < 5
        x64, th64 = R.prior_fwd_ref(t)
        x32, th32 = R.prior_fwd_f32(t)
        assert np.array_equal(x32[:, alg], R.round_once(x64[:, alg])) and np.array_equal(th32[:, alg], R.round_once(th64[:, alg]))
        assert np.array_equal(R.prior_bwd_f32(t)[:, alg], R.round_once(R.prior_bwd_ref(t)[:, alg]))
        assert not np.isinf(x64).any()                                     # log10 of theta <= 0 is a NaN, never an infinity
        if nin >= 5:
            lgc = (t["lg"] != 0) & (t["is_flat"] == 0)
            assert np.isnan(x64[:, lgc]).any() and np.any(th64[:, lgc] == 0) and np.any(th64[:, lgc] < 0)
            assert np.isfinite(x64[:, t["is_flat"] != 0]).all() and np.isfinite(th64).all()


def test_f32_restatement_gather_and_targets():
    for B in R.XFORM_B:
        for w in R.XFORM_W:
            t = R.gather_table(B, w)
            plain = t["lg"] == 0
            for name, rows in R.rows_tables(B, t["ntot"]).items():
                ref = R.gather_xform_ref(t, rows)
                assert np.isfinite(ref).all()
                assert np.array_equal(R.gather_xform_f32(t, rows)[:, plain], R.round_once(ref[:, plain]))
                if name == "repeat":
                    assert rows[-1] == t["ntot"] - 1 and (B == 1 or len(np.unique(rows)) < B)
            c = R.loss_consts(w, "exact")
            Y = R.loss_Y(("targets", B, w), B + 3, w)
            ref = R.loss_targets_ref(c, Y)
            f32 = (Y / c["sigma"][None, :] - c["ymean"][None, :]) / c["ystd"][None, :]
            ok = ~np.isnan(ref)
            assert np.array_equal(f32[ok], R.round_once(ref[ok]))
            assert np.isnan(ref[1, 0]) and np.isnan(ref[2, w - 1]) and (w < 2 or np.isnan(ref[:, 1]).all())


@pytest.mark.parametrize("nout", (1, 3, 63, 64, 65, 130))
def test_chi2_md_rows_below_at_and_above_the_floor(nout):
    """With Cinv = I / 2: delta = 0 gives chi2 = 0 (below), |delta_j| = 1 everywhere gives nout / 2 (at), 2 gives 2 nout."""
    c = R.loss_consts(nout, "exact", "diag")
    Y = R.floor_Y(c)
    den = R.chi2_md_ref(c, Y)
    assert not np.any(c["dn"] == F(1e-30)) and np.array_equal(Y, Y.astype(F))
    assert den.tolist() == [0.5 * nout, 0.5 * nout, 2.0 * nout, 0.5 * nout]
    chi2 = 0.5 * (np.nan_to_num(R.loss_targets_ref(c, Y)) - R.f64(c["dn"])[None, :]) ** 2
    assert chi2.sum(-1).tolist() == [0.0, 0.5 * nout, 2.0 * nout, 0.5 * (nout - 1)]
    assert np.array_equal(R.round_once(den), den)


def test_adamw_reference_constants():
    for step in (1, 2, 3, 10000):
        bc1, sbc2 = R.adamw_bc(step)
        assert 0 < bc1 <= 1 and 0 < sbc2 <= 1
    p, g = R.adamw_table(257)
    assert np.all(g[:, 0] == 0) and np.all(np.sign(g[0, 1:]) == np.sign(g[2, 1:]))
    p1, m1, v1 = R.adamw_ref(p, g[0], np.zeros_like(p), np.zeros_like(p), 1, R.LR, 1e-4)
    assert m1[0] == 0 and v1[0] == 0 and p1[0] == float(p[0]) * float(F(1 - float(R.LR) * float(F(1e-4))))
