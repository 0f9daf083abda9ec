"""GPU: the lean ("plain") instantiation of the whole-network serving kernel computes, bit for bit, what the generic
instantiation computes -- compared in one process through ``linna_serve_plain`` on the 16-row engine -- and launches that
are not plain keep the generic one."""
import numpy as np
import pytest

import cases
from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_serving import build_logprob, _custom_problem  # noqa: E402


@pytest.fixture
def engine16():
    rows, plain = _lib.engine_rows(16), _lib.serve_plain(1)
    yield
    _lib.engine_rows(rows)
    _lib.serve_plain(plain)


def both(lp, zd):
    """(plain, generic) lnP of the same rows from the same handle."""
    _lib.serve_plain(1)
    a = lp.evaluate(zd).cpu().numpy()
    _lib.serve_plain(0)
    b = lp.evaluate(zd).cpu().numpy()
    _lib.serve_plain(1)
    return a, b


# nin, nout, width, depth, rows, must be plain
SHAPES = [
    (33, 33, 512, 2, 21, True),       # 33 -> 512 -> 512 -> 33, two workgroups, the second ragged
    (33, 33, 512, 4, 300, True),      # the bench's network
    (9, 33, 1024, 2, 21, True),       # a 1024-wide layer: two WIDE passes
    (20, 100, 256, 3, 37, True),      # hidden 256 <- 256: SPLIT, four column groups x two K parts
    (12, 100, 128, 2, 21, True),      # hidden 128 <- 128: SPLIT, two column groups; 100 outputs (past the finish's registers)
    (5, 3, 40, 1, 21, False),         # 5 -> 40 -> 3: the planner makes the 40 -> 3 layer a SIDE segment (pinned on the CPU): generic
    (5, 100, 40, 1, 21, True),        # the same short-K first layer in front of a short-K WIDE last layer: plain
    (65, 40, 512, 1, 17, True),       # 65 inputs: the prologue's wide-input loop
]


@pytest.mark.parametrize("T", [1.0, 4.0])
@pytest.mark.parametrize("nin,nout,width,depth,B,plain", SHAPES)
def test_plain_equals_generic_bit_for_bit(nin, nout, width, depth, B, plain, T, engine16):
    prob = _custom_problem(nin, nout, 700 + nin + width, width, depth)
    lp = build_logprob(None, temperature=T, prob=prob)[0]
    z = (0.7 * np.random.RandomState(B + nin).standard_normal((B, nin))).astype(np.float32)
    z[min(5, B - 1), nin // 2] = np.nan                         # one non-finite row among finite ones
    zd = torch.as_tensor(z, device="cuda")
    assert lp.serves_plain(B) is plain
    _lib.serve_plain(0)
    assert not lp.serves_plain(B)
    _lib.serve_plain(1)
    a, b = both(lp, zd)
    np.testing.assert_array_equal(a, b)
    assert a[min(5, B - 1)] == -np.inf and np.isfinite(np.delete(a, min(5, B - 1))).all()
    # one row alone, and a strided view of a wider buffer
    np.testing.assert_array_equal(lp.evaluate(zd[:1].contiguous()).cpu().numpy(), b[:1])
    wide = torch.zeros((B, nin + 3), device="cuda")
    wide[:, :nin] = zd
    np.testing.assert_array_equal(lp.evaluate(wide[:, :nin]).cpu().numpy(), b)


def test_plain_against_the_oracle(engine16):
    """The bench's network at 4096 + 5 rows against the numpy oracle, at the tolerance test_gpu_serving.py uses for lnP of
    the whole-network kernel."""
    from oracle import likelihood
    prob = _custom_problem(33, 33, 733, 512, 4)
    lp = build_logprob(None, prob=prob)[0]
    z = (0.7 * np.random.RandomState(11).standard_normal((4101, 33))).astype(np.float32)
    zd = torch.as_tensor(z, device="cuda")
    assert lp.serves_plain(len(z))
    a, b = both(lp, zd)
    np.testing.assert_array_equal(a, b)
    ref = likelihood.log_prob(z, cases.oracle_emulator(prob), prob["priors"], prob["data"], prob["invcov"], 1.0)
    np.testing.assert_allclose(a, ref, rtol=2e-5, atol=4e-5)


def test_theta_output_keeps_the_generic_instantiation(engine16):
    """A launch that also writes the physical parameters is not plain: same lnP, theta written."""
    from oracle import likelihood
    prob = _custom_problem(33, 33, 733, 512, 2)
    lp = build_logprob(None, prob=prob)[0]
    z = (0.7 * np.random.RandomState(3).standard_normal((21, 33))).astype(np.float32)
    zd = torch.as_tensor(z, device="cuda")
    theta = torch.zeros_like(zd)
    with_theta = lp.evaluate(zd, theta=theta).cpu().numpy()
    np.testing.assert_array_equal(with_theta, lp.evaluate(zd).cpu().numpy())
    np.testing.assert_allclose(theta.cpu().numpy(), likelihood.prior_map(z, prob["priors"]), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", ["v2_33_33", "mlp_33_33_dense", "v2_4_2_ypos"])
def test_programs_that_are_not_plain_are_untouched(name, engine16):
    """ChtoModelv2(33,33) (SIDE segments), a dense covariance and a ypositive model: reported "not plain", the switch
    changes nothing, and lnP is the golden one."""
    g = cases.golden(name)
    lp = build_logprob(name, float(g["temps"][0]))[0]
    zd = torch.as_tensor(np.asarray(g["z"], np.float32), device="cuda")
    assert not lp.serves_plain(zd.shape[0])
    a, b = both(lp, zd)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_allclose(a, g["loglike"][:, 0], rtol=2e-5)


def test_small_engines_are_not_plain():
    prob = _custom_problem(33, 33, 733, 512, 2)
    lp = build_logprob(None, prob=prob)[0]
    prev = _lib.engine_rows(0)
    try:
        assert not lp.serves_plain(64)            # 64 rows: the 4-row engine
        for rows in (4, 8):
            _lib.engine_rows(rows)
            assert not lp.serves_plain(4096)
        _lib.engine_rows(16)
        assert lp.serves_plain(64)
    finally:
        _lib.engine_rows(prev)
