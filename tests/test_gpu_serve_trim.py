"""GPU: the hand-placed plain serving launch without the MFMAs on zero padding (``net_stream_trim_kernel``, the default)
computes, bit for bit, what the hand-placed kernel (``linna_serve_plain_trim(0)``) and the generic instantiation compute --
compared in one process on the 16-row engine.  Random, asymmetric weights: a ring slot, a tile or a k slice taken for another
changes bits.  The shapes are those of tests/test_serve_trim_host.py, whose liveness is worked out by hand there: S1 at runs of
one, two, three and five steps and at the end of each of two passes, T3 in SPLIT and WIDE last layers, T3 beside the full text
within one run, a run that is both T3 and S1, every ``G mod 6``; one problem with a log10 input index (the prologue)."""
import numpy as np
import pytest

from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_serving import build_logprob, _custom_problem  # noqa: E402
from test_serve_trim_host import SHAPES  # noqa: E402

VARIANTS = {"trim": (1, 1), "placed": (1, 0), "generic": (0, 1)}      # (linna_serve_plain, linna_serve_plain_trim)


@pytest.fixture
def engine16():
    rows, plain, sched, trim = _lib.engine_rows(16), _lib.serve_plain(1), _lib.serve_plain_sched(1), _lib.serve_plain_trim(1)
    yield
    _lib.engine_rows(rows)
    _lib.serve_plain(plain)
    _lib.serve_plain_sched(sched)
    _lib.serve_plain_trim(trim)


def three(lp, zd):
    """lnP of the same rows from the same handle by the three instantiations."""
    out = {}
    for name, (plain, trim) in VARIANTS.items():
        _lib.serve_plain(plain)
        _lib.serve_plain_trim(trim)
        out[name] = lp.evaluate(zd).cpu().numpy()
    _lib.serve_plain(1)
    _lib.serve_plain_trim(1)
    return out


@pytest.mark.parametrize("nin,nout,width,depth,G", [s[:5] for s in SHAPES])
def test_trimmed_equals_hand_placed_equals_generic(nin, nout, width, depth, G, engine16):
    prob = _custom_problem(nin, nout, 2100 + nin + width + depth, width, depth)
    lp = build_logprob(None, prob=prob)[0]
    for B in (1, 21, 300):              # one row; two workgroups, the second ragged; nineteen workgroups
        z = (0.7 * np.random.RandomState(B + nin).standard_normal((B, nin))).astype(np.float32)
        bad = []
        if B > 1:                       # two non-finite rows among finite ones
            bad = [5, 17]
            z[5, nin // 2] = np.nan
            z[17, 0] = np.inf
        zd = torch.as_tensor(z, device="cuda")
        assert lp.serves_plain(B)
        r = three(lp, zd)
        np.testing.assert_array_equal(r["trim"], r["placed"])
        np.testing.assert_array_equal(r["trim"], r["generic"])
        assert (r["trim"][bad] == -np.inf).all() and np.isfinite(np.delete(r["trim"], bad)).all()
        # three launches in a row on one handle, the trimmed kernel: nothing of a launch leaks into the next
        for _ in range(3):
            np.testing.assert_array_equal(lp.evaluate(zd).cpu().numpy(), r["generic"])


def test_a_log10_input_index(engine16):
    """The trimmed kernel's prologue computes ``log10f`` only when the launch has a log10 index: with one (parameter 0, a flat
    prior on positive values) the three instantiations still agree bit for bit, and a launch without one follows on the same
    process."""
    prob = _custom_problem(33, 33, 2177, 512, 2)
    prob["dolog10"] = [0]
    prob["priors"][0] = {"param": "p0", "dist": "flat", "arg1": 0.1, "arg2": 2.0}
    lp = build_logprob(None, prob=prob)[0]
    same = _custom_problem(33, 33, 2177, 512, 2)                        # the same problem without the index
    same["priors"][0] = dict(prob["priors"][0])
    plain = build_logprob(None, prob=same)[0]
    for B in (21, 300):
        z = (0.7 * np.random.RandomState(B).standard_normal((B, 33))).astype(np.float32)
        zd = torch.as_tensor(z, device="cuda")
        assert lp.serves_plain(B)
        r = three(lp, zd)
        np.testing.assert_array_equal(r["trim"], r["placed"])
        np.testing.assert_array_equal(r["trim"], r["generic"])
        assert np.isfinite(r["trim"]).all()
        q = three(plain, zd)
        np.testing.assert_array_equal(q["trim"], q["generic"])
        assert not np.array_equal(q["trim"], r["trim"])             # (the index is not ignored)


def test_the_switch_leaves_other_launches_alone(engine16):
    """A launch that also writes theta is not plain: the generic instantiation whatever ``linna_serve_plain_trim`` says."""
    prob = _custom_problem(33, 33, 733, 512, 2)
    lp = build_logprob(None, prob=prob)[0]
    z = (0.7 * np.random.RandomState(3).standard_normal((21, 33))).astype(np.float32)
    zd = torch.as_tensor(z, device="cuda")
    theta = torch.zeros_like(zd)
    with_theta = {}
    for trim in (1, 0):
        _lib.serve_plain_trim(trim)
        with_theta[trim] = lp.evaluate(zd, theta=theta).cpu().numpy()
    _lib.serve_plain_trim(1)
    np.testing.assert_array_equal(with_theta[0], with_theta[1])
    np.testing.assert_array_equal(with_theta[1], lp.evaluate(zd).cpu().numpy())
