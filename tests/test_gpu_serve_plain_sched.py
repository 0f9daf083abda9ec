"""GPU: the plain serving launch with its step placed by hand (``net_stream_placed_kernel``, the default) computes, bit for
bit, what the plain instantiation with the compiler-scheduled step and the generic instantiation compute -- all three
compared in one process through ``linna_serve_plain_sched`` / ``linna_serve_plain`` on the 16-row engine.  Random,
asymmetric weights: a ring slot, a tile or a k index taken for another changes bits.  The shapes are chosen by the steps
per wave ``G`` of their programs (``linna_program_describe``, read on the CPU): every ``G mod 6`` (the ring has six slots,
the tail of the stream refills nothing), ``G < 6`` (the prefetch is shorter than the ring), runs of one to three steps,
two WIDE passes, SPLIT layers of 256 and 128 columns, 65 inputs."""
import numpy as np
import pytest

from linna_amd import _lib

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_serving import build_logprob, _custom_problem  # noqa: E402

VARIANTS = {"hand": (1, 1), "sched": (1, 0), "generic": (0, 1)}      # (linna_serve_plain, linna_serve_plain_sched)


@pytest.fixture
def engine16():
    rows, plain, sched = _lib.engine_rows(16), _lib.serve_plain(1), _lib.serve_plain_sched(1)
    yield
    _lib.engine_rows(rows)
    _lib.serve_plain(plain)
    _lib.serve_plain_sched(sched)


def three(lp, zd):
    """lnP of the same rows from the same handle by the three instantiations."""
    out = {}
    for name, (plain, sched) in VARIANTS.items():
        _lib.serve_plain(plain)
        _lib.serve_plain_sched(sched)
        out[name] = lp.evaluate(zd).cpu().numpy()
    _lib.serve_plain(1)
    _lib.serve_plain_sched(1)
    return out


def program(nin, nout, width, depth):
    """(G, [(kind, steps, passes)]) of the forward program on the 16-row engine."""
    from linna_amd import nn
    m = nn.MLP(nin, nout, None, width=width, depth=depth)
    assert nn.program_is_plain(m, 16)
    text = nn.describe_program(m, 16)[1].splitlines()
    hdr = text[0].split()
    nfwd = int(hdr[hdr.index("nseg_f") + 1])
    segs = [(ln.split()[0], int(ln.split()[2]), int(ln.split()[4])) for ln in text[1:1 + nfwd]]
    return int(hdr[hdr.index("G") + 1]), segs


# nin, nout, width, depth, G of the program
SHAPES = [
    (9, 33, 1024, 2, 138),      # G mod 6 = 0; a 1024-wide layer: two WIDE passes of 64 steps
    (33, 33, 512, 1, 7),        # 1
    (20, 33, 512, 2, 38),       # 2
    (65, 40, 512, 1, 9),        # 3; 65 inputs: the prologue's wide-input loop, a first run of five steps
    (20, 100, 256, 3, 22),      # 4; hidden 256 <- 256: SPLIT, four column groups
    (12, 100, 128, 2, 5),       # 5, and G < 6; hidden 128 <- 128: SPLIT, two column groups, runs of one and two steps
    (5, 100, 40, 1, 4),         # G < 6 again: WIDE runs of one and three steps
    (33, 33, 512, 4, 103),      # the bench's network
]


@pytest.mark.parametrize("nin,nout,width,depth,G", SHAPES)
def test_hand_placed_equals_compiler_scheduled_equals_generic(nin, nout, width, depth, G, engine16):
    prob = _custom_problem(nin, nout, 1300 + nin + width + depth, width, depth)
    lp = build_logprob(None, prob=prob)[0]
    for B in (1, 21, 300):              # one row; two workgroups, the second ragged; nineteen workgroups
        z = (0.7 * np.random.RandomState(B + nin).standard_normal((B, nin))).astype(np.float32)
        bad = min(5, B - 1) if B > 1 else None
        if bad is not None:
            z[bad, nin // 2] = np.nan                             # one non-finite row among finite ones
        zd = torch.as_tensor(z, device="cuda")
        assert lp.serves_plain(B)
        r = three(lp, zd)
        np.testing.assert_array_equal(r["hand"], r["sched"])
        np.testing.assert_array_equal(r["hand"], r["generic"])
        if bad is None:
            assert np.isfinite(r["hand"]).all()
        else:
            assert r["hand"][bad] == -np.inf and np.isfinite(np.delete(r["hand"], bad)).all()
        # three launches in a row on one handle, the hand-placed step: nothing of a launch leaks into the next
        for _ in range(3):
            np.testing.assert_array_equal(lp.evaluate(zd).cpu().numpy(), r["generic"])


def test_the_switch_leaves_other_launches_alone(engine16):
    """A launch that also writes theta is not plain: the generic instantiation whatever ``linna_serve_plain_sched`` says."""
    prob = _custom_problem(33, 33, 733, 512, 2)
    lp = build_logprob(None, prob=prob)[0]
    z = (0.7 * np.random.RandomState(3).standard_normal((21, 33))).astype(np.float32)
    zd = torch.as_tensor(z, device="cuda")
    theta = torch.zeros_like(zd)
    with_theta = {}
    for sched in (1, 0):
        _lib.serve_plain_sched(sched)
        with_theta[sched] = lp.evaluate(zd, theta=theta).cpu().numpy()
    _lib.serve_plain_sched(1)
    np.testing.assert_array_equal(with_theta[0], with_theta[1])
    np.testing.assert_array_equal(with_theta[1], lp.evaluate(zd).cpu().numpy())
