"""CPU: the opt-in one-launch gradient of a DENSE inverse covariance (``Log_prob(dense_grad="fused")``,
linna_logprob_set_dense_grad) -- the program the planner builds (forward segments, U = d L, the transposed factor, the dX
chain), where U sits, which engines it fits, what it refuses, that the diagonal programs and their 20-segment limit stand,
the new ABI entries and the instantiations in the code object (no GPU needed)."""
import ctypes
import os
import re

import pytest

import codeobj
import csrc_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "linna_hip.h")
LDS = 160 * 1024
NEW = ("linna_logprob_set_dense_grad", "linna_logprob_dense_grad", "linna_program_describe_grad_dense")


def _model(kind, nin, nout, kw):
    import torch  # noqa: F401
    from linna_amd import nn
    return getattr(nn, kind)(nin, nout, None, **kw)


def plan(model, rows, tri=2):
    """(segments, header fields, segment lines, u_same, u_col, {engine: LDS bytes}, engines that fit)."""
    from linna_amd import nn
    n, txt = nn.describe_grad_dense_program(model, rows, tri)
    lines = txt.strip().splitlines()
    if n == 0:
        return 0, txt
    assert lines[0].startswith("ok ") and len(lines) == 1 + n + 2, txt
    w = lines[0].split()
    hdr = {w[i]: int(w[i + 1]) for i in range(1, len(w) - 1, 2)}
    m = re.fullmatch(r"u_same (\d) u_col (\d+)", lines[n + 1])
    assert m, lines[n + 1]
    last = lines[n + 2]
    per = {int(a): int(b) for a, b in re.findall(r"(\d+):(\d+)", last.split(" of ")[0])}
    assert sorted(per) == [4, 8, 16], last
    f = re.search(r"one launch \(rows((?: \d+)+)\)$", last)
    eng = [int(r) for r in f.group(1).split()] if f else []
    assert f or last.endswith(": layered"), last
    for e in (16, 8, 4):                                     # the engines named are exactly those whose bytes fit
        assert (e in eng) == (0 < per[e] <= LDS), last
    return n, hdr, lines[1:n + 1], int(m.group(1)), int(m.group(2)), per, eng


def seg(line):
    w = line.split()
    d = {w[i]: int(w[i + 1]) for i in range(1, len(w) - 1, 2)}
    d["type"] = w[0]
    return d


def test_small_mlp_u_behind_d_in_the_same_buffer():
    """MLP 5 -> 64 -> 64 -> 7: three layers and L forward, then L^T and three transposed layers."""
    model = _model("MLP", 5, 7, dict(width=64, depth=2))
    for rows in (16, 8, 4):
        n, hdr, segs, u_same, u_col, per, eng = plan(model, rows)
        assert n == 8 and hdr["nseg_f"] == 4, (rows, hdr)
        assert u_same == 1 and u_col == 16
        assert [seg(s)["N"] for s in segs] == [64, 64, 7, 7, 7, 64, 64, 5]
        assert seg(segs[3])["dst"] == 16 and seg(segs[4])["dst"] == 0   # U behind d; the transposed map from column 0
        assert eng == [16, 8, 4]


def test_wide_output_u_in_the_other_buffer():
    model = _model("MLP", 9, 457, dict(width=512, depth=2))
    for rows in (16, 8, 4):
        n, hdr, segs, u_same, u_col, per, eng = plan(model, rows)
        assert n == 8 and hdr["nseg_f"] == 4
        assert u_same == 0 and u_col == 0
        d, b = seg(segs[3]), seg(segs[4])
        assert d["type"] == b["type"] == "WIDE" and d["passes"] == b["passes"] == 1 and d["N"] == b["N"] == 457
        assert b["zext"] == 0                                   # every zero of the transposed factor is multiplied
        assert eng == [16, 8, 4]


def test_two_passes():
    model = _model("MLP", 10, 1000, dict(width=64, depth=1))
    for tri in (0, 1, 2):
        n, hdr, segs, u_same, u_col, per, eng = plan(model, 8, tri)
        assert n == 6 and hdr["nseg_f"] == 3 and u_same == 0
        d, b = seg(segs[2]), seg(segs[3])
        assert d["type"] == b["type"] == "WIDE" and d["passes"] == b["passes"] == 2
        # the forward factor keeps linna_dense_tri's modes; its transpose runs whole in every mode
        assert (d["zext"] == 0) if tri == 0 else (d["zext"] > 0) if tri == 1 else (d["zext"] < 0)
        assert b["zext"] == 0 and b["steps"] == 63
        assert eng


@pytest.mark.parametrize("nin,nout", [(26, 457), (40, 1000)])
def test_chtomodelv2_is_22_segments_and_fits_the_small_engines(nin, nout, capsys):
    model = _model("ChtoModelv2", nin, nout, {})
    fits = None
    for rows in (16, 8, 4):
        n, hdr, segs, u_same, u_col, per, eng = plan(model, rows)
        assert n == 22 and hdr["nseg_f"] == 11 and u_same == 0
        assert seg(segs[10])["N"] == nout and seg(segs[11])["N"] == nout and seg(segs[-1])["N"] == nin
        assert 8 in eng and 4 in eng
        assert fits in (None, eng)
        fits = eng
    with capsys.disabled():
        print("\nChtoModelv2(%d,%d) dense one-launch gradient: LDS %s, engines %s" % (nin, nout, per, fits))


def test_what_is_refused():
    from linna_amd import nn
    for rows in (16, 8, 4):
        n, txt = nn.describe_grad_dense_program(_model("MLP", 70, 33, dict(width=64, depth=1)), rows)
        assert n == 0 and txt.startswith("not eligible"), txt          # 70 inputs: the prologue holds 64
        n, txt = nn.describe_grad_dense_program(_model("ChtoModelv2_linear", 10, 33, {}), rows)
        assert n == 0 and txt.startswith("not eligible"), txt          # an input skip has no dX chain in the launch
    from linna_amd import _lib
    lib = _lib.load()
    arr = nn.program_layers(_model("MLP", 5, 7, dict(width=64, depth=1)))
    buf = ctypes.create_string_buffer(4096)
    assert lib.linna_program_describe_grad_dense(arr, 2, 5, 8, 2, 16, buf, len(buf)) < 0    # 8 columns for 7 outputs
    assert lib.linna_program_describe_grad_dense(arr, 2, 5, 7, 3, 16, buf, len(buf)) < 0    # no such triangle mode
    assert "program_describe_grad_dense" in lib.linna_last_error().decode()


def test_diagonal_programs_keep_their_limit_and_their_text():
    """The tables hold 22 segments now; every other kind is still planned against 20."""
    from linna_amd import nn
    for rows in (16, 8, 4):
        n, txt = nn.describe_program(_model("ChtoModelv2", 26, 457, {}), rows, -1)
        assert n == 20 and txt.startswith("ok "), txt
    # twelve layers: 24 segments with their transposes -- beyond the diagonal one-launch gradient as before, and (26 with
    # the dense pair) beyond the dense one
    deep = _model("MLP", 5, 7, dict(width=64, depth=11))
    assert nn.describe_program(deep, 8, -1)[0] == 0
    assert nn.describe_grad_dense_program(deep, 8)[0] == 0
    # ten layers: 20 diagonal, 22 dense
    ten = _model("MLP", 5, 7, dict(width=64, depth=9))
    assert nn.describe_program(ten, 8, -1)[0] == 20
    assert plan(ten, 8)[0] == 22
    # eleven layers: 22 diagonal segments are refused though the tables would hold them
    assert nn.describe_program(_model("MLP", 5, 7, dict(width=64, depth=10)), 8, -1)[0] == 0
    src = open(os.path.join(ROOT, "linna_amd", "csrc", "net_program.h")).read()
    assert re.search(r"constexpr int NS_MAXSEG = 20;", src) and re.search(r"constexpr int NS_SEGCAP = 22;", src)


def test_entries_header_and_binding():
    from linna_amd import _lib, util
    lib = _lib.load()
    src = open(HEADER).read()
    api = csrc_text.hip_sources()
    assert re.search(r"int linna_logprob_set_dense_grad\(linna_logprob_t\* lp, int on\);", src)
    assert re.search(r"int linna_logprob_dense_grad\(const linna_logprob_t\* lp, int\* out\);", src)
    assert re.search(r"int linna_program_describe_grad_dense\(const linna_layer_t\* layers, int nlayers, int in_size, int nout, int tri, int rows,", src)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.EXPORTED
        assert re.search(r"int %s\([^)]*\) try \{" % name, api), name        # a function-try-block: no exception crosses the ABI
    assert re.search(r"#define LINNA_ABI_VERSION 12\b", src) and _lib.ABI_VERSION == 12 and lib.linna_abi_version() == 12
    out = ctypes.c_int(5)
    assert lib.linna_logprob_set_dense_grad(None, 1) == _lib.ERR_INVALID
    assert "logprob_set_dense_grad" in lib.linna_last_error().decode()
    assert lib.linna_logprob_dense_grad(None, ctypes.byref(out)) == _lib.ERR_INVALID and out.value == 5
    with pytest.raises(ValueError):
        util.Log_prob(None, None, None, None, None, 1.0, dense_grad="one-launch")
    lp = util.Log_prob(None, None, None, None, None, 1.0)
    assert lp.dense_grad == "layered"
    assert util.Log_prob(None, None, None, None, None, 1.0, dense_grad="fused").dense_grad == "fused"


def test_code_object_holds_the_six_dense_instantiations():
    from linna_amd import _lib
    ks = codeobj.kernels(_lib.LIB_PATH)
    mine = [k for k in ks if "net_stream_dense_kernel" in k["name"]]
    # R 6, MOVE 0, GRAD, STORE 2, rows, fp32, EPS
    tags = sorted(re.search(r"net_stream_dense_kernelILi6ELi0ELb1ELi2ELi(\d+)ELb0ELb([01])E", k["name"]).groups() for k in mine)
    assert tags == [("16", "0"), ("16", "1"), ("4", "0"), ("4", "1"), ("8", "0"), ("8", "1")], [k["name"] for k in mine]
    for k in mine:
        assert k["scratch"] == 0 and 0 < k["vgpr"] <= 256, k
        assert "net_stream_wide_kernel" not in k["name"] and not k["name"].startswith("_ZN5linna17net_stream_kernel")
