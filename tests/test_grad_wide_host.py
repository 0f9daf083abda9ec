"""CPU: the fp32 one-launch gradient (lnP and d lnP / d z in one launch of the whole-network kernel) for networks with more
than 64 outputs -- what the planner accepts and on which engines, what it still refuses, the new ABI entry, and the
wide-output instantiations in the code object (no GPU needed)."""
import ctypes
import os
import re

import pytest

import codeobj
import csrc_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "linna_hip.h")
LDS = 160 * 1024

WIDE = [("MLP", 10, 65, dict(width=64, depth=1)), ("MLP", 12, 100, dict(width=128, depth=2)), ("MLP", 20, 250, dict(width=256, depth=3)),
        ("MLP", 9, 457, dict(width=512, depth=2)), ("MLP", 9, 700, dict(width=1000, depth=2)), ("ChtoModelv2", 26, 457, {}),
        ("ChtoModelv2", 40, 1000, {})]


def _model(kind, nin, nout, kw):
    import torch  # noqa: F401
    from linna_amd import nn
    return getattr(nn, kind)(nin, nout, None, **kw)


def engines_of(last):
    """(engines the launch fits, {engine: LDS bytes}) from the last line of a gradient program's text."""
    assert last.startswith("lds ") and "sign-bit columns: " in last, last
    tail = last.split("sign-bit columns: ")[1]
    m = re.fullmatch(r"one launch \(rows((?: \d+)+)\)", tail)
    if m:                                                   # not on every engine: each engine's bytes are printed
        per = {int(a): int(b) for a, b in re.findall(r"(\d+):(\d+)", last.split(" of ")[0])}
        assert sorted(per) == [4, 8, 16], last
        return [int(r) for r in m.group(1).split()], per
    assert tail == "one launch", last
    return [16, 8, 4], {16: int(last.split()[1])}           # (the 16-row figure bounds the smaller engines')


@pytest.mark.parametrize("kind,nin,nout,kw", WIDE, ids=["%s-%d-%d" % c[:3] for c in WIDE])
def test_wide_outputs_have_a_one_launch_gradient_program(kind, nin, nout, kw):
    """``describe_program(model, rows, -1)``: a program where the planner refused anything beyond 64 outputs, forward
    segments then the dX chain, and a last line that names the engines whose LDS holds it with its sign bits."""
    from linna_amd import nn
    model = _model(kind, nin, nout, kw)
    fits = None
    for rows in (16, 8, 4):
        n, txt = nn.describe_program(model, rows, -1)
        lines = txt.strip().splitlines()
        assert n > 0 and lines[0].startswith("ok "), (rows, txt)
        assert len(lines) == 1 + n + 1
        nseg_f = int(lines[0].split()[lines[0].split().index("nseg_f") + 1])
        assert n > nseg_f and lines[nseg_f].endswith("N %d" % nout) and lines[n].endswith("N %d" % nin), txt
        eng, per = engines_of(lines[-1])
        assert eng, lines[-1]
        for e in eng:
            assert 0 < per.get(e, per[16]) <= LDS, lines[-1]
        for e in set(per) - set(eng):
            assert per[e] > LDS or per[e] == 0, lines[-1]
        assert fits in (None, eng)                          # the same answer whichever engine's program is printed
        fits = eng
    if kind == "ChtoModelv2":
        assert n == 20                                      # exactly NS_MAXSEG segments at any nout
        assert 8 in fits and 4 in fits
    else:
        assert fits == [16, 8, 4]


def test_what_is_still_refused():
    from linna_amd import nn
    n, txt = nn.describe_grad_bf16_program(_model("MLP", 33, 65, dict(width=64, depth=1)), 16)
    assert n == 0 and txt.startswith("not eligible"), txt                  # the bf16 gradient keeps its 64-output limit
    for rows in (16, 8, 4):
        n, txt = nn.describe_program(_model("MLP", 65, 33, dict(width=64, depth=1)), rows, -1)
        assert n == 0 and txt.startswith("not eligible"), txt              # 65 inputs: the prologue holds 64
        n, txt = nn.describe_program(_model("MLP", 12, 1100, dict(width=64, depth=1)), rows, -1)
        assert n == 0 and txt.startswith("not eligible"), txt              # wider than the kernel


# ChtoModelv2(33, 33): header and last line of the text on each engine, captured from the build before the limit was lifted
V2_33 = {
    16: ("ok G 107 Gstride 219 nseg_f 10 LD 1092 kpad0 48 packed_floats 1872192 grad 0", 20),
    8: ("ok G 121 Gstride 240 nseg_f 10 LD 1092 kpad0 48 packed_floats 1970496 grad 0", 20),
    4: ("ok G 121 Gstride 240 nseg_f 10 LD 1092 kpad0 48 packed_floats 1970496 grad 0", 20),
}
V2_33_LAST = "lds 162944 of 163840 bytes with 2688 sign-bit columns: one launch"


@pytest.mark.parametrize("rows", [16, 8, 4])
def test_programs_that_fit_every_engine_keep_their_text(rows):
    from linna_amd import nn
    n, txt = nn.describe_program(_model("ChtoModelv2", 33, 33, {}), rows, -1)
    lines = txt.strip().splitlines()
    assert (lines[0], n) == V2_33[rows]
    assert lines[-1] == V2_33_LAST
    assert txt.endswith("one launch\n")


def test_entry_header_and_binding():
    from linna_amd import _lib
    lib = _lib.load()
    src = open(HEADER).read()
    assert re.search(r"int linna_logprob_grad_launches\(linna_logprob_t\* lp, int B, int\* out\);", src)
    assert hasattr(lib, "linna_logprob_grad_launches") and "linna_logprob_grad_launches" in _lib.EXPORTED
    assert re.search(r"#define LINNA_ABI_VERSION 12\b", src) and lib.linna_abi_version() == 12
    api = csrc_text.hip_sources()
    assert re.search(r"int linna_logprob_grad_launches\(linna_logprob_t\* lp, int B, int\* out\) try \{", api)
    # bad arguments are refused on the host, with a text, and leave *out alone
    out = ctypes.c_int(7)
    assert lib.linna_logprob_grad_launches(None, 4, ctypes.byref(out)) == _lib.ERR_INVALID and out.value == 7
    assert "logprob_grad_launches" in lib.linna_last_error().decode()
    dummy = ctypes.create_string_buffer(64)
    assert lib.linna_logprob_grad_launches(ctypes.cast(dummy, ctypes.c_void_p), 0, ctypes.byref(out)) == _lib.ERR_INVALID
    assert lib.linna_logprob_grad_launches(ctypes.cast(dummy, ctypes.c_void_p), 4, None) == _lib.ERR_INVALID
    from linna_amd import util
    assert callable(util.Log_prob.grad_launches)


def test_code_object_holds_the_six_wide_instantiations():
    from linna_amd import _lib
    ks = codeobj.kernels(_lib.LIB_PATH)
    mine = [k for k in ks if "net_stream_wide_kernel" in k["name"]]
    # R 6, MOVE 0, GRAD, STORE 2, rows, fp32, EPS
    tags = sorted(re.search(r"net_stream_wide_kernelILi6ELi0ELb1ELi2ELi(\d+)ELb0ELb([01])E", k["name"]).groups() for k in mine)
    assert tags == [("16", "0"), ("16", "1"), ("4", "0"), ("4", "1"), ("8", "0"), ("8", "1")], [k["name"] for k in mine]
    for k in mine:
        assert k["scratch"] == 0 and 0 < k["vgpr"] <= 256, k
        # none is counted by the bf16 tests' name patterns
        assert "net_stream_grad_bf16_kernel" not in k["name"] and not k["name"].startswith("_ZN5linna17net_stream_kernel")
        assert not k["name"].startswith("_ZN5linna28net_stream_train_bf16_kernel")
