"""CPU: the trimmed hand-placed serving launch (``net_stream_trim_kernel``) -- its process-wide switch, what the code-object
metadata says about the kernel, and the liveness the launcher derives for it (``linna_program_trim``) against values worked
out by hand for the shapes tests/test_gpu_serve_trim.py runs."""
import os
import re
import subprocess

import pytest

import codeobj
from linna_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIM = "_ZN5linna22net_stream_trim_kernelILi6EEEvNS_6NsArgsE"
PLACED = "_ZN5linna24net_stream_placed_kernelILi6EEEvNS_6NsArgsE"
PLAIN = "_ZN5linna23net_stream_plain_kernelILi6EEEvNS_6NsArgsE"

F, T3, S1 = "full", "T3", "S1"
# nin, nout, width, depth, G, then per forward segment (kind, steps, passes, slive per K part, tlive and text per (pass, wave))
# -- hidden 512 <- 512 layers are ("WIDE", 32, 1, [4], [4] * 8, [F] * 8) and are filled in by `expected`
SHAPES = [
    (33, 33, 512, 4, 103, ("WIDE", 3, 1, [1], [4] * 8, [S1] * 8), ("SPLIT", 4, 1, [4] * 8, [3] * 8, [T3] * 8)),
    (17, 40, 512, 1, 6, ("WIDE", 2, 1, [1], [4] * 8, [S1] * 8), ("SPLIT", 4, 1, [4] * 8, [3] * 8, [T3] * 8)),
    (1, 48, 512, 1, 5, ("WIDE", 1, 1, [1], [4] * 8, [S1] * 8), ("SPLIT", 4, 1, [4] * 8, [3] * 8, [T3] * 8)),
    (34, 49, 512, 1, 7, ("WIDE", 3, 1, [2], [4] * 8, [F] * 8), ("SPLIT", 4, 1, [4] * 8, [4] * 8, [F] * 8)),
    (32, 33, 512, 1, 6, ("WIDE", 2, 1, [4], [4] * 8, [F] * 8), ("SPLIT", 4, 1, [4] * 8, [3] * 8, [T3] * 8)),
    (65, 40, 512, 1, 9, ("WIDE", 5, 1, [1], [4] * 8, [S1] * 8), ("SPLIT", 4, 1, [4] * 8, [3] * 8, [T3] * 8)),
    (20, 33, 512, 2, 38, ("WIDE", 2, 1, [4], [4] * 8, [F] * 8), ("SPLIT", 4, 1, [4] * 8, [3] * 8, [T3] * 8)),
    (49, 17, 512, 2, 40, ("WIDE", 4, 1, [1], [4] * 8, [S1] * 8), ("SPLIT", 4, 1, [4] * 8, [2] * 8, [F] * 8)),
    (33, 16, 512, 1, 7, ("WIDE", 3, 1, [1], [4] * 8, [S1] * 8), ("SPLIT", 4, 1, [4] * 8, [1] * 8, [F] * 8)),
    # 256 columns over eight waves: the upper four hold none.  Last layer: two column groups, the second of 36 columns
    (20, 100, 256, 3, 22, ("WIDE", 2, 1, [4], [4] * 4 + [0] * 4, [F] * 8), ("SPLIT", 4, 1, [4] * 4, [4, 3] * 4, [F, T3] * 4)),
    # a WIDE last layer of 300 columns: wave 4 holds 44 of them, waves 5-7 none
    (33, 300, 512, 1, 35, ("WIDE", 3, 1, [1], [4] * 8, [S1] * 8), ("WIDE", 32, 1, [4], [4] * 4 + [3, 0, 0, 0], [F] * 4 + [T3, F, F, F])),
    (9, 33, 1024, 2, 138, ("WIDE", 1, 2, [4], [4] * 16, [F] * 16), ("SPLIT", 8, 1, [4] * 8, [3] * 8, [T3] * 8)),
    # S1 at the end of EACH of two passes (the run's count and the text choice start again with the second pass)
    (33, 33, 1024, 1, 14, ("WIDE", 3, 2, [1], [4] * 16, [S1] * 16), ("SPLIT", 8, 1, [4] * 8, [3] * 8, [T3] * 8)),
    # a 33-wide hidden layer: wave 0 of the first layer T3 in a run of one step; the last layer 33 -> 100 is WIDE with Ka 33, three
    # steps: wave 1 holds 36 columns and is BOTH T3 and S1 (two T3 steps, then the S1 step), the other waves S1
    (5, 100, 33, 1, 4, ("WIDE", 1, 1, [4], [3] + [0] * 7, [T3] + [F] * 7), ("WIDE", 3, 1, [1], [4, 3] + [0] * 6, [S1, "T3+S1"] + [S1] * 6)),
]


def expected(width, depth, first, last):
    if width == 512:
        hidden = [("WIDE", 32, 1, [4], [4] * 8, [F] * 8)] * (depth - 1)
    elif width == 1024:
        hidden = [("WIDE", 64, 2, [4], [4] * 16, [F] * 16)] * (depth - 1)
    elif depth == 1:
        hidden = []
    else:                                   # 256 <- 256: SPLIT, four column groups, two K parts of eight steps
        hidden = [("SPLIT", 8, 1, [4, 4], [4] * 8, [F] * 8)] * (depth - 1)
    return [first] + hidden + [last]


def trim(nin, nout, width, depth):
    """(G, [(kind, steps, passes, slive, tlive, text)]) from ``linna_program_trim``; the shape must be plain."""
    from linna_amd import nn
    m = nn.MLP(nin, nout, None, width=width, depth=depth)
    assert nn.program_is_plain(m, 16)
    n, text = nn.program_trim(m, 16)
    lines = text.splitlines()
    hdr = lines[0].split()
    assert hdr[0] == "plain" and n == len(lines) - 1 == int(hdr[hdr.index("nseg_f") + 1])
    segs = []
    for ln in lines[1:]:
        w = ln.split()
        i, j, k = w.index("slive"), w.index("tlive"), w.index("text")
        segs.append((w[0], int(w[2]), int(w[4]), [int(x) for x in w[i + 1:j]], [int(x) for x in w[j + 1:k]], w[k + 1:]))
    return int(hdr[hdr.index("G") + 1]), segs


def test_switch_without_a_gpu():
    """``linna_serve_plain_trim``: process-wide, -1 queries, returns the previous value, refuses anything else with
    LINNA_ERR_INVALID and a text, and a refused call changes nothing."""
    lib = _lib.load()
    prev = lib.linna_serve_plain_trim(-1)
    assert prev in (0, 1)
    try:
        assert lib.linna_serve_plain_trim(0) == prev and lib.linna_serve_plain_trim(-1) == 0
        assert lib.linna_serve_plain_trim(1) == 0 and lib.linna_serve_plain_trim(-1) == 1
        rc = lib.linna_serve_plain_trim(2)
        assert rc < 0 and "linna_serve_plain_trim" in lib.linna_last_error().decode()
        assert lib.linna_serve_plain_trim(-1) == 1
        assert _lib.serve_plain_trim(0) == 1 and _lib.serve_plain_trim() == 0
    finally:
        lib.linna_serve_plain_trim(prev)


def test_the_default_in_a_fresh_process():
    code = "from linna_amd import _lib; print(_lib.load().linna_serve_plain_trim(-1))"
    out = subprocess.run([os.sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip() == "1"


def test_header_entries():
    src = open(os.path.join(ROOT, "include", "linna_hip.h")).read()
    assert re.search(r"int linna_serve_plain_trim\(int on\);", src)
    assert re.search(r"int linna_program_trim\(const linna_layer_t\* layers, int nlayers, int in_size, int rows, char\* buf, size_t n\);", src)


def test_the_kernel_fits_two_waves_per_simd():
    """The trimmed kernel beside the plain and the hand-placed one: no scratch, at most 256 registers (two waves per SIMD)."""
    ks = {k["name"]: k for k in codeobj.kernels(_lib.LIB_PATH)}
    assert TRIM in ks and PLAIN in ks and PLACED in ks
    assert sum("net_stream_placed_kernel" in n for n in ks) == 1 and sum("net_stream_trim_kernel" in n for n in ks) == 1
    assert ks[TRIM]["scratch"] == 0 and ks[TRIM]["vgpr"] <= 256 and ks[TRIM]["sgpr"] <= 102


@pytest.mark.parametrize("nin,nout,width,depth,G,first,last", SHAPES)
def test_liveness_against_hand_derived_values(nin, nout, width, depth, G, first, last):
    g, segs = trim(nin, nout, width, depth)
    assert g == G == sum(s * p for _, s, p, *_ in segs)
    assert segs == expected(width, depth, first, last)


def test_not_plain_has_no_liveness():
    from linna_amd import nn
    m = nn.MLP(33, 33, None, width=512, depth=2)
    assert nn.program_trim(m, 8)[0] == 0 and nn.program_trim(m, 8)[1].startswith("not plain")


def test_the_shapes_cover_what_they_are_there_for():
    """Every ``G mod 6``, a ``G < 6``, S1 at a run of one, two, three and five steps and in a two-pass segment, T3 and full
    within one run, a run that is both T3 and S1."""
    assert {G % 6 for *_, G, _, _ in SHAPES} == set(range(6))
    assert any(G < 6 for *_, G, _, _ in SHAPES)
    assert {f[1] for *_, f, _ in SHAPES if S1 in f[5]} >= {1, 2, 3, 5}
    assert sum(T3 in l[5] and F in l[5] for *_, l in SHAPES) >= 2
    assert any(l[0] == "WIDE" and T3 in l[5] for *_, l in SHAPES) and any(l[0] == "SPLIT" and T3 in l[5] for *_, l in SHAPES)
    assert any(f[2] == 2 and S1 in f[5] for *_, f, _ in SHAPES)                 # S1 in a two-pass segment
    assert any("T3+S1" in l[5] for *_, l in SHAPES)                             # a run that is both
