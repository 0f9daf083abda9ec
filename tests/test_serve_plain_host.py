"""CPU: the lean ("plain") instantiation of the whole-network serving kernel -- which op lists its host-side predicate
accepts, the process-wide switch, and what the code-object metadata says about the instantiation itself."""
import os
import re
import subprocess
import tempfile

import pytest

import codeobj
from linna_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = "_ZN5linna23net_stream_plain_kernelILi6EEEvNS_6NsArgsE"
GENERIC = "_ZN5linna17net_stream_kernelILi6ELi0ELb0ELi0ELi16ELb0EEEvNS_6NsArgsE"      # R 6, MOVE 0, no GRAD, STORE 0, 16 rows, fp32


def test_switch_without_a_gpu():
    """``linna_serve_plain``: process-wide, on by default, -1 queries, returns the previous value, refuses anything else
    with LINNA_ERR_INVALID and a text, and a refused call changes nothing."""
    lib = _lib.load()
    prev = lib.linna_serve_plain(-1)
    assert prev in (0, 1)
    try:
        assert lib.linna_serve_plain(0) == prev and lib.linna_serve_plain(-1) == 0
        assert lib.linna_serve_plain(1) == 0 and lib.linna_serve_plain(-1) == 1
        rc = lib.linna_serve_plain(2)
        assert rc < 0 and "linna_serve_plain" in lib.linna_last_error().decode()
        assert lib.linna_serve_plain(-1) == 1
        assert _lib.serve_plain(0) == 1 and _lib.serve_plain() == 0
    finally:
        lib.linna_serve_plain(prev)


def test_the_default_is_on_in_a_fresh_process():
    code = "from linna_amd import _lib; print(_lib.load().linna_serve_plain(-1))"
    out = subprocess.run([os.sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip() == "1"


def test_header_entries():
    src = open(os.path.join(ROOT, "include", "linna_hip.h")).read()
    assert re.search(r"int linna_serve_plain\(int on\);", src)
    assert re.search(r"int linna_program_plain\(const linna_layer_t\* layers, int nlayers, int in_size, int rows, int dense_nout\);", src)
    assert re.search(r"int linna_logprob_serve_plain\(linna_logprob_t\* lp, int B, int\* out\);", src)


# (model, constructor arguments, plain on the 16-row engine)
OP_LISTS = [
    ("MLP", (33, 33), {}, True),                              # the bench's 33 -> 512 x 4 -> 33
    ("MLP", (33, 33), {"width": 512, "depth": 2}, True),
    ("MLP", (9, 33), {"width": 1024, "depth": 2}, True),      # two WIDE passes
    ("MLP", (20, 100), {"width": 256, "depth": 3}, True),     # SPLIT hidden segments, four column groups
    ("MLP", (12, 100), {"width": 128, "depth": 2}, True),     # SPLIT hidden segments, two column groups
    ("ChtoModelv2", (33, 33), {}, False),                     # residual blocks: SIDE segments
    ("ChtoModelv2", (26, 457), {}, False),
    ("ChtoModelv2_linear", (5, 3), {}, False),                # input skip
    ("ChtoModelsimple", (6, 4), {}, False),
]


@pytest.mark.parametrize("kind,shape,kw,plain", OP_LISTS)
def test_which_op_lists_are_plain(kind, shape, kw, plain):
    """The predicate against the planner's own text: plain means every forward segment is WIDE or SPLIT; and only the
    16-row engine, and never with a dense segment."""
    import torch  # noqa: F401
    from linna_amd import nn
    m = getattr(nn, kind)(shape[0], shape[1], None, **kw)
    assert nn.program_is_plain(m, 16) is plain
    assert not nn.program_is_plain(m, 8) and not nn.program_is_plain(m, 4)
    assert not nn.program_is_plain(m, 16, dense_nout=shape[1]) and not nn.program_is_plain(m, 16, dense_nout=-shape[1])
    n, text = nn.describe_program(m, 16)
    hdr = text.splitlines()[0]
    nfwd = int(hdr.split()[hdr.split().index("nseg_f") + 1])
    kinds = [ln.split()[0] for ln in text.splitlines()[1:1 + nfwd]]
    if plain:
        assert set(kinds) <= {"WIDE", "SPLIT"}, text
    if "SIDE" in kinds:
        assert not plain


def test_the_small_mlps():
    """5 -> 40 -> 3: on the 16-row engine the planner makes the 40 -> 3 last layer a one-step SIDE segment (it pays there as it
    does for ChtoModelv2's 33 -> 33), so this network is NOT plain and keeps the generic instantiation; 5 -> 40 -> 100, the
    same short-K first layer in front of a short-K WIDE last layer, is."""
    import torch  # noqa: F401
    from linna_amd import nn

    def kinds(m):
        n, text = nn.describe_program(m, 16)
        hdr = text.splitlines()[0].split()
        return [ln.split()[0] for ln in text.splitlines()[1:1 + int(hdr[hdr.index("nseg_f") + 1])]]
    small = nn.MLP(5, 3, None, width=40, depth=1)
    assert kinds(small) == ["WIDE", "SIDE"] and not nn.program_is_plain(small, 16)
    wider = nn.MLP(5, 100, None, width=40, depth=1)
    assert kinds(wider) == ["WIDE", "WIDE"] and nn.program_is_plain(wider, 16)


def test_describe_text_is_unchanged_by_the_switch():
    import torch  # noqa: F401
    from linna_amd import nn
    m = nn.MLP(33, 33, None)
    prev = _lib.serve_plain(0)
    try:
        off = nn.describe_program(m, 16)
        _lib.serve_plain(1)
        assert nn.describe_program(m, 16) == off
    finally:
        _lib.serve_plain(prev)


def _function_sizes(path):
    sizes = {}
    for _, blob in codeobj.code_objects(path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob); f.flush()
            txt = subprocess.run([codeobj.READELF, "--symbols", "--wide", f.name], capture_output=True, text=True).stdout
        for line in txt.splitlines():
            p = line.split()
            if len(p) >= 8 and p[3] == "FUNC":
                sizes[p[7]] = int(p[2], 0)
    return sizes


def test_the_plain_instantiation_is_lean():
    """One plain instantiation in the bundle: no scratch, fewer registers than the generic 16-row serving instantiation,
    and a shorter code -- a condition, not a measurement (about half of it when this was written)."""
    ks = {k["name"]: k for k in codeobj.kernels(_lib.LIB_PATH)}
    assert PLAIN in ks and GENERIC in ks, sorted(n for n in ks if "net_stream" in n)[:4]
    assert sum("net_stream_plain_kernel" in n for n in ks) == 1
    assert ks[PLAIN]["scratch"] == 0 and ks[GENERIC]["scratch"] == 0
    assert ks[PLAIN]["vgpr"] <= ks[GENERIC]["vgpr"] and ks[PLAIN]["sgpr"] <= ks[GENERIC]["sgpr"]
    sizes = _function_sizes(_lib.LIB_PATH)
    assert 0 < sizes[PLAIN] < sizes[GENERIC], (sizes[PLAIN], sizes[GENERIC])
