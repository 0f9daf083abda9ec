"""CPU: the hand-placed step of the plain serving launch -- its process-wide switch, what the code-object metadata says about
the kernel, and that the shapes of tests/test_gpu_serve_plain_sched.py cover the step counts they are there for."""
import os
import re
import subprocess

import codeobj
from linna_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLACED = "_ZN5linna24net_stream_placed_kernelILi6EEEvNS_6NsArgsE"
PLAIN = "_ZN5linna23net_stream_plain_kernelILi6EEEvNS_6NsArgsE"


def test_switch_without_a_gpu():
    """``linna_serve_plain_sched``: process-wide, -1 queries, returns the previous value, refuses anything else with
    LINNA_ERR_INVALID and a text, and a refused call changes nothing."""
    lib = _lib.load()
    prev = lib.linna_serve_plain_sched(-1)
    assert prev in (0, 1)
    try:
        assert lib.linna_serve_plain_sched(0) == prev and lib.linna_serve_plain_sched(-1) == 0
        assert lib.linna_serve_plain_sched(1) == 0 and lib.linna_serve_plain_sched(-1) == 1
        rc = lib.linna_serve_plain_sched(2)
        assert rc < 0 and "linna_serve_plain_sched" in lib.linna_last_error().decode()
        assert lib.linna_serve_plain_sched(-1) == 1
        assert _lib.serve_plain_sched(0) == 1 and _lib.serve_plain_sched() == 0
    finally:
        lib.linna_serve_plain_sched(prev)


def test_the_default_is_the_hand_placed_step_in_a_fresh_process():
    code = "from linna_amd import _lib; print(_lib.load().linna_serve_plain_sched(-1))"
    out = subprocess.run([os.sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip() == "1"


def test_header_entry():
    src = open(os.path.join(ROOT, "include", "linna_hip.h")).read()
    assert re.search(r"int linna_serve_plain_sched\(int hand\);", src)


def test_the_kernel_fits_two_waves_per_simd():
    """One kernel with the hand-placed step beside the compiler-scheduled plain one: no scratch, at most 256 registers (two
    waves per SIMD, what its 512-thread workgroup needs)."""
    ks = {k["name"]: k for k in codeobj.kernels(_lib.LIB_PATH)}
    assert PLACED in ks and PLAIN in ks
    assert sum("net_stream_placed_kernel" in n for n in ks) == 1
    assert ks[PLACED]["scratch"] == 0 and ks[PLACED]["vgpr"] <= 256 and ks[PLACED]["sgpr"] <= 102


def test_the_gpu_shapes_cover_the_step_counts():
    """The table of the GPU test holds what its comments say (the planner decides G, not that file)."""
    import torch  # noqa: F401
    from test_gpu_serve_plain_sched import SHAPES, program
    seen, kinds = set(), {}
    for nin, nout, width, depth, G in SHAPES:
        g, segs = program(nin, nout, width, depth)
        assert g == G == sum(s * p for _, s, p in segs), (nin, nout, width, depth, g, segs)
        seen.add(g % 6)
        kinds[(nin, nout, width, depth)] = segs
    assert seen == set(range(6))
    assert sum(G < 6 for *_, G in SHAPES) >= 1
    assert ("WIDE", 64, 2) in kinds[(9, 33, 1024, 2)]
    assert [k for k, _, _ in kinds[(20, 100, 256, 3)]].count("SPLIT") == 3
    assert [k for k, _, _ in kinds[(12, 100, 128, 2)]].count("SPLIT") == 2
    assert sorted(s for _, s, _ in kinds[(5, 100, 40, 1)]) == [1, 3]
    assert sorted(s for _, s, _ in kinds[(12, 100, 128, 2)]) == [1, 2, 2]
