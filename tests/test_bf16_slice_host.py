"""CPU: the bf16 slice evaluation of the whole-network kernel -- its code objects and what the header says (no GPU needed)."""
import os
import re

import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "linna_hip.h")
KERNEL = "_ZN5linna28net_stream_slice_bf16_kernel"


def _slice_kernels():
    from linna_amd import _lib
    return [k for k in codeobj.kernels(_lib.LIB_PATH) if k["name"].startswith(KERNEL)]


def test_three_slice_kernels_without_scratch():
    """net_stream_slice_bf16_kernel<R, MOVE = 2, no GRAD, no STORE, ROWS, BF> for the 16-, 8- and 4-row engines, none spilling."""
    ks = _slice_kernels()
    tags = sorted(re.search(r"ILi6ELi(\d)ELb0ELi0ELi(\d+)ELb1EEEvNS_6NsArgsE$", k["name"]).groups() for k in ks)
    assert tags == sorted(("2", r) for r in ("16", "8", "4")), [k["name"] for k in ks]
    assert all(k["scratch"] == 0 for k in ks), [(k["name"], k["scratch"]) for k in ks]
    assert all(0 < k["vgpr"] <= 256 for k in ks), [(k["name"], k["vgpr"]) for k in ks]    # two waves per SIMD, as the family


def test_they_are_kernels_of_their_own():
    """Not further instantiations of net_stream_kernel (whose bf16 instantiations test_bf16_host.py pins to six), and
    net_stream_kernel itself has no bf16 MOVE == 2 instantiation."""
    from linna_amd import _lib
    ks = _slice_kernels()
    assert ks and not any("net_stream_kernel" in k["name"] for k in ks)
    every = [k["name"] for k in codeobj.kernels(_lib.LIB_PATH)]
    assert not [n for n in every if n.startswith("_ZN5linna17net_stream_kernel") and re.search(r"ILi6ELi2E.*Lb1EEEvNS_6NsArgsE$", n)]


def test_header_names_the_slice_entries_as_served_in_bf16():
    src = open(HEADER).read()
    assert re.search(r"#define LINNA_ABI_VERSION 12\b", src)
    m = re.search(r"/\* Emulator precision of a log-probability object\.(.*?)\*/\s*#define LINNA_PRECISION_FP32", src, re.S)
    assert m, "the comment block of linna_logprob_set_precision"
    text = " ".join(m.group(1).replace("\n *", " ").split())
    served, _, rest = text.partition("Served in bf16:")
    assert rest, "the comment lists the entries served in bf16"
    served_list, _, not_served = rest.partition("Not served:")
    assert "linna_slice_half_step" in served_list and "linna_logprob_eval_slice_points" in served_list
    assert not_served and "linna_logprob_grad" in not_served and "linna_slice_half_step" not in not_served
    from linna_amd import _lib
    assert _lib.ABI_VERSION == 12 and _lib.PRECISION == {"fp32": 0, "bf16": 1}
