"""CPU: the opt-in bf16 serving engine's C ABI, Python validation and code objects (no GPU needed)."""
import ctypes
import os
import re
import subprocess
import tempfile

import pytest

import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "linna_hip.h")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def test_header_declares_the_precision_entries_and_abi_12():
    src = open(HEADER).read()
    assert re.search(r"#define LINNA_ABI_VERSION 12\b", src)
    assert re.search(r"#define LINNA_PRECISION_FP32 0\b", src) and re.search(r"#define LINNA_PRECISION_BF16 1\b", src)
    assert re.search(r"int linna_logprob_set_precision\(linna_logprob_t\* lp, int precision\);", src)
    assert re.search(r"int linna_logprob_precision\(const linna_logprob_t\* lp, int\* out\);", src)
    from linna_amd import _lib
    assert _lib.ABI_VERSION == 12 and _lib.PRECISION == {"fp32": 0, "bf16": 1}


def test_null_handle_and_bad_code_are_invalid_without_a_gpu():
    from linna_amd import _lib
    lib = _lib.load()
    assert lib.linna_logprob_set_precision(None, 0) == _lib.ERR_INVALID
    assert lib.linna_logprob_set_precision(None, 1) == _lib.ERR_INVALID
    assert "null" in lib.linna_last_error().decode()
    out = ctypes.c_int(5)
    assert lib.linna_logprob_precision(None, ctypes.byref(out)) == _lib.ERR_INVALID and out.value == 5
    # an unknown code is refused before the handle is looked at: any non-null pointer will do here
    dummy = ctypes.create_string_buffer(64)
    for bad in (2, -1, 16):
        assert lib.linna_logprob_set_precision(ctypes.cast(dummy, ctypes.c_void_p), bad) == _lib.ERR_INVALID
        assert "unknown precision" in lib.linna_last_error().decode()


def test_log_prob_rejects_an_unknown_precision():
    from linna_amd import util
    with pytest.raises(ValueError, match="fp32.*bf16"):
        util.Log_prob(None, None, None, None, None, 1.0, precision="fp16")
    lp = util.Log_prob(None, None, None, None, None, 1.0, precision="bf16")
    assert lp.precision == "bf16"
    assert util.Log_prob(None, None, None, None, None, 1.0).precision == "fp32"


def test_bf16_instantiations_exist_without_scratch():
    from linna_amd import _lib
    ks = codeobj.kernels(_lib.LIB_PATH)
    bf = [k for k in ks if k["name"].startswith("_ZN5linna17net_stream_kernel") and k["name"].endswith("Lb1EEEvNS_6NsArgsE")]
    # MOVE 0 (evaluation) and 1 (fused stretch move) on the 16-, 8- and 4-row engines
    tags = sorted((re.search(r"ILi6ELi(\d)ELb0ELi0ELi(\d+)ELb1E", k["name"]).groups()) for k in bf)
    assert tags == sorted((m, r) for m in ("0", "1") for r in ("16", "8", "4")), tags
    assert all(k["scratch"] == 0 for k in bf), [(k["name"], k["scratch"]) for k in bf]


def _disassembly():
    from linna_amd import _lib
    out = []
    for triple, blob in codeobj.code_objects(_lib.LIB_PATH):
        if "gfx950" not in triple:
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob); f.flush()
            out.append(subprocess.run([OBJDUMP, "-d", f.name], capture_output=True, text=True).stdout)
    return "\n".join(out)


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump of the ROCm toolchain")
def test_bundle_holds_the_bf16_matrix_instructions():
    asm = _disassembly()
    assert "v_mfma_f32_16x16x32_bf16" in asm
    assert re.search(r"v_mfma_f32_4x4x4_16b_bf16 .*cbsz:4 abid:\d+", asm), "4x4x4 bf16 with the CBSZ / ABID broadcast"
    assert "v_cvt_pk_bf16_f32" in asm
