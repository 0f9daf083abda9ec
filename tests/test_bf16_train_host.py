"""CPU: the opt-in bf16 training step's interface (linna_net_set_train_precision) -- declared, bound, checked without a
GPU, refused by the Python entries for an unknown precision before any GPU work, and its kernel in the bundle."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
ENTRIES = ("linna_net_set_train_precision", "linna_net_train_precision")


def test_header_declares_and_lib_binds_the_entries():
    from linna_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "linna_hip.h")).read()
    assert "int linna_net_set_train_precision(linna_net_t* net, int precision);" in hdr
    assert "int linna_net_train_precision(const linna_net_t* net, int* out);" in hdr
    lib = _lib.load()
    for name in ENTRIES:
        assert callable(getattr(lib, name)), name
    assert _lib.PRECISION == {"fp32": 0, "bf16": 1}


def test_null_handle_and_unknown_code_are_invalid_without_a_gpu():
    from linna_amd import _lib
    lib = _lib.load()
    assert lib.linna_net_set_train_precision(None, 1) == _lib.ERR_INVALID
    assert "null" in lib.linna_last_error().decode()
    out = C.c_int(-1)
    assert lib.linna_net_train_precision(None, C.byref(out)) == _lib.ERR_INVALID
    assert "null" in lib.linna_last_error().decode()
    # an unknown code is checked before the handle is looked at: a non-null dummy never gets dereferenced
    dummy = C.c_void_p(8)
    assert lib.linna_net_set_train_precision(dummy, 7) == _lib.ERR_INVALID
    msg = lib.linna_last_error().decode()
    assert "unknown precision 7" in msg and "FP32" in msg and "BF16" in msg


def test_unknown_precision_raises_before_any_gpu_work():
    from linna_amd import predictor_gpu, util, main
    pred = predictor_gpu.Predictor.__new__(predictor_gpu.Predictor)
    with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
        pred.train(None, 1, None, precision="fp16")
    with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
        util.train_NN(None, None, None, [1.0], "/nonexistent/", [], None, precision="tf32")
    with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
        main.ml_sampler_core(None, None, None, None, None, None, None, "/nonexistent/", None, None, None, None, None, None, 4,
                             "cuda", None, False, None, train_precision="half")


def _bf16_train_kernel():
    from linna_amd import _lib
    ks = [k for k in codeobj.kernels(_lib.LIB_PATH) if k["name"].startswith("_ZN5linna28net_stream_train_bf16_kernel")]
    return ks


def test_bf16_training_kernel_is_in_the_bundle_without_scratch():
    ks = _bf16_train_kernel()
    assert len(ks) == 1, [k["name"] for k in ks]
    assert ks[0]["scratch"] == 0, ks[0]
    # the serving instantiations stay exactly the six net_stream_kernel<..., BF = true> ones (tests/test_bf16_host.py)
    assert not ks[0]["name"].startswith("_ZN5linna17net_stream_kernel")


def test_bf16_training_kernel_uses_bf16_and_fp32_matrix_cores():
    """bf16 runs on v_mfma_f32_4x4x4_16b_bf16, the loss run on v_mfma_f32_4x4x1_16b_f32 -- in the one kernel."""
    from linna_amd import _lib
    name = _bf16_train_kernel()[0]["name"]
    text = None
    for triple, blob in codeobj.code_objects(_lib.LIB_PATH):
        if "gfx950" not in triple:
            continue
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob); f.flush()
            dis = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True).stdout
        m = re.search(r"<%s>:\n(.*?)(?:\n\n|\Z)" % re.escape(name), dis, re.S)
        if m:
            text = m.group(1)
            break
    assert text is not None
    assert "v_mfma_f32_4x4x4_16b_bf16" in text
    assert "v_mfma_f32_4x4x1_16b_f32" in text
