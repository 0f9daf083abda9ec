"""CPU: the bf16 one-launch gradient's C ABI, code objects, program planning and the emulation helper (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

import bf16_emul
import bf16_grad_emul
import cases
import codeobj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "linna_hip.h")
NEW = ("linna_logprob_set_grad_precision", "linna_logprob_grad_precision", "linna_program_describe_grad_bf16")


def test_exports_bindings_and_header():
    from linna_amd import _lib
    lib = _lib.load()
    src = open(HEADER).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name
    assert re.search(r"int linna_logprob_set_grad_precision\(linna_logprob_t\* lp, int precision\);", src)
    assert re.search(r"int linna_logprob_grad_precision\(const linna_logprob_t\* lp, int\* out\);", src)
    assert re.search(r"int linna_program_describe_grad_bf16\(const linna_layer_t\* layers, int nlayers, int in_size, int rows, char\* buf, size_t n\);", src)
    assert re.search(r"#define LINNA_ABI_VERSION 12\b", src) and _lib.ABI_VERSION == 12 and lib.linna_abi_version() == 12
    assert _lib.PRECISION == {"fp32": 0, "bf16": 1}
    # the first opt-in's contract is still written down: the gradient stays under "Not served:"
    assert re.search(r"Not served: linna_logprob_grad and linna_logprob_grad_leapfrog", src)
    # null handle / unknown code: refused without a GPU
    assert lib.linna_logprob_set_grad_precision(None, 1) == _lib.ERR_INVALID and "null" in lib.linna_last_error().decode()
    out = ctypes.c_int(5)
    assert lib.linna_logprob_grad_precision(None, ctypes.byref(out)) == _lib.ERR_INVALID and out.value == 5
    dummy = ctypes.create_string_buffer(64)
    assert lib.linna_logprob_set_grad_precision(ctypes.cast(dummy, ctypes.c_void_p), 2) == _lib.ERR_INVALID
    assert "unknown precision" in lib.linna_last_error().decode()


def test_code_objects_hold_the_three_engines_within_budget():
    from linna_amd import _lib
    ks = codeobj.kernels(_lib.LIB_PATH)
    mine = [k for k in ks if "net_stream_grad_bf16_kernel" in k["name"]]
    tags = sorted(re.search(r"ILi6ELi0ELb1ELi2ELi(\d+)ELb1E", k["name"]).group(1) for k in mine)
    assert tags == ["16", "4", "8"], [k["name"] for k in mine]
    for k in mine:
        assert k["scratch"] == 0 and 0 < k["vgpr"] <= 256, k
        assert "net_stream_kernel" not in k["name"], k["name"]
    # the six bf16 instantiations of net_stream_kernel are still exactly six
    bf = [k for k in ks if k["name"].startswith("_ZN5linna17net_stream_kernel") and k["name"].endswith("Lb1EEEvNS_6NsArgsE")]
    assert len(bf) == 6, [k["name"] for k in bf]


# the header lines of the programs as the planner builds them (nn.describe_grad_bf16_program): pinned
PINNED = {
    ("v2", 4): "ok G 65 Gstride 127 nseg_f 10 LD 1092 kpad0 96 packed_floats 1044800 grad 0",
    ("v2", 16): "ok G 65 Gstride 127 nseg_f 10 LD 1092 kpad0 96 packed_floats 1044800 grad 0",
    ("mlp", 4): "ok G 53 Gstride 105 nseg_f 5 LD 516 kpad0 96 packed_floats 862784 grad 0",
    ("mlp", 16): "ok G 53 Gstride 105 nseg_f 5 LD 516 kpad0 96 packed_floats 862784 grad 0",
}


def _models():
    from linna_amd import nn
    return {"v2": nn.ChtoModelv2(33, 33, None), "mlp": nn.MLP(33, 33, None, width=512, depth=4)}


@pytest.mark.parametrize("net", ["v2", "mlp"])
@pytest.mark.parametrize("rows", [4, 16])
def test_planning(net, rows):
    from linna_amd import nn
    model = _models()[net]
    n, txt = nn.describe_grad_bf16_program(model, rows)
    n32, txt32 = nn.describe_program(model, rows, -1)
    lines, lines32 = txt.strip().splitlines(), txt32.strip().splitlines()
    assert lines[0] == PINNED[(net, rows)], lines[0]
    field = lambda ln, k: int(ln.split()[ln.split().index(k) + 1])
    # a SIDE segment of the fp32 program is a SPLIT one re-shaped: the segment counts agree
    assert n == n32 and field(lines[0], "nseg_f") == field(lines32[0], "nseg_f")
    assert len(lines) == 1 + n + 1
    assert not any(ln.startswith("SIDE") for ln in lines), txt
    assert field(lines[0], "Gstride") <= field(lines32[0], "Gstride")          # a bf16 step covers twice the k
    assert lines[-1].startswith("lds ") and "sign-bit columns" in lines[-1] and lines[-1].endswith("one launch"), lines[-1]
    assert int(lines[-1].split()[1]) <= 160 * 1024
    # the first layer is [W | W] over 2 x 33 inputs (96 k: three steps); the last backward segment is W0^T, 33 columns, not doubled
    assert lines[1].split()[:3] == ["WIDE", "steps", "3"] and lines[n].endswith("N 33")
    # every segment takes 32-k steps: the 512 -> 512 layers of the MLP are 16 steps each, forward and transposed
    if net == "mlp":
        assert [ln.split()[2] for ln in lines[2:5]] == ["16"] * 3 and [ln.split()[2] for ln in lines[7:10]] == ["16"] * 3


def test_plan_level_refusals():
    from linna_amd import nn
    for what, model in (("input skip", nn.ChtoModelv2_linear(5, 3, None)), ("65 inputs", nn.MLP(65, 33, None, width=64, depth=1)),
                        ("65 outputs", nn.MLP(33, 65, None, width=64, depth=1)), ("1100 wide", nn.MLP(12, 20, None, width=1100, depth=2))):
        n, txt = nn.describe_grad_bf16_program(model, 16)
        assert n == 0 and txt.startswith("not eligible"), (what, txt)


def test_log_prob_argument_checks_without_a_gpu():
    from linna_amd import util
    with pytest.raises(ValueError, match="grad_precision"):
        util.Log_prob(None, None, None, None, None, 1.0, precision="fp32", grad_precision="bf16")
    with pytest.raises(ValueError, match="fp32.*bf16"):
        util.Log_prob(None, None, None, None, None, 1.0, precision="bf16", grad_precision="fp16")
    lp = util.Log_prob(None, None, None, None, None, 1.0, precision="bf16", grad_precision="bf16")
    assert lp.precision == "bf16" and lp.grad_precision == "bf16"
    assert util.Log_prob(None, None, None, None, None, 1.0, precision="bf16").grad_precision == "fp32"
    assert util.Log_prob(None, None, None, None, None, 1.0).grad_precision == "fp32"


@pytest.mark.parametrize("name", ["simple_6_4", "mlp_7_5_small"])
def test_the_emulation_helper_is_the_oracle_when_it_does_not_round(name):
    """tests/bf16_grad_emul.py with rounded=False is the float64 oracle's lnP and gradient; rounded, its lnP is
    bf16_emul.log_prob's (the forward the serving tests pin) and its gradient differs from the exact one."""
    from oracle import likelihood
    prob = cases.serving_problem(name)
    w = np.diagonal(np.asarray(prob["invcov"], np.float64)).copy()
    prob = dict(prob, invcov=np.diag(w))
    z = (0.5 * np.random.RandomState(4).standard_normal((64, prob["nin"]))).astype(np.float32)
    l0, g0 = bf16_grad_emul.log_prob_grad(z, prob, w, 2.0, rounded=False)
    lr, gr = likelihood.grad_log_prob(z, cases.oracle_emulator(prob), prob["priors"], prob["data"], prob["invcov"], 2.0, dtype=np.float64)
    np.testing.assert_allclose(l0, lr, rtol=1e-6)                      # (the helper's network input is fp32: 2^-24 relative)
    np.testing.assert_allclose(g0, gr, rtol=1e-5, atol=1e-6 * np.abs(gr).max())
    l1, g1 = bf16_grad_emul.log_prob_grad(z, prob, w, 2.0)
    np.testing.assert_allclose(l1, bf16_emul.log_prob(z, prob, w, 2.0), rtol=1e-12)
    assert np.abs(g1 - g0).max() > 1e-4 * np.abs(g0).max()
