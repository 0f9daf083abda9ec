"""CPU: every program the whole-network kernel's planner (csrc/net_program.hip) builds, pinned field by field.

tests/net_program_dump.hip, linked with the planner object alone, prints each case's NsProgram (every segment and pack
record), its sign-bit gates, net_stream_plan's answer and the AdamW descriptor table; tests/golden/net_programs.txt holds one
line per case -- a describe-style summary and a 64-bit hash of the full dump -- recorded from the planner as it stood before
it became a translation unit of its own.  A mismatch prints the case's full dump."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linna_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "net_programs.txt")
KINDS = ["SERVE", "SERVE_DENSE", "SERVE_BF16", "STORE", "TRAIN_FWD", "DX", "DX_INPUT", "GRAD_INPUT", "TRAIN_STEP", "TRAIN_STEP_BF16"]   # NsKind
SERVING = ("SERVE", "SERVE_DENSE", "SERVE_BF16")            # ns_kind_full_layers: these see the trailing input skip
TAKES_DENSE = ("SERVE_DENSE", "TRAIN_FWD", "TRAIN_STEP", "TRAIN_STEP_BF16")
DENSE = [("unfactored", 1, 2), ("tri0", 2, 0), ("tri1", 2, 1), ("tri2", 2, 2)]   # tag, NsDense::factored + 1, NsDense::tri


def networks():
    from linna_amd import nn
    nets = [("v2_%d_%d" % s, nn.ChtoModelv2(s[0], s[1], None)) for s in ((33, 33), (26, 457), (40, 1000), (4, 2))]
    nets += [("simple_6_4", nn.ChtoModelsimple(6, 4, None)), ("v2_linear_5_3", nn.ChtoModelv2_linear(5, 3, None)),
             ("mlp_33_33", nn.MLP(33, 33, None))]
    nets += [("mlp_10_%d" % nout, nn.MLP(10, nout, None, width=64, depth=1)) for nout in (700, 960, 961, 1024)]
    # refusals: a one-layer network, 257 inputs, a 1025-wide layer
    nets += [("one_layer", nn.MLP(10, 5, None, width=64, depth=0)), ("in_257", nn.MLP(257, 33, None, width=64, depth=1)),
             ("wide_1025", nn.MLP(10, 33, None, width=1025, depth=1))]
    return nets


def layer_lines(model):
    """(the dump program's layer lines of ``model``, the layer table they were taken from)."""
    from linna_amd import nn
    arr = nn.program_layers(model)
    return ["%d %d %d %d %d %r %d %d %d %d %d %d %d" % ((L.op, L.K, L.C, L.N, L.relu, L.alpha) + tuple(
        int(getattr(L, f) or 0) for f in ("W", "b", "W1", "b1", "W2", "b2", "Ws"))) for L in arr], arr


def case_line(case_id, kind, rows, in_size, dense, tri, nl):
    return "case %s %d %d %d %d %d %d" % (case_id, KINDS.index(kind), rows, in_size, dense, tri, nl)


def build_dump(directory):
    """Compile tests/net_program_dump.hip with the planner alone (host only) into ``directory``; the executable's path."""
    exe = os.path.join(str(directory), "dump")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "--offload-host-only", "-O1", "-std=c++17", "-I", CSRC, os.path.join(CSRC, "net_program.hip"),
                           os.path.join(ROOT, "tests", "net_program_dump.hip"), "-o", exe])
    return exe


def run_dump(exe, text):
    """(summary lines, {case id: full dump}) of the cases in ``text``."""
    out = subprocess.run([exe], input=text, stdout=subprocess.PIPE, universal_newlines=True, check=True).stdout
    summary, full, cur = [], {}, []
    for line in out.splitlines():
        if line.startswith("== "):
            summary.append(line[3:])
            full[line[3:].split(" | ")[0]] = "\n".join(cur)
            cur = []
        else:
            cur.append(line)
    return summary, full


def dump_records(full_text, what):
    """The records ``what`` ("seg", "pack", "nseg", ...) of one case's full dump, each as a {field: value} dict of strings."""
    recs = []
    for line in full_text.splitlines():
        f = line.split()
        if f and f[0] == what:
            recs.append(dict(zip(f[0::2], f[1::2])))
    return recs


def case_text():
    """The dump program's input: every network x NsKind x engine (x dense form), layer lists as nn.program_layers builds them."""
    from linna_amd import _lib
    out = []
    for name, model in networks():
        lines, arr = layer_lines(model)
        trained = [ln for ln, L in zip(lines, arr) if L.op != _lib.OP_INSKIP]
        for k, kind in enumerate(KINDS):
            layers = lines if kind in SERVING else trained
            for rows in (16, 4):
                for tag, dense, tri in (DENSE if kind in TAKES_DENSE else [("plain", 0, 2)]):
                    out.append("case %s/%s/r%d/%s %d %d %d %d %d %d" % (name, kind, rows, tag, k, rows, model.in_size, dense, tri, len(layers)))
                    out.extend(layers)
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    """(summary lines, {case id: full dump}) of the planner in the tree."""
    return run_dump(build_dump(tmp_path_factory.mktemp("net_program")), case_text())


def test_every_program_kind_matches_the_recorded_plan(dump):
    summary, full = dump
    want = open(GOLDEN).read().splitlines()
    assert len(summary) == 14 * 2 * (6 + 4 * 4) and len(set(full)) == len(summary)     # networks x engines x (plain kinds + dense kinds x forms)
    assert [w.split(" | ")[0] for w in want] == [s.split(" | ")[0] for s in summary]
    bad = [(w, s) for w, s in zip(want, summary) if w != s]
    for w, s in bad[:3]:
        print("expected %s\ngot      %s\n%s\n" % (w, s, full[s.split(" | ")[0]]))
    assert not bad, "%d of %d programs differ from tests/golden/net_programs.txt; the first: %s" % (len(bad), len(want), bad[0][1])


def test_the_recorded_plans_cover_every_kind_and_the_refusals():
    """The expectation itself: all ten kinds plan somewhere; the networks outside the kernel plan nowhere, and a one-layer
    network has no dX chain down to op 1, alone or in a merged training step."""
    want = dict(w.split(" | ")[:2] for w in open(GOLDEN).read().splitlines())
    planned = {i for i, summary in want.items() if summary.endswith(" plan 1")}
    assert {i.split("/")[1] for i in planned} == set(KINDS)
    assert not [i for i in planned if i.startswith(("in_257/", "wide_1025/", "one_layer/DX/", "one_layer/TRAIN_STEP"))]
    assert [i for i in planned if i.startswith("one_layer/")]
