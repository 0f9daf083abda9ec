"""GPU: every log-probability entry takes the route it took before the routes were decided in one place (api.hip:
lp_eval_route, lp_grad_route) -- the return codes, the refusal texts character for character and the answers of
linna_logprob_grad_launches / linna_logprob_serve_plain over the handles of tests/logprob_routes.py on every engine, against
the table recorded with the parent's library (tests/golden/logprob_routes.json: recorded results only)."""
import json
import os

import pytest

import logprob_routes

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logprob_routes.json")


def test_every_entry_takes_the_recorded_route():
    want = json.load(open(GOLDEN))
    got = json.loads(json.dumps(logprob_routes.table()))
    assert sorted(got) == sorted(want)
    for handle in want:
        assert sorted(got[handle]) == sorted(want[handle]) == sorted(str(r) for r in logprob_routes.ENGINES), handle
        for rows in want[handle]:
            assert got[handle][rows] == want[handle][rows], (handle, rows)
    # the table walks what it says it walks: every route's mark shows somewhere in it
    at = lambda h, r, k: want[h][r][k]
    assert at("c_mlp_5_64_70", "16", "linna_logprob_serve_plain") == 1 and at("c_mlp_5_64_70", "4", "linna_logprob_serve_plain") == 0
    assert at("a_mlp_5_64_64_7", "0", "linna_logprob_grad_launches") == 1 and at("k_mlp_5_512_7", "0", "linna_logprob_grad_launches") == 1
    assert at("b_simple_6_4", "0", "linna_logprob_grad_launches") == 1 and at("c_mlp_5_64_70", "0", "linna_logprob_grad_launches") == 1
    assert at("d_v2_26_457", "16", "linna_logprob_grad_launches") == 0 and at("d_v2_26_457", "4", "linna_logprob_grad_launches") == 1
    assert at("f_ypositive", "0", "linna_logprob_grad")[0] != 0 and at("f_ypositive", "0", "linna_stretch_half_step")[0] == 0
    assert at("g_disable_fused", "0", "linna_stretch_half_step")[0] != 0 and at("g_disable_fused", "0", "linna_logprob_eval")[0] == 0
    assert at("h_disable_fused_grad", "0", "linna_logprob_grad_launches") == 0
    assert at("i_bf16", "0", "linna_logprob_grad")[0] != 0 and at("i_bf16_grad_bf16", "0", "linna_logprob_grad_launches") == 1
    assert at("j_mlp_70_inputs", "0", "linna_stretch_half_step")[0] != 0 and at("j_mlp_70_inputs", "0", "linna_logprob_eval")[0] == 0
