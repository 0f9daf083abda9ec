"""Which route every log-probability entry takes, as the caller sees it: a table of return codes, refusal texts and the two
route queries over a set of small handles that between them take every route of api.hip's lp_eval_route / lp_grad_route
(one launch, forward + likelihood, layered, the three one-launch gradients, the refusals), on every engine.  Not a test
module: tests/test_gpu_logprob_routes.py compares the table with tests/golden/logprob_routes.json, recorded with the library
before the routes were decided in one place; run under a kernel trace it shows the launches behind every route.

usage: python tests/logprob_routes.py [out.json]     (needs the GPU; LINNA_LIB_PATH selects another build of the library)"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), os.path.join(HERE, "golden"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import synth  # noqa: E402

B = 19                      # no multiple of 4: every engine has a ragged last workgroup
ENGINES = (0, 4, 8, 16)
T = 2.0


def problem(kind, nin, nout, seed, dense=False, ypositive=False, **kw):
    """A serving problem with every array drawn from numpy.random.RandomState (tests/golden/synth.py)."""
    data, cov, priors = synth.gaussian_problem(nin, nout, seed, dense=dense)
    X_mean, X_std, y_mean, y_std = synth.transform_constants(nin, nout, seed)
    if ypositive:
        data, y_std = np.abs(data) + 0.5, (0.1 * y_std).astype(np.float32)
    return dict(kind=kind, nin=nin, nout=nout, kw=kw, weights=synth.weights(kind, nin, nout, seed, **kw), priors=priors, data=data,
                invcov=np.linalg.inv(cov), sigma=np.sqrt(np.diag(cov)), X_mean=X_mean, X_std=X_std, y_mean=y_mean, y_std=y_std,
                ypositive=ypositive)


def create(prob, env=None):
    """The Log_prob of `prob` with its handle created under the switches `env` (linna_logprob_create reads them)."""
    import torch
    from linna_amd import nn, predictor_gpu, util
    model = getattr(nn, prob["kind"])(prob["nin"], prob["nout"], None, **prob["kw"])
    model.load_state_dict({k: torch.as_tensor(v) for k, v in prob["weights"].items()})
    t = lambda a: torch.as_tensor(np.asarray(a, np.float32))
    Xt = util.X_transform_class(t(prob["X_mean"]), t(prob["X_std"]), "cpu", None)
    Yt = util.Y_transform_class(t(prob["y_mean"]), t(prob["y_std"]), "cpu", ypositive=prob["ypositive"])
    pred = predictor_gpu.Predictor(prob["nin"], prob["nout"], model=model, X_transform=Xt, y_transform=Yt, device="cuda")
    lp = util.Log_prob(t(prob["data"]), t(prob["invcov"]), pred, util.Y_invtransform_data(prob["sigma"], "cpu"),
                       util.Transform(prob["priors"]), T, util.gaussianlogliklihood, nograd=True)
    env = env or {}
    assert not any(k in os.environ for k in env), env
    os.environ.update(env)
    try:
        lp._ensure()
    finally:
        for k in env:
            del os.environ[k]
    return lp


def walk(lp, seed):
    """{engine: {entry or query: [return code, refusal text or None] or the query's answer}} of one handle as it is set now."""
    import torch
    from linna_amd import _lib
    lib, P, I = _lib.load(), _lib.ptr, _lib.iptr
    p = lp._ensure()
    h, nin = p["handle"], p["nin"]
    ld = _lib.ld4(nin)
    rs = np.random.RandomState(seed)
    dev = lambda a, dt=np.float32: torch.as_tensor(np.ascontiguousarray(a, dt), device="cuda")
    z0 = np.zeros((2 * B, ld), np.float32)
    z0[:, :nin] = 0.4 * rs.standard_normal((2 * B, nin))
    mass, eps = dev(np.linspace(0.5, 2.0, nin)), dev(np.full(B, 0.01))
    gate, step = dev([1], np.int32), dev([0], np.int32)
    S, Cc = dev(np.arange(B), np.int32), dev(np.arange(B, 2 * B), np.int32)
    wgt = dev(0.1 * rs.standard_normal(B))
    ws = lp._workspace(2 * B, True)
    out = {}
    for rows in ENGINES:
        _lib.engine_rows(rows)
        Z, Q, Pm, DIR, coords = dev(z0[:B]), dev(z0[:B]), dev(z0[B:]), dev(0.1 * z0[B:]), dev(z0)
        lnp, G, logp = torch.zeros(B, device="cuda"), torch.zeros(B, ld, device="cuda"), torch.zeros(2 * B, device="cuda")
        nacc = torch.zeros(2 * B, dtype=torch.int32, device="cuda")
        f, st = C.c_float, _lib.stream()
        calls = [
            ("linna_logprob_eval", (h, P(Z), ld, B, P(ws), P(lnp), None, 0, st)),
            ("linna_logprob_eval_if", (h, P(Z), ld, B, P(ws), P(lnp), None, 0, I(gate), st)),
            ("linna_logprob_grad", (h, P(Z), ld, B, P(ws), P(lnp), P(G), ld, st)),
            ("linna_logprob_grad_leapfrog", (h, P(Q), ld, B, P(ws), P(lnp), P(G), ld, P(Pm), ld, P(mass), f(0.01), f(0.01), st)),
            ("linna_logprob_grad_leapfrog_eps", (h, P(Q), ld, B, P(ws), P(lnp), P(G), ld, P(Pm), ld, P(mass), P(eps), f(1.0), f(1.0), st)),
            ("linna_stretch_half_step", (h, P(coords), ld, nin, P(logp), I(S), B, P(coords), ld, I(Cc), B, C.c_uint64(7), I(step), 0, 0,
                                         f(2.0), I(nacc), st)),
            ("linna_logprob_eval_slice_points", (h, P(coords), ld, nin, I(S), B, P(DIR), ld, P(wgt), 1, P(lnp), None, st)),
        ]
        res = {}
        for name, args in calls:
            rc = getattr(lib, name)(*args)
            res[name] = [rc, lib.linna_last_error().decode() if rc != 0 else None]
        torch.cuda.synchronize()
        for query in ("linna_logprob_grad_launches", "linna_logprob_serve_plain"):
            ans = C.c_int(-1)
            _lib.call(query, h, B, C.byref(ans))
            res[query] = ans.value
        out[str(rows)] = res
    _lib.engine_rows(0)
    return out


def table():
    from linna_amd import _lib
    lib = _lib.load()
    mlp = dict(width=64, depth=2)
    a = problem("MLP", 5, 7, 41, **mlp)
    handles = [
        ("a_mlp_5_64_64_7", a, None),
        ("b_simple_6_4", problem("ChtoModelsimple", 6, 4, 42), None),
        ("c_mlp_5_64_70", problem("MLP", 5, 70, 43, width=64, depth=1), None),
        ("d_v2_26_457", problem("ChtoModelv2", 26, 457, 44), None),       # its gradient program does not fit the 16-row engine's LDS
        ("e_dense_fused", problem("MLP", 5, 7, 41, dense=True, **mlp), None),
        ("e_dense_not_fused", problem("MLP", 5, 7, 41, dense=True, **mlp), {"LINNA_DENSE_FUSED": "0"}),
        ("f_ypositive", problem("MLP", 5, 7, 41, ypositive=True, **mlp), None),
        ("g_disable_fused", a, {"LINNA_DISABLE_FUSED": "1"}),
        ("h_disable_fused_grad", a, {"LINNA_DISABLE_FUSED_GRAD": "1"}),
        ("j_mlp_70_inputs", problem("MLP", 70, 7, 45, **mlp), None),
        # WIDE segments only: the serving stream holds the backward segments (the MLP one-launch gradient; (a)'s 64-wide
        # layers are SPLIT segments, which that gradient does not cover: (a) takes the any-network one)
        ("k_mlp_5_512_7", problem("MLP", 5, 7, 46, width=512, depth=1), None),
    ]
    out = {}
    for i, (name, prob, env) in enumerate(handles):
        out[name] = walk(create(prob, env), 100 + i)
    # (i) the handle of (a) set to bf16: no gradient; with the bf16 gradient precision; back to fp32
    lp = create(a)
    h = lp._ensure()["handle"]
    _lib.check(lib.linna_logprob_set_precision(h, _lib.PRECISION["bf16"]))
    out["i_bf16"] = walk(lp, 110)
    _lib.check(lib.linna_logprob_set_grad_precision(h, _lib.PRECISION["bf16"]))
    out["i_bf16_grad_bf16"] = walk(lp, 110)
    _lib.check(lib.linna_logprob_set_precision(h, _lib.PRECISION["fp32"]))
    out["i_back_to_fp32"] = walk(lp, 110)
    return out


if __name__ == "__main__":
    text = json.dumps(table(), indent=1, sort_keys=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write(text + "\n")
    else:
        print(text)
