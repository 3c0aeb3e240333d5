"""The dissipation objective of the Burgers env on the host (no GPU): the objective header, its binding table and the
library; every refusal; ``bg_step_objective_host`` against the frozen C oracle and against the fp64 reference of the
dissipation sum; ``bg_reward_rows_host`` against its numpy spelling; the env, the stack recognition and the test phase on
the env without a device side (tests/_burgers_world_scenario.py::bare_env)."""
import ctypes
import itertools
import logging
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _burgers_cases as bc  # noqa: E402
import _burgers_objective as ob  # noqa: E402
import _burgers_world_scenario as bw  # noqa: E402
from _rollout_scenario import fma_chain  # noqa: E402
from test_capi_symbols import LIBDIR, ROOT, declared_functions  # noqa: E402

from oracle import burgers_oracle as bo  # noqa: E402
from pdegym.burgers import _hip  # noqa: E402

HEADER = os.path.join("burgers", "objective.h")
ENTRIES = ["bg_objective_last_error", "bg_reward_rows", "bg_reward_rows_host", "bg_step_objective", "bg_step_objective_host",
           "bg_step_span_objective"]
L2, DISS = 0, 1
PTR = ctypes.c_void_p(4096)          # a fake pointer: the refusals read nothing


@pytest.fixture(scope="module")
def lib():
    assert os.path.exists(os.path.join(LIBDIR, "libburgers_hip.so")), "libburgers_hip.so not built (run __graft_entry__.build())"
    return _hip.load()


def _strip(text):
    return re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)


def _c_arguments(text, name):
    """The C types of ``name``'s parameters in a comment-free header, as ctypes."""
    args = re.search(rf"\b{name}\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    out = []
    for arg in (a.strip() for a in args.split(",")):
        if arg == "void":
            continue
        if "*" in arg:
            out.append("pointer")
        else:
            out.append({"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double}[arg.split()[0]])
    return out


def _table_arguments(argtypes):
    return ["pointer" if (a is ctypes.c_void_p or hasattr(a, "contents")) else a for a in argtypes]


# ----------------------------------------------------------------------------------------------------------------------
# headers, binding tables and libraries
# ----------------------------------------------------------------------------------------------------------------------
def test_the_objective_header_its_table_and_the_library_agree(lib):
    declared = declared_functions(HEADER, "bg")
    assert declared == ENTRIES == sorted(name for name, _, _ in _hip.OBJECTIVE_SYMBOLS)
    for other in (declared_functions("burgers_hip.h", "bg"), declared_functions(os.path.join("burgers", "eval.h"), "bg"),
                  [n for n, _, _ in _hip.SYMBOLS], [n for n, _, _ in _hip.EVAL_SYMBOLS]):
        assert not set(declared) & set(other)
    raw = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "../burgers_hip.h"' in raw
    for top in os.listdir(os.path.join(ROOT, "include")):          # included by nothing at top level
        if top.endswith(".h"):
            assert "burgers/objective.h" not in open(os.path.join(ROOT, "include", top)).read(), top
    text = _strip(raw)
    assert int(re.search(r"#define BG_OBJECTIVE_L2CONTROL\s+(\d+)", text).group(1)) == _hip.OBJECTIVES["l2control"] == L2
    assert int(re.search(r"#define BG_OBJECTIVE_DISSIPATION\s+(\d+)", text).group(1)) == _hip.OBJECTIVES["dissipation"] == DISS
    for name, restype, argtypes in _hip.OBJECTIVE_SYMBOLS:         # argument for argument
        assert _c_arguments(text, name) == _table_arguments(argtypes), name
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # the step entries are bg_step's / bg_step_span's arguments plus the objective; the host twin drops the stream
    pinned = {name: args for name, _, args in _hip.SYMBOLS}
    table = {name: args for name, _, args in _hip.OBJECTIVE_SYMBOLS}
    assert table["bg_step_objective"] == pinned["bg_step"] + [ctypes.c_int]
    assert table["bg_step_span_objective"] == pinned["bg_step_span"] + [ctypes.c_int]
    assert table["bg_step_objective_host"] == pinned["bg_step"][1:] + [ctypes.c_int]
    assert table["bg_reward_rows_host"] == table["bg_reward_rows"][1:]


def test_the_rollout_header_its_table_and_the_library_agree():
    from pdecontrol.mbrl import rollout_hip as ro
    header = os.path.join("rollout", "settle_burgers_dissipation.h")
    raw = open(os.path.join(ROOT, "include", header)).read()
    assert '#include "settle_dissipation.h"' in raw
    text = _strip(raw)
    declared = declared_functions(header, "ro")
    assert declared == ["ro_settle_burgers_dissipation"] == sorted(name for name, _, _ in ro.BURGERS_DISSIPATION_SYMBOLS)
    assert not set(declared) & {name for name, _, _ in ro.SYMBOLS + ro.DISSIPATION_SYMBOLS}
    assert re.findall(r"typedef struct (\w+)", text) == ["ro_burgers_dissipation_args"]
    fields = re.search(r"typedef struct ro_burgers_dissipation_args \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [name for name, _ in ro.BurgersDissipationArgs._fields_] == ["d", "nu"]
    assert ro.BurgersDissipationArgs._fields_[0][1] is ro.DissipationArgs
    assert os.path.exists(ro.LIB_PATH), "librollout_hip.so not built (run __graft_entry__.build())"
    lib = ro.load()
    for name, restype, argtypes in ro.SYMBOLS + ro.DISSIPATION_SYMBOLS + ro.BURGERS_DISSIPATION_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    assert _c_arguments(text, "ro_settle_burgers_dissipation") == ["pointer"] * 4


# ----------------------------------------------------------------------------------------------------------------------
# refusals: by code and prefix, with fake pointers and no HIP call
# ----------------------------------------------------------------------------------------------------------------------
def test_every_stepper_refusal_is_made_on_the_host(lib):
    good = dict(u=PTR, actions=PTR, F=PTR, n_act=4, n_envs=3, N=128, T=2, dx=0.05, dt=1e-3, nu=0.01, n_substeps=5, out=PTR,
                objective=1)

    def step(name, **over):
        a = {**good, **over}
        stream = () if name.endswith("_host") else (None,)
        rc = getattr(lib, name)(*stream, a["u"], a["actions"], a["F"], a["n_act"], a["n_envs"], a["N"], a["dx"], a["dt"], a["nu"],
                                a["n_substeps"], None, None, None, a["objective"])
        return rc, lib.bg_objective_last_error().decode()

    def span(name, **over):
        a = {**good, **over}
        rc = lib.bg_step_span_objective(None, a["u"], a["actions"], a["F"], a["n_act"], a["n_envs"], a["N"], a["T"], a["dx"],
                                        a["dt"], a["nu"], a["n_substeps"], a["out"], None, None, a["objective"])
        return rc, lib.bg_objective_last_error().decode()

    shared = [(-1, dict(u=None)), (-1, dict(n_envs=0)), (-1, dict(n_act=0)), (-1, dict(n_act=17)), (-1, dict(n_substeps=-1)),
              (-1, dict(dx=0.0)), (-1, dict(dt=-1e-3)), (-1, dict(nu=-0.1)), (-1, dict(dx=float("nan"))),
              (-1, dict(objective=2)), (-1, dict(objective=-1)),
              (-4, dict(N=100)), (-4, dict(N=0)), (-4, dict(N=192)), (-4, dict(N=2048))]
    for name, call, extra in (("bg_step_objective", step, [(-1, dict(F=None))]),
                              ("bg_step_objective_host", step, [(-1, dict(F=None))]),
                              ("bg_step_span_objective", span, [(-1, dict(actions=None)), (-1, dict(F=None)), (-1, dict(out=None)),
                                                                (-1, dict(T=0)), (-1, dict(T=-3))])):
        for code, over in shared + extra:
            rc, message = call(name, **over)
            assert rc == code, (name, over, rc, message)
            assert message.startswith(name + ":"), (name, over, message)


def test_every_row_reward_and_settle_refusal_is_made_on_the_host(lib):
    good = dict(u=PTR, phi=PTR, actions=None, F=None, M=3, N=64, A=4, dx=0.1, nu=0.01, reward=PTR)

    def rows(name, **over):
        a = {**good, **over}
        stream = () if name.endswith("_host") else (None,)
        rc = getattr(lib, name)(*stream, a["u"], a["phi"], a["actions"], a["F"], a["M"], a["N"], a["A"], a["dx"], a["nu"], a["reward"])
        return rc, lib.bg_objective_last_error().decode()

    cases = [dict(u=None), dict(reward=None), dict(actions=PTR, F=PTR), dict(phi=None, actions=PTR), dict(phi=None, actions=PTR, F=PTR, A=0),
             dict(phi=None, actions=PTR, F=PTR, A=17), dict(M=0), dict(M=2 ** 30 + 1), dict(N=2), dict(dx=0.0), dict(dx=float("inf")),
             dict(dx=float("nan")), dict(nu=-1e-3), dict(nu=float("nan")), dict(nu=float("inf"))]
    for name in ("bg_reward_rows", "bg_reward_rows_host"):
        for over in cases:
            rc, message = rows(name, **over)
            assert rc == -1 and message.startswith(name + ":"), (name, over, rc, message)

    from pdecontrol.mbrl import rollout_hip as ro
    rlib, ptr = ro.load(), PTR.value
    geometry = dict(B=4, T=3, N=64, A=4, L=64, act_start=0, act_stride=1, obs_start=0, obs_stride=1, members=2)

    def settle_args(**missing):
        a = ro.SettleArgs()
        a.member[0] = a.member[1] = ptr
        for name in ("chosen", "state", "traj", "policy_obs", "steps0", "steps", "rewards", "reward_coef", "step"):
            setattr(a, name, None if name in missing else ptr)
        return a

    def args(actions=ptr, forcing=ptr, dx=0.1, nu=0.01):
        return ro.BurgersDissipationArgs(ro.DissipationArgs(actions, None, forcing, dx), nu)

    def call(g=None, a=None, d="default"):
        g = ro.Geometry(**{**geometry, **(g or {})})
        d = args() if d == "default" else d
        rc = rlib.ro_settle_burgers_dissipation(None, ctypes.byref(g), ctypes.byref(settle_args() if a is None else a),
                                                None if d is None else ctypes.byref(d))
        return rc, ro.last_error()

    for code, kwargs in [(-10, dict(d=None)), (-10, dict(d=args(actions=None))), (-10, dict(d=args(forcing=None))),
                         (-10, dict(a=settle_args(rewards=True))), (-10, dict(a=settle_args(chosen=True))),
                         (-11, dict(g=dict(L=32))), (-11, dict(g=dict(L=128))),
                         (-12, dict(d=args(dx=0.0))), (-12, dict(d=args(dx=-0.3))), (-12, dict(d=args(dx=float("nan")))),
                         (-12, dict(d=args(dx=float("inf")))),
                         (-13, dict(d=args(nu=-0.01))), (-13, dict(d=args(nu=float("nan")))), (-13, dict(d=args(nu=float("inf"))))]:
        rc, message = call(**kwargs)
        assert rc == code and message.startswith("ro_settle_burgers_dissipation"), (code, rc, message)
    rc, message = call(g=dict(N=8, L=8))                       # the geometry refusals keep their numbers and their prefix
    assert rc == -4 and message.startswith("rollout:")
    with pytest.raises(ro.RolloutHipError, match="ro_settle_burgers_dissipation"):
        ro.settle_burgers_dissipation(None, ro.Geometry(**geometry), settle_args(), args(nu=-1.0))


# ----------------------------------------------------------------------------------------------------------------------
# the stepper twin
# ----------------------------------------------------------------------------------------------------------------------
WIDTHS, SUBSTEPS, ENVS, ACTUATORS = (64, 128, 256, 1024), (0, 1, 3, 50), (1, 5), (0, 1, 4, 16)


@pytest.mark.parametrize("N", WIDTHS)
def test_objective_0_of_the_host_twin_has_the_bits_of_the_oracle(lib, N):
    """u against oracle/burgers_oracle.c's twin bit for bit (the anchor of the new host code to the frozen oracle); obs is
    u, the status is clear, and the l2control sum is the oracle's fp64 sum within the fp32 chains' bound."""
    dx, dt, nu = bc.params(N)
    for n, E, A in itertools.product(SUBSTEPS, ENVS, ACTUATORS):
        u0, act, F = ob.inputs(N, E, A)
        twin_u, twin_ssq = bo.twin_step(u0, act, F, dx, dt, nu, n)
        u, obs, ssq, status = ob.host_step(lib, u0, act, F, N, n, L2)
        bc.assert_bits(u, twin_u, f"u at N={N} n={n} E={E} A={A}")
        bc.assert_bits(obs, u, "obs")
        assert not status.any()
        np.testing.assert_allclose(ssq, twin_ssq, rtol=bc.ssq_rtol(N), atol=0)
    white = bc.case(N, 5, 4, 3)                                     # and on the white-noise case of tests/test_burgers.py
    bc.assert_bits(ob.host_step(lib, white["u0"], white["act"], white["F"], N, 3, L2)[0], white["twin_u"], "white noise")


@pytest.mark.parametrize("N", WIDTHS)
def test_objective_1_keeps_the_state_and_sums_within_the_derived_bound(lib, N):
    """Under dissipation u, obs and status are objective 0's bytes; the sum is within the derived bound of the fp64
    reference on the twin's own pre-update states, and on the forced cases neither term hides behind the other."""
    worst = 0.0
    for n, E, A in itertools.product(SUBSTEPS, ENVS, ACTUATORS):
        u0, act, F = ob.inputs(N, E, A)
        u, obs, _, status = ob.host_step(lib, u0, act, F, N, n, L2)
        u1, obs1, S, status1 = ob.host_step(lib, u0, act, F, N, n, DISS)
        bc.assert_bits(u1, u, f"u at N={N} n={n} E={E} A={A}")
        bc.assert_bits(obs1, obs, "obs")
        assert np.array_equal(status1, status)
        ref, bound, d, p, _ = ob.dissipation_reference(u0, act, F, N, n)
        if n == 0:
            assert np.array_equal(S, np.zeros(E))
            continue
        assert (d > 0).all()
        if A:
            assert (np.abs(p) >= 0.01 * d).all(), (N, n, E, A, p, d)
        err = np.abs(S - ref)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (N, n, E, A, err / bound)
    print(f"dissipation sum of the host twin at N={N}: worst error {worst:.3f} of the derived bound")


@pytest.mark.parametrize("N", WIDTHS)
def test_each_term_of_the_dissipation_sum_alone(lib, N):
    """actions NULL: S = nu sum G^2.  nu = 0: S = sum u phi (and the state is the inviscid one, the oracle's bits)."""
    for n, E in itertools.product((1, 3), ENVS):
        u0, act, F = ob.inputs(N, E, 4)
        _, _, S, _ = ob.host_step(lib, u0, None, None, N, n, DISS)
        ref, bound, d, p, _ = ob.dissipation_reference(u0, None, None, N, n)
        assert np.array_equal(p, np.zeros(E)) and (np.abs(S - d) <= bound).all() and (S > 0).all()
        u, _, S, _ = ob.host_step(lib, u0, act, F, N, n, DISS, nu=0.0)
        ref, bound, d, p, _ = ob.dissipation_reference(u0, act, F, N, n, nu=0.0)
        assert np.array_equal(d, np.zeros(E)) and (np.abs(S - p) <= bound).all() and (S != 0).all()
        dx, dt, _ = bc.params(N)
        bc.assert_bits(u, bo.twin_step(u0, act, F, dx, dt, np.float32(0.0), n)[0], "nu = 0")


# ----------------------------------------------------------------------------------------------------------------------
# the row reward
# ----------------------------------------------------------------------------------------------------------------------
def _rows_host(lib, u, phi, act, F, dx, nu):
    M, N = u.shape
    out = np.full(M, np.nan)
    rc = lib.bg_reward_rows_host(ob.ptr(u), ob.ptr(phi), ob.ptr(act), ob.ptr(F), M, N, 0 if act is None else act.shape[1], dx, nu,
                                 ob.ptr(out))
    assert rc == 0, lib.bg_objective_last_error()
    return out


@pytest.mark.parametrize("N", (5, 16, 64, 98, 512))
def test_reward_rows_host_has_the_bits_of_the_numpy_expression(lib, N):
    from pdegym.burgers.burgers import dissipation_rows
    rs = np.random.RandomState(N)
    M, dx, nu = 4, 2 * np.pi / N, 0.01
    u = ob.smooth(3 + N, M, N) + 0.05 * rs.uniform(-1, 1, (M, N)).astype(np.float32)
    phi = rs.uniform(-1, 1, (M, N)).astype(np.float32)
    for A in (1, 4, 16):
        act, F = rs.uniform(-1, 1, (M, A)).astype(np.float32), rs.uniform(-1, 1, (A, N)).astype(np.float32)
        got = _rows_host(lib, u, None, act, F, dx, nu)
        assert np.array_equal(got, ob.row_reward_numpy(u, fma_chain(act, F), dx, nu)), (N, A)
    got = _rows_host(lib, u, phi, None, None, dx, nu)
    assert np.array_equal(got, ob.row_reward_numpy(u, phi, dx, nu)) and np.isfinite(got).all() and (got != 0).all()
    assert np.array_equal(got, dissipation_rows(u, phi, dx, nu))                 # the env's host path: the same bits
    none = _rows_host(lib, u, None, None, None, dx, nu)                          # no forcing: minus the dissipation alone
    assert np.array_equal(none, ob.row_reward_numpy(u, np.zeros_like(u), dx, nu)) and (none < 0).all()


@pytest.mark.parametrize("N", (64, 128, 256, 512, 1024))
def test_a_one_sub_step_reward_is_the_row_reward_of_its_state(lib, N):
    """n = 1: S * c against the row reward of the same state, within (P + 9) 2^-24 (nu <ux^2> + <|u phi|>): the two differ
    in fp32 against fp64 coefficients (1 / (2 dx), two roundings in g entering twice) and in the P-term chains."""
    dx, _, nu = bc.params(N)
    P = N // 64
    for A in (0, 4):
        u0, act, F = ob.inputs(N, 5, A)
        phi = np.zeros_like(u0) if act is None else fma_chain(act, F)
        _, _, S, _ = ob.host_step(lib, u0, act, F, N, 1, DISS)
        step_reward = S * (-(1.0 / N) / 1)
        row = _rows_host(lib, u0, phi, None, None, float(dx), float(nu))
        d, pabs = ob.row_reward_terms(u0, phi, float(dx), float(nu))
        bound = (P + 9) * ob.U24 * (d + pabs)
        err = np.abs(step_reward - row)
        print(f"step against row reward at N={N} A={A}: worst error {float((err / bound).max()):.3f} of the bound")
        assert (err <= bound).all(), (N, A, err / bound)


# ----------------------------------------------------------------------------------------------------------------------
# the env, the recognition and the test phase without a device
# ----------------------------------------------------------------------------------------------------------------------
def _dissipation_env(**over):
    env = bw.bare_env(objective="dissipation", **over)
    env.reward_func = env._reward_transform()
    return env


def test_the_env_takes_two_objectives_by_name():
    from pdegym.burgers import BurgersBatchedVecEnv, BurgersEnv
    for bad in ("tracking", "", None, True, "Dissipation"):        # refused before anything touches the device
        with pytest.raises(ValueError, match="objective must be one of"):
            BurgersBatchedVecEnv(2, objective=bad)
        with pytest.raises(ValueError, match="objective must be one of"):
            BurgersEnv(objective=bad)
    assert BurgersEnv(objective="dissipation").objective == "dissipation" and BurgersEnv().objective == "l2control"
    assert bw.bare_env().scenario["objective"] == "l2control"
    env = _dissipation_env()
    assert env.scenario["objective"] == "dissipation" and env.scenario["nu"] == env.nu
    assert env.reward_scale(5) == -(1.0 / env.N) / 5


def test_reward_func_and_batched_reward_func_agree_row_by_row():
    env = _dissipation_env()
    B, N = 6, env.N
    rs = np.random.RandomState(2)
    obs = ob.smooth(1, B, N).reshape(B, 1, N)
    phi = rs.uniform(-1, 1, (B, 1, N)).astype(np.float32)
    act = rs.uniform(-1, 1, (B, 1, 4)).astype(np.float32)
    want = ob.row_reward_numpy(obs.reshape(B, N), phi.reshape(B, N), env.dx, env.nu).astype(np.float32)
    batched = env.batched_reward_func(obs, phi)
    assert batched.dtype == np.float32 and np.array_equal(batched, want)
    as_tensor = env.batched_reward_func(torch.from_numpy(obs), torch.from_numpy(phi))
    assert as_tensor.dtype == torch.float32 and np.array_equal(as_tensor.numpy(), want)
    for b in range(B):
        one = env.reward_func(torch.from_numpy(obs[b]), torch.from_numpy(phi[b]))
        assert isinstance(one, torch.Tensor) and one.dtype == torch.float32 and one.item() == want[b]
        assert env.reward_func(obs[b], phi[b]).item() == want[b]
    # actions go through the env's forcing (KuramotoSivashinskyEnv._forcing_field's rule)
    field = env.forcing(torch.from_numpy(act)).numpy()
    assert field.shape == (B, 1, N)
    assert np.array_equal(env.batched_reward_func(obs, act), env.batched_reward_func(obs, field))
    for call in (lambda: env.batched_reward_func(obs), lambda: env.batched_reward_func(obs, None),
                 lambda: env.reward_func(torch.from_numpy(obs[0])), lambda: env.reward_func(obs[0], None)):
        with pytest.raises(ValueError, match="needs the forcing"):
            call()
    # the l2control env keeps its expression and ignores phi
    plain = bw.bare_env()
    l2 = plain.batched_reward_func(obs, phi)
    assert np.array_equal(l2, plain.batched_reward_func(obs)) and not np.array_equal(l2, want)


def test_the_stack_is_recognised_under_dissipation_only_when_asked():
    from pdecontrol.mbrl import imagination_phase as ip
    from pdecontrol.mbrl.recognition import Unrecognized
    M = bw.repo_namespace()
    env = _dissipation_env()
    s = bw.build(M, env=env)
    assert s.world.batched_reward_func.__self__ is env
    geo = ip.recognize_stack(s.stack, objectives=("l2control", "dissipation"))
    assert (geo.objective, geo.owner, geo.nu, geo.dx) == ("dissipation", "burgers", env.nu, env.L / env.N)
    assert tuple(geo.forcing.shape) == (4, bw.N)
    with pytest.raises(Unrecognized, match="^the dissipation objective$"):
        ip.recognize_stack(s.stack)                                   # the default keeps the refusal
    with pytest.raises(Unrecognized, match="^the dissipation objective$"):
        ip.recognize_stack(s.stack, objectives=("l2control",))
    plain = ip.recognize_stack(bw.build(M).stack, objectives=("l2control", "dissipation"))
    assert (plain.objective, plain.owner) == ("l2control", "burgers")
    # any other name keeps its refusal, asked for or not
    other = bw.bare_env(scenario={**bw.bare_env().scenario, "objective": "tracking"})
    s.world.batched_reward_func = other.batched_reward_func
    with pytest.raises(Unrecognized, match="BurgersBatchedVecEnv whose scenario names the tracking objective"):
        ip.recognize_stack(s.stack, objectives=("l2control", "dissipation", "tracking"))


def test_a_forcing_narrower_than_the_state_is_refused_under_dissipation():
    from pdecontrol.mbrl import imagination_phase as ip
    from pdecontrol.mbrl.recognition import Unrecognized
    from pdegym._gym import gym
    M = bw.repo_namespace()
    s = bw.build(M, env=_dissipation_env())
    T, half = M.T, bw.N // 2
    narrow = T.GaussianForcing(s.env.x[:half], s.env.Xi, s.env.sigma, s.env.L / 2, half)
    s.world.single_action_space = gym.spaces.Box(-1.0, 1.0, shape=(1, half), dtype=np.float32)
    tf = s.transforms
    import _rollout_scenario as rsc
    stack = rsc.make_stack(M, s.world, [tf.agent_sensor],
                           [(tf.world_sensor, False), (T.BatchTransform(narrow), True), (tf.ascaling, True)])
    with pytest.raises(Unrecognized, match=f"{half} columns.*{bw.N} grid points"):
        ip.recognize_stack(stack, objectives=("l2control", "dissipation"))


def test_the_test_phase_takes_its_host_lines_under_dissipation(caplog):
    from pdecontrol.surrogates import ops
    M = bw.repo_namespace()
    env = _dissipation_env()
    module = bw.fno_module(M, env.cfg_steps * env.dt, 0, "cpu")
    module.env = env
    states = torch.zeros(2, 3, 1, env.N)
    ops._NOTIFIED.difference_update({reason for reason in ops._NOTIFIED if "dissipation objective" in str(reason)})
    with caplog.at_level(logging.INFO, logger="pdecontrol.surrogates"):
        assert module._test_kernel_plan(states, None) is None
        assert module._test_kernel_plan(states, None) is None
    said = [r.getMessage() for r in caplog.records if "test_step computes its metrics with torch on the host" in r.getMessage()]
    assert len(said) == 1 and "the Burgers env's dissipation objective" in said[0], said       # one notice, naming the objective
    caplog.clear()
    module.env = bw.bare_env()
    with caplog.at_level(logging.INFO, logger="pdecontrol.surrogates"):
        assert module._test_kernel_plan(states, None) is None                  # a host batch: another reason
    assert not any("objective" in r.getMessage() for r in caplog.records)
