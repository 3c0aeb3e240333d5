"""The Burgers side of the collection phase without a GPU: header, binding and library agree on ``bg_step_span`` and
``bg_record``; both refuse bad arguments on the host, before any HIP call, with messages that start with their names; a
stack over a ``BurgersBatchedVecEnv`` is recognised and a scripted agent over it is given to the kernel tier, while a stack
over another class and the KS stepper's CPU twin keep their reasons."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _collect_scenario as sc  # noqa: E402
from test_capi_symbols import LIBDIR, declared_functions  # noqa: E402

import kspde  # noqa: E402
from pdecontrol.mbrl import collection_phase as cp  # noqa: E402
from pdecontrol.mbrl.recognition import Unrecognized  # noqa: E402
from pdegym.burgers import _hip  # noqa: E402


# ----------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ----------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_two_entries():
    declared = declared_functions("burgers_hip.h", "bg")
    rows = {name: (res, args) for name, res, args in _hip.SYMBOLS}
    assert sorted(rows) == declared and {"bg_step_span", "bg_record"} <= set(declared)
    res, args = rows["bg_step_span"]
    assert res is ctypes.c_int and len(args) == 15 and len(args) == len(rows["bg_step"][1]) + 1
    res, args = rows["bg_record"]
    assert res is ctypes.c_int and len(args) == 13 and args[-1] == ctypes.POINTER(_hip.Slabs)
    # the slabs are ks_record's, field for field: a DeviceExperienceReplay hands over the same seven pointers
    assert [n for n, _ in _hip.Slabs._fields_] == [n for n, _ in kspde.ks_record._fields_]
    assert ctypes.sizeof(_hip.Slabs) == ctypes.sizeof(kspde.ks_record) == 8 * 8
    assert [getattr(_hip.Slabs, n).offset for n, _ in _hip.Slabs._fields_] == \
        [getattr(kspde.ks_record, n).offset for n, _ in kspde.ks_record._fields_]
    assert os.path.exists(os.path.join(LIBDIR, "libburgers_hip.so")), "libburgers_hip.so not built (run __graft_entry__.build())"
    lib = _hip.load()
    assert all(hasattr(lib, name) for name in rows)


# ----------------------------------------------------------------------------------------------------------------------
# refusals, with pointers that are never dereferenced
# ----------------------------------------------------------------------------------------------------------------------
FAKE = ctypes.c_void_p(64)


def _texts(lib, entry, call, cases):
    texts = {}
    for what, change in cases.items():
        assert call(**change) < 0, what
        texts[what] = lib.bg_last_error().decode()
        assert texts[what].startswith(entry + ":"), (what, texts[what])
    return texts


def test_bg_step_span_refuses_before_any_device_call():
    lib = _hip.load()
    good = dict(u=FAKE, actions=FAKE, F=FAKE, n_act=4, E=3, N=64, T=2, dx=0.1, dt=1e-3, nu=0.01, sub=2, traj=FAKE)

    def call(**change):
        a = {**good, **change}
        return lib.bg_step_span(None, a["u"], a["actions"], a["F"], a["n_act"], a["E"], a["N"], a["T"], a["dx"], a["dt"], a["nu"],
                                a["sub"], a["traj"], None, None)

    cases = {"NULL u": dict(u=None), "NULL actions": dict(actions=None), "NULL F": dict(F=None), "NULL traj": dict(traj=None),
             "T = 0": dict(T=0), "T < 0": dict(T=-3), "no env": dict(E=0), "no actuator": dict(n_act=0),
             "17 actuators": dict(n_act=17), "negative sub-steps": dict(sub=-1), "N = 0": dict(N=0), "N = 96": dict(N=96),
             "N = 192": dict(N=192), "N = 2048": dict(N=2048), "dx = 0": dict(dx=0.0), "dt < 0": dict(dt=-1e-3),
             "nu < 0": dict(nu=-0.01), "nu NaN": dict(nu=float("nan"))}
    texts = _texts(lib, "bg_step_span", call, cases)
    assert "0 steps" in texts["T = 0"] and "17" in texts["17 actuators"] and "96" in texts["N = 96"]
    assert "supported sizes" in texts["N = 192"] and "supported sizes" in texts["N = 2048"]
    assert len({texts[k] for k in ("NULL u", "T = 0", "no env", "no actuator", "negative sub-steps", "N = 96", "N = 192",
                                   "dx = 0")}) == 8
    # what bg_step refuses as a grid size, the span refuses
    for N in (0, 96, 192, 2048):
        assert lib.bg_step(None, FAKE, None, None, 0, 3, N, 0.1, 1e-3, 0.01, 2, None, None, None) < 0, N
    with pytest.raises(_hip.BurgersHipError, match="bg_step_span: 0 steps"):
        _hip.check(call(T=0))


def test_bg_record_refuses_before_any_device_call():
    lib = _hip.load()
    E, T, A = 3, 2, 4
    dst = np.arange(T * E, dtype=np.int64)
    d = dst.ctypes.data_as(ctypes.c_void_p)
    slabs = lambda rows=16, **kw: _hip.Slabs(**{**{n: 64 for n, _ in _hip.Slabs._fields_[:7]}, "rows": rows, **kw})
    good = dict(traj=FAKE, actions=FAKE, E=E, N=64, A=A, ssq=FAKE, steps=FAKE, T=T, sub=2, dst=d, dst_host=d, out=slabs())

    def call(**change):
        a = {**good, **change}
        out = a["out"]
        return lib.bg_record(None, a["traj"], a["actions"], a["E"], a["N"], a["A"], a["ssq"], a["steps"], a["T"], a["sub"],
                             a["dst"], a["dst_host"], None if out is None else ctypes.byref(out))

    twice = dst.copy()
    twice[4] = twice[1]
    beyond = dst.copy()
    beyond[5] = 16
    cases = {"NULL traj": dict(traj=None), "NULL actions": dict(actions=None), "NULL ssq": dict(ssq=None),
             "NULL steps": dict(steps=None), "NULL dst": dict(dst=None), "NULL dst_host": dict(dst_host=None),
             "NULL out": dict(out=None), "NULL slab": dict(out=slabs(rewards=None)), "NULL flags": dict(out=slabs(truncated=None)),
             "T = 0": dict(T=0), "no env": dict(E=0), "N = 0": dict(N=0), "A = 0": dict(A=0), "A = 17": dict(A=17),
             "negative sub-steps": dict(sub=-1), "no rows": dict(out=slabs(rows=0)),
             "beyond": dict(dst_host=beyond.ctypes.data_as(ctypes.c_void_p)),
             "twice": dict(dst_host=twice.ctypes.data_as(ctypes.c_void_p))}
    texts = _texts(lib, "bg_record", call, cases)
    assert "beyond" in texts["beyond"] and "16" in texts["beyond"] and "twice" in texts["twice"]
    assert len({texts[k] for k in ("T = 0", "no env", "N = 0", "A = 0", "negative sub-steps", "no rows", "beyond", "twice")}) == 8


# ----------------------------------------------------------------------------------------------------------------------
# recognition
# ----------------------------------------------------------------------------------------------------------------------
def _bare_env(E=5, N=64):
    """A ``BurgersBatchedVecEnv`` without its device side (the constructor allocates on the GPU): the spaces and the host
    attributes the recognition and the tier choice read; nothing here can launch."""
    from pdegym._gym import gym
    from pdegym.burgers.burgers import BurgersBatchedVecEnv
    env = BurgersBatchedVecEnv.__new__(BurgersBatchedVecEnv)
    gym.vector.VectorEnv.__init__(env, E, gym.spaces.Box(-np.inf, np.inf, shape=(1, N), dtype=np.float32),
                                  gym.spaces.Box(-1.0, 1.0, shape=(1, 4), dtype=np.float32))
    env.N, env.cfg_steps, env.dt, env.max_episode_steps = N, 2, 1e-3, 4
    env.timestep = np.zeros(E, dtype=np.int64)
    env.stepper = types.SimpleNamespace(device=0, n_act=4)
    return env


@pytest.mark.parametrize("stride", [1, 4])
def test_a_burgers_stack_is_recognised(stride):
    from pdegym.burgers.burgers import BurgersBatchedVecEnv
    env = _bare_env()
    tf = sc.transforms(env, stride)
    for frozen in (False, True):
        geo = cp.recognize_real_stack(sc.make_stack(env, tf, frozen=frozen))
        assert geo.env is env and geo.kind == "burgers" and type(geo.env) is BurgersBatchedVecEnv
        assert geo.update == (0 if frozen else 1) and geo.scaling is tf.oscaling
        assert (geo.agent_obs.start, geo.agent_obs.stride, geo.agent_obs.width) == (stride // 2, stride, len(range(stride // 2, 64, stride)))
        assert geo.action.width == 4


def test_a_scripted_agent_over_a_burgers_stack_is_given_to_the_kernel_tier():
    """Every condition of the scripted tier is a host condition: it holds without a device, and nothing is drawn."""
    from pdecontrol.mbrl import utils
    from pdecontrol.mbrl.worker import Worker
    env = _bare_env()
    worker = Worker(sc.make_stack(env, sc.transforms(env), frozen=False))
    space = worker.stack.envs.action_space
    table = np.random.RandomState(3).uniform(-1, 1, (5, 16, 1, 4)).astype(np.float32)
    for agent in (utils.RandomAgent(space), utils.ActionRepeatAgent(table)):
        geo, fused, reason = cp._kernel_tier(worker, agent, lambda ts, ep: ts >= 10)
        assert reason is None and fused is None and geo.kind == "burgers" and geo.env is env


def test_the_ks_route_keeps_its_geometry_and_the_other_reasons_stay():
    from pdecontrol.mbrl import utils
    s = sc.build(E=5, N=64, device=-1)
    geo = cp.recognize_real_stack(s.stack)
    assert geo.kind == "ks" and geo.env is s.env
    agent = utils.RandomAgent(s.stack.envs.action_space)
    assert cp._kernel_tier(s.worker, agent, lambda ts, ep: ts >= 10)[2] == "the CPU twin of the KS stepper"
    for env in (s.env, _bare_env()):
        class Other(type(env)):
            pass

        stack = sc.make_stack(env, sc.transforms(env), frozen=False)
        kept = env.__class__
        stack.ostore.env.__class__ = Other
        try:
            with pytest.raises(Unrecognized, match="a Other in place of the KSBatchedVecEnv"):
                cp.recognize_real_stack(stack)
        finally:
            env.__class__ = kept
