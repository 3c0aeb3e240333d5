"""The whole-segment entries of libcollect_hip.so on the host (include/collect/span.h): header, second binding table and
exports held to each other, their refusals before any HIP call, the workspace rule against the header's statement, and
the tier ``collect`` chooses for the two scripted agents of pdecontrol/mbrl/utils.py over the stepper's CPU twin."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _collect_scenario as sc  # noqa: E402

from pdecontrol.mbrl import collect_hip as co  # noqa: E402
from pdecontrol.mbrl import collection_phase as cp  # noqa: E402
from pdecontrol.mbrl import utils  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "collect", "span.h")
LIB = os.path.join(ROOT, "model-based-pde-control_amd", "lib", "libcollect_hip.so")
SPAN = ["co_act_span", "co_observe_span", "co_span_workspace_floats"]


def _declared():
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", open(HEADER).read(), flags=re.S)
    return text, sorted(set(re.findall(r"\b(co_[a-z0-9_]+)\s*\(", text)))


# ----------------------------------------------------------------------------------------------------------------------
# header, binding, library
# ----------------------------------------------------------------------------------------------------------------------
def test_span_header_binding_and_library_agree():
    text, names = _declared()
    assert names == SPAN
    assert '#include "../collect_hip.h"' in text
    assert sorted(name for name, _, _ in co.SPAN_SYMBOLS) == SPAN
    assert not set(SPAN) & {name for name, _, _ in co.SYMBOLS}
    assert os.path.exists(LIB), "libcollect_hip.so not built (run __graft_entry__.build())"
    import torch  # noqa: F401  (its bundled HIP runtime must be the one the library binds to)
    handle = ctypes.CDLL(LIB)
    assert not [n for n in SPAN if not hasattr(handle, n)]
    lib = co.load()
    for name, restype, argtypes in co.SPAN_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    cap = int(re.search(r"#define\s+CO_SPAN_MAX_PARTS\s+(\d+)", text).group(1))
    assert cap == co.SPAN_MAX_PARTS == 1024


def test_span_refusals_happen_before_any_hip_call():
    """No GPU here: every refusal below returns before the first HIP call."""
    lib = co.load()
    good = dict(E=5, T=3, N=64, A=4, obs_start=0, obs_stride=1)
    g = co.Geometry(**good)
    fake = ctypes.c_void_p(64)                                         # never dereferenced on the host
    act = co.ActSpanArgs(fake, None, fake, fake, 0)
    obs = co.ObserveArgs(fake, fake, fake, -1.0, 1.0, 1, fake)
    # a geometry co_supported refuses: its code, from all three
    for code, change in ((-2, dict(E=0)), (-3, dict(T=0)), (-4, dict(N=8)), (-4, dict(N=1028)), (-5, dict(A=17)),
                         (-6, dict(obs_stride=0)), (-6, dict(obs_start=64))):
        bad = co.Geometry(**{**good, **change})
        assert lib.co_act_span(None, ctypes.byref(bad), ctypes.byref(act)) == code, change
        assert co.last_error().startswith("collect:")
        assert lib.co_observe_span(None, ctypes.byref(bad), ctypes.byref(obs)) == code, change
        assert lib.co_span_workspace_floats(ctypes.byref(bad)) == code, change
    assert lib.co_act_span(None, None, ctypes.byref(act)) == -1
    assert lib.co_observe_span(None, None, ctypes.byref(obs)) == -1
    assert lib.co_span_workspace_floats(None) == -1
    # NULL pointers, as co_act / co_observe refuse them
    assert lib.co_act_span(None, ctypes.byref(g), None) == -10
    assert lib.co_observe_span(None, ctypes.byref(g), None) == -10
    for hole in range(4):
        if hole == 1:
            continue                                                   # a NULL coef is the identity
        ptrs = [fake] * 4
        ptrs[hole] = None
        assert lib.co_act_span(None, ctypes.byref(g), ctypes.byref(co.ActSpanArgs(*ptrs, 0))) == -10, hole
        assert "co_act_span" in co.last_error()
    assert lib.co_observe_span(None, ctypes.byref(g), ctypes.byref(co.ObserveArgs(None, fake, fake, -1.0, 1.0, 1, fake))) == -10
    assert lib.co_observe_span(None, ctypes.byref(g), ctypes.byref(co.ObserveArgs(fake, None, fake, -1.0, 1.0, 1, fake))) == -10
    assert "co_observe_span" in co.last_error()
    # update = 1 without a workspace
    assert lib.co_observe_span(None, ctypes.byref(g), ctypes.byref(co.ObserveArgs(fake, fake, fake, -1.0, 1.0, 1, None))) == -12
    assert "workspace" in co.last_error()
    with pytest.raises(co.CollectHipError, match="workspace"):
        co.observe_span(None, g, co.ObserveArgs(fake, fake, fake, -1.0, 1.0, 1, None))
    with pytest.raises(co.CollectHipError, match="state width"):
        co.span_workspace_floats(co.Geometry(**{**good, "N": 8}))


def test_span_workspace_follows_the_headers_statement():
    text = open(HEADER).read()
    assert "co_span_workspace_floats(g) = 2 * min(ceil(T * E / 4), CO_SPAN_MAX_PARTS)" in text
    for T, E in ((1, 1), (1, 4), (1, 5), (3, 5), (3, 257), (5, 1025), (61, 4096), (1, 4096), (1, 4097), (20000, 10)):
        g = co.Geometry(E=E, T=T, N=64, A=4, obs_start=0, obs_stride=1)
        assert co.span_workspace_floats(g) == 2 * min(-(-(T * E) // 4), 1024), (T, E)
    assert co.span_workspace_floats(co.Geometry(E=4096, T=1, N=64, A=4, obs_start=0, obs_stride=1)) == 2048
    assert co.span_workspace_floats(co.Geometry(E=4096, T=61, N=64, A=4, obs_start=0, obs_stride=1)) == 2048


# ----------------------------------------------------------------------------------------------------------------------
# utils and the tier choice over the CPU twin
# ----------------------------------------------------------------------------------------------------------------------
def test_the_scripted_agents_keep_the_reference_semantics():
    import torch

    class Space:
        def __init__(self):
            self.n = 0

        def sample(self):
            self.n += 1
            return self.n

    space = Space()
    agent = utils.RandomAgent(space)
    assert agent.action_space is space
    assert [agent.select_action(None, deterministic=True), agent.select_action(), agent.select_action(1, 2, x=3)] == [1, 2, 3]
    table = np.arange(2 * 3 * 1 * 4, dtype=np.float32).reshape(2, 3, 1, 4)
    repeat = utils.ActionRepeatAgent(table)
    assert repeat.nstep == 0 and repeat.actions is table
    np.testing.assert_array_equal(repeat.select_action(None, deterministic=False), table[:, 0])
    np.testing.assert_array_equal(repeat.select_action(), table[:, 1])
    assert repeat.nstep == 2
    with pytest.raises(AssertionError):
        utils.ActionRepeatAgent(table[0])
    assert isinstance(utils.totorch([1.0, 2.0]), torch.Tensor) and utils.totorch([1.0]).dtype == torch.float32
    t = torch.ones(2)
    assert utils.totorch(t) is t and isinstance(utils.tonumpy(t), np.ndarray) and utils.tonumpy(table) is table


class _Drawn(Exception):
    pass


def _no_draw(agent):
    def select_action(*args, **kwargs):
        raise _Drawn("the tier choice drew from the agent")
    agent.select_action = select_action
    return agent


def test_tier_choice_for_scripted_agents_over_the_cpu_twin():
    s = sc.build(E=3)
    E = 3
    stop = lambda ts, ep: ts >= 2 * E
    space = s.stack.envs.action_space
    assert tuple(space.shape) == (E, 1, 4) and space.dtype == np.float32
    table = np.random.RandomState(3).uniform(-1, 1, (E, 16, 1, 4)).astype(np.float32)

    # the utils agents: everything holds but the GPU
    for agent in (utils.RandomAgent(space), utils.ActionRepeatAgent(table)):
        geo, fused, reason = cp._kernel_tier(s.worker, _no_draw(agent), stop)
        assert geo is None and fused is None and reason == "the CPU twin of the KS stepper", reason

    # a subclass and a namesake are no scripted agents
    class Sub(utils.RandomAgent):
        pass

    class RandomAgent:
        def __init__(self, action_space):
            self.action_space = action_space

    for agent in (Sub(space), RandomAgent(space)):
        geo, fused, reason = cp._kernel_tier(s.worker, agent, stop)
        assert geo is None and fused is None and "not a SAC" in reason and type(agent).__name__ in reason

    # a space of the wrong shape, a table that is too short, of the wrong width or dtype: reasons of their own
    single = s.env.single_action_space
    for agent, word in ((utils.RandomAgent(single), "action space of shape"),
                        (utils.ActionRepeatAgent(table[:, :1]), "holds 1 steps"),
                        (utils.ActionRepeatAgent(table[:2]), "table is not"),
                        (utils.ActionRepeatAgent(table.astype(np.float64)), "table is not")):
        geo, fused, reason = cp._kernel_tier(s.worker, _no_draw(agent), stop)
        assert geo is None and fused is None and word in reason and "CPU twin" not in reason, reason
    # the table's length counts from nstep: 15 + 2 steps do not fit 16 columns, 14 + 2 do
    late = utils.ActionRepeatAgent(table)
    late.nstep = 15
    assert "holds 16 steps where the phase ends at step 17" in cp._kernel_tier(s.worker, _no_draw(late), stop)[2]
    late.nstep = 14
    assert cp._kernel_tier(s.worker, _no_draw(late), stop)[2] == "the CPU twin of the KS stepper"


def test_collect_runs_the_loop_for_scripted_agents_on_the_cpu_twin():
    """The loop's result, with the reason, from the same seeds."""
    E = 3
    stop = lambda ts, ep: ts >= 2 * E
    out = []
    for route in ("loop", "collect"):
        s = sc.build(E=E)
        sc.seed()
        sc.prime(s.worker, 11)
        space = s.stack.envs.action_space
        space.seed(7)
        agent = utils.RandomAgent(space)
        replay = s.worker.rollout(agent, stop) if route == "loop" else cp.collect(s.worker, agent, stop)
        out.append((replay, sc.state_record(s.worker)))
    sc.assert_same_replay(out[0][0], out[1][0])
    sc.assert_same_state(out[0][1], out[1][1])
    got = out[1][0]
    assert got.tier == "loop" and got.tier_reason == "the CPU twin of the KS stepper" and got.host_steps == 2
