"""The dissipation objective of the imagined-rollout phase on the host: stack recognition, the numpy twin of
``ro_settle_dissipation``'s reward (tests/_rollout_dissipation.py) against the loop tier on the CPU, and the host
refusals of the entry point (no device needed)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _rollout_scenario as sc  # noqa: E402
from _rollout_dissipation import dissipation_terms, dissipation_twin  # noqa: E402

DEVICE_REWARD = {"batched_reward_func": lambda env: env.batched_reward_func}
BOTH = ("l2control", "dissipation")
SIZES = {"n64": {}, "n256": dict(L=88.0, N=256)}


@pytest.fixture(scope="module")
def M():
    return sc.repo_namespace()


def _build(M, tag, **kwargs):
    return sc.build(M, env_kwargs=dict(objective="", **SIZES[tag]), world_kwargs=DEVICE_REWARD, **kwargs)


# ----------------------------------------------------------------------------------------------------------------------
# recognition
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(SIZES))
def test_the_dissipation_stack_is_recognised_when_asked_for(M, tag):
    from pdecontrol.mbrl import imagination_phase as ip
    from pdecontrol.mbrl.recognition import Unrecognized
    s = _build(M, tag)
    geo = ip.recognize_stack(s.stack, objectives=BOTH)
    assert geo.objective == "dissipation" and geo.dx == s.env.L / s.env.N
    assert geo.world is s.world and tuple(geo.forcing.shape) == (4, s.env.N)
    with pytest.raises(Unrecognized, match="the dissipation objective"):
        ip.recognize_stack(s.stack)                                   # the default keeps the refusal
    with pytest.raises(Unrecognized, match="the dissipation objective"):
        ip.recognize_stack(s.stack, objectives=("l2control",))
    plain = sc.build(M, env_kwargs=dict(SIZES[tag]), world_kwargs=DEVICE_REWARD)
    for objectives in (("l2control",), BOTH):
        geo = ip.recognize_stack(plain.stack, objectives=objectives)
        assert geo.objective == "l2control" and geo.dx == plain.env.L / plain.env.N
    with pytest.raises(Unrecognized, match="the l2control objective"):
        ip.recognize_stack(plain.stack, objectives=("dissipation",))


def test_a_forcing_narrower_than_the_state_is_refused_under_dissipation(M):
    """The reward reads phi at every grid point: a world that takes 32 forcing columns for 64 grid points is recognised
    under l2control and refused, with both widths, under dissipation."""
    from pdecontrol.mbrl import imagination_phase as ip
    from pdecontrol.mbrl.recognition import Unrecognized
    from pdegym._gym import gym
    T = M.T
    for objective, refused in (("dissipation", False), ("", True)):
        s = sc.build(M, env_kwargs=dict(objective=objective), world_kwargs=DEVICE_REWARD)
        N, half = s.env.N, s.env.N // 2
        narrow = T.GaussianForcing(s.env.x[:half], s.env.Xi, s.env.sigma, s.env.L / 2, half)
        assert tuple(narrow.forcing.shape) == (4, half)
        s.world.single_action_space = gym.spaces.Box(-1.0, 1.0, shape=(1, half), dtype=np.float32)
        tf = s.transforms
        stack = sc.make_stack(M, s.world, [tf.agent_sensor],
                              [(tf.world_sensor, False), (T.BatchTransform(narrow), True), (tf.ascaling, True)])
        if refused:
            with pytest.raises(Unrecognized, match=f"{half} columns.*{N} grid points"):
                ip.recognize_stack(stack, objectives=BOTH)
        else:
            assert tuple(ip.recognize_stack(stack, objectives=BOTH).forcing.shape) == (4, half)


# ----------------------------------------------------------------------------------------------------------------------
# the twin against the loop tier
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(SIZES))
def test_twin_equals_the_loop_tier_on_the_cpu(M, tag):
    """Every reward of ``Worker.rollout`` under dissipation, both passes, within
        2^-23 |r| + 2 (A + 1) 2^-24 mean_i(|u_i| sum_k |a_k| F_ki)
    of the twin evaluated on the replay's own next observations and raw actions: two fp32 roundings of the result, and
    any order of an A-term fp32 product sum on either side (the loop forces the action it recovers from the world's
    action row through the host's matmul; the twin forces the scaled raw action by the fma chain)."""
    from pdecontrol.mbrl import imagination_phase as ip
    worst = 0.0
    for limit in (False, True):
        s = _build(M, tag, limit=limit)
        geo = ip.recognize_stack(s.stack, objectives=BOTH)
        A, N = (int(v) for v in geo.forcing.shape)
        s.world.setup(s.starting)
        sc.seed()
        replay = M.Worker(s.stack).rollout(s.agent, sc.stop())
        assert replay.ntimesteps == (2 if limit else 6) * sc.NUM_ENVS
        rows, actions, rewards = [], [], []
        for key in replay.episodes:
            rows += [np.asarray(v).reshape(N) for v in replay.nxtobs[key]]
            actions += [np.asarray(v).reshape(A) for v in replay.actions[key]]
            rewards += [np.asarray(v) for v in replay.rewards[key]]
        rewards = np.asarray(rewards)
        assert rewards.dtype == np.float32 and np.isfinite(rewards).all() and (rewards != 0).all()
        r64, scale = dissipation_terms(np.stack(rows), np.stack(actions), geo, s.env)
        twin = dissipation_twin(np.stack(rows), np.stack(actions), geo, s.env)
        assert twin.dtype == np.float32 and np.array_equal(twin, r64.astype(np.float32))
        err = np.abs(rewards.astype(np.float64) - twin.astype(np.float64))
        bound = 2.0 ** -23 * np.abs(r64) + 2 * (A + 1) * 2.0 ** -24 * scale
        worst = max(worst, float((err / bound).max()))
        print(f"twin against the CPU loop, {tag}, limit={limit}: {int((err == 0).sum())} of {err.size} rewards bit-equal, "
              f"worst error {float((err / bound).max()):.3f} of the bound")
        assert (err <= bound).all()
    assert worst <= 1.0


# ----------------------------------------------------------------------------------------------------------------------
# header, binding table and library of the entry point
# ----------------------------------------------------------------------------------------------------------------------
def test_the_dissipation_header_its_table_and_the_library_agree():
    """include/rollout/settle_dissipation.h declares exactly the names of ``DISSIPATION_SYMBOLS``, none of them is also in
    the l2control header's table, ``load()`` types both tables, and the built library exports every name (what
    tests/test_capi_symbols.py checks for the headers directly under include/)."""
    import re
    from pdecontrol.mbrl import rollout_hip as ro
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rollout", "settle_dissipation.h")).read()
    assert '#include "../rollout_hip.h"' in text
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(ro_[a-z0-9_]+)\s*\(", text)))
    assert declared == ["ro_settle_dissipation"] == sorted(name for name, _, _ in ro.DISSIPATION_SYMBOLS)
    assert not set(declared) & {name for name, _, _ in ro.SYMBOLS}
    assert sorted(re.findall(r"typedef struct (\w+)", text)) == ["ro_dissipation_args"]
    fields = re.search(r"typedef struct ro_dissipation_args \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"(\w+);", fields) == [name for name, _ in ro.DissipationArgs._fields_]
    if not os.path.exists(ro.LIB_PATH):
        pytest.skip("librollout_hip.so not built (run __graft_entry__.build())")
    lib = ro.load()
    for name, restype, argtypes in ro.SYMBOLS + ro.DISSIPATION_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ----------------------------------------------------------------------------------------------------------------------
# host refusals of ro_settle_dissipation
# ----------------------------------------------------------------------------------------------------------------------
def test_ro_settle_dissipation_refuses_on_the_host():
    """-10, -11 and -12 are decided before any HIP call: no device is touched (the pointers are never read)."""
    from pdecontrol.mbrl import rollout_hip as ro
    if not os.path.exists(ro.LIB_PATH):
        pytest.skip("librollout_hip.so not built (run __graft_entry__.build())")
    lib = ro.load()
    ptr = ctypes.c_void_p(4096).value
    good = dict(B=4, T=3, N=64, A=4, L=64, act_start=0, act_stride=1, obs_start=0, obs_stride=1, members=2)

    def settle_args(**missing):
        a = ro.SettleArgs()
        a.member[0] = a.member[1] = ptr
        for name in ("chosen", "state", "traj", "policy_obs", "steps0", "steps", "rewards", "reward_coef", "step"):
            setattr(a, name, None if name in missing else ptr)
        return a

    def call(geometry=None, a=None, d="default"):
        g = ro.Geometry(**{**good, **(geometry or {})})
        a = settle_args() if a is None else a
        if d == "default":
            d = ro.DissipationArgs(ptr, None, ptr, 22.0 / 64)
        rc = lib.ro_settle_dissipation(None, ctypes.byref(g), ctypes.byref(a), None if d is None else ctypes.byref(d))
        return rc, ro.last_error()

    cases = [(-10, dict(d=None)), (-10, dict(d=ro.DissipationArgs(None, None, ptr, 0.3))),
             (-10, dict(d=ro.DissipationArgs(ptr, ptr, None, 0.3))), (-10, dict(a=settle_args(rewards=True))),
             (-10, dict(a=settle_args(chosen=True))),
             (-11, dict(geometry=dict(L=32))), (-11, dict(geometry=dict(L=128))),
             (-12, dict(d=ro.DissipationArgs(ptr, None, ptr, 0.0))), (-12, dict(d=ro.DissipationArgs(ptr, None, ptr, -0.3))),
             (-12, dict(d=ro.DissipationArgs(ptr, None, ptr, float("nan")))),
             (-12, dict(d=ro.DissipationArgs(ptr, None, ptr, float("inf"))))]
    for code, kwargs in cases:
        rc, message = call(**kwargs)
        assert rc == code, (code, rc, message)
        assert message.startswith("ro_settle_dissipation"), message
    rc, message = call(geometry=dict(N=8, L=8))                # the geometry refusals keep their numbers and their prefix
    assert rc == -4 and message.startswith("rollout:")
    with pytest.raises(ro.RolloutHipError, match="ro_settle_dissipation"):
        ro.settle_dissipation(None, ro.Geometry(**good), settle_args(), ro.DissipationArgs(ptr, None, ptr, 0.0))
