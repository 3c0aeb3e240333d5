"""The controller's real-env collection phases (reference ``pdecontrol/mbrl/mbrl.py:397-449``: ``worker.rollout(agent,
sampling)`` and ``eval_worker.rollout(agent, eval_stop)``) behind one call.

``Worker.rollout`` crosses the host four times per step: ``select_action`` (H2D, launch, D2H), the action wrappers in
numpy, the KS step (H2D, launch, D2H of the ``[E, 1, N]`` block, a synchronisation), the observation wrappers in numpy (a
running min / max over the whole block, then an affine map), and ``Sample.split`` + ``ExperienceReplay.add`` (seven
appends per env) under a stop test that re-counts every deque.  ``collect(worker, agent, stop)`` returns the
``ExperienceReplay`` ``worker.rollout(agent, stop)`` returns, on one of two tiers (chosen per call, announced once per
reason; the result carries ``tier``, ``tier_reason`` and ``host_steps``):

loop tier     ``Worker.rollout`` itself: CPU agents and agents that are neither a ``SAC`` nor one of the two scripted
              agents of pdecontrol/mbrl/utils.py, ``PDECONTROL_FUSED=0``, a SAC
              geometry the fused kernels refuse, the CPU twin and ``KSShardedVecEnv``, an env on another device than the
              agent, any stack ``recognize_real_stack`` does not reduce to the controller's.
kernel tier   truncation is the only way an episode ends, so ``plan_phase`` knows from host integers alone how many steps
              the phase takes, at which of them an env truncates, and every sample's ``steps``, calling ``stop`` exactly
              as the loop does.  The plan is cut into segments of consecutive steps without a truncation (and under
              ``SEGMENT_BYTES``).  Inside a segment a step is, eagerly on torch's current stream and with no host
              synchronisation,
                  noise.normal_() -> sac_policy_forward -> co_act -> ks_step_device -> co_observe
              (csrc/collect.hip): the stepper writes its observations straight into the segment's trajectory block.  One
              D2H copy and one synchronisation per segment bring the block back; rewards are formed on the host from the
              fp64 sums with ``KSBatchedVecEnv._finish_step``'s expression and the replay is built with one deque per
              episode and field.  A step at which an env truncates is one ordinary host step of the stack between two
              segments, on the state just written back: the autoreset and the final-observation quirks of
              ``TransformObsWrapper`` are the stack's own.

scripted tier the kernel tier for an agent whose class IS ``pdecontrol.mbrl.utils.RandomAgent`` or ``ActionRepeatAgent``
              (the controller's warm-up and its surrogate evaluation): the actions do not depend on the observation, so a
              segment's ``T`` actions are drawn on the host first, in the loop's order, uploaded once, and the segment is
                  co_act_span -> T x ks_step_device -> co_observe_span
              (include/collect/span.h): ``T + 3`` launches, ``T + 1`` with a frozen or absent scaling, where the SAC tier
              takes ``5 T``.  The device is the env's.  Before anything is drawn the action space must be float32
              ``(E, 1, A)``, the table float32 ``[E, >= nstep + K, 1, A]``; otherwise the loop runs, with that reason.
              Plan, segments, truncation steps, replay build, sink and write-back are the kernel tier's; the result
              carries ``tier = "kernel"``.

There is one segment path.  ``_Segment`` writes slot 0 and the running bounds to the pinned block, uploads them and the
action coefficients and binds the stepper (``env.bind_stream``); a tier's runner (``_run_segment`` for a SAC, ``_run_span``
for a scripted agent) enqueues its launch sequence; ``_Segment.finish`` ends in ``_write_back`` (the whole block comes
back, the rewards are the env's ``rewards_of`` of the fp64 sums) or, with a sink, in ``record_device`` and ``_restore``.
The two steppers (``kspde.KSStepper``, ``pdegym.burgers.burgers.BurgersStepper``) have one face: ``step_device``,
``step_span`` and ``record_device`` on raw device pointers.  What an env knows about itself -- how it binds a stream, how
a reward is formed -- is a method of the env, and nothing here branches on which env it is.

In both tiers everything the loop mutates ends where the loop leaves it: the worker's two observations, the stores, the
scaling's bounds, ``env.timestep``, the stepper's state, the env's MT19937 streams, numpy's and torch's generators, and
the calls to ``callback.on_rollout_end``.  The worker is not reset between calls: consecutive ``collect`` calls continue
the running episodes as consecutive ``rollout`` calls do.

``collect(..., sink=replay)`` (``replay`` a ``DeviceExperienceReplay``) returns a ``StagedRollout`` that
``replay.extend(staged)`` commits, in place of the host ``ExperienceReplay``.  On the kernel tier a segment's transitions
go from the block into the sink's slabs (``sink.slab()``: include/replay/slabs.h) with one ``ks_record_device`` launch
(csrc/ks_record.hip) after its T steps, on the same stream: the rewards are formed on the device, only what the write-back needs comes back to the host (the last
observation row, the last action row, the policy's observation, the bounds and the status), and no host replay is built.
A truncation step's ``Sample`` is packed, uploaded and placed like a host replay's rows.  On the loop tier the loop's host
replay is staged through ``_stage_host``.

A stack over a ``BurgersBatchedVecEnv`` (pdegym/burgers/burgers.py) runs on the same tiers through the env's
``BurgersStepper``: the SAC tier's step is ``... -> co_act -> bg_step -> co_observe``, a scripted segment is
    co_act_span -> bg_step_span -> co_observe_span
(include/burgers_hip.h: its ``step_span`` is all ``T`` steps in one launch, the state held in registers between them; 4
launches with an updating scaling, 2 without), a sink's segment is placed by one ``bg_record`` launch, and the host rewards
are the env's ``ssq * reward_scale()``.  Truncation steps are host steps of the stack, so the env's per-env ``RandomState`` autoreset
exists once.
"""
import gc
from collections import deque
from dataclasses import dataclass
from itertools import chain
from typing import Any, List, Optional

import numpy as np
import torch

from pdecontrol.mbrl.device_replay import _DTYPES, _Episode, _carve, _rows_of, _same_device
from pdecontrol.mbrl.recognition import (FieldMap, Unrecognized, action_store, field_map, flatten, is_forcing, notice,
                                         observation_store, one_channel_each, same_device, updates_statistics)
from pdecontrol.mbrl.replay import ExperienceReplay
from pdecontrol.mbrl.types import Sample
from pdecontrol.mbrl.worker import _stored
from pdecontrol.surrogates import ops
from pdegym.common import transforms as tr
from pdegym.common import vec_wrappers as vw

#: byte budget of one segment's trajectory block (an evaluation phase is 400 steps of 4 MB at 4096 x 256)
SEGMENT_BYTES = 256 << 20


# ----------------------------------------------------------------------------------------------------------------------
# 1. stack recognition
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class RealStackGeometry:
    """What a recognised real-env stack does between the agent and the stepper.

    ``env``         the ``KSBatchedVecEnv`` or ``BurgersBatchedVecEnv`` at the bottom
    ``action``      the scaling of the agent's action columns (identity sensor; ``coef`` None: identity)
    ``record_raw``  the action store sits on top of the scaling: it holds the raw action, else the env-side one
    ``scaling``     the observation ``ScaleTransform`` (scalar bounds) or None
    ``update``      1 when a step joins the block's extrema with the scaling's running bounds first
    ``agent_obs``   the agent sensor over the state columns
    ``kind``        "ks" or "burgers": which of the two steppers ``env`` drives
    """
    env: Any
    action: FieldMap
    record_raw: bool
    scaling: Optional[tr.ScaleTransform]
    update: int
    agent_obs: FieldMap
    kind: str = "ks"


def _bare_scale(t):
    """The ``ScaleTransform`` a wrapper's transform IS (its ``update`` then runs the scalar numpy path), else None."""
    return t if type(t) is tr.ScaleTransform else None


def recognize_real_stack(stack):
    """``RealStackGeometry`` of the controller's collection stack (mbrl.py:259-272) or evaluation stack (:275-291), or
    raises ``Unrecognized`` with the reason.  From the outside in: frozen ``TransformActionWrapper``s that flatten to at
    most one scaling and hold no forcing and no sensor, with the one-step ``StoreNActionsVecWrapper`` that is
    ``stack.astore`` under or on top of them; ``TransformObsWrapper``s and the pass-through ``BaseWorldVecEnvWrapper`` in
    any order, holding sensors and at most one ``ScaleTransform`` with scalar bounds (``aggregate`` and ``batched``), which,
    where it updates, sits directly above the observation store; the one-step ``StoreNObsVecWrapper`` that is
    ``stack.ostore``; a ``KSBatchedVecEnv`` or a ``BurgersBatchedVecEnv``."""
    from pdecontrol.mbrl.world.wrappers import BaseWorldVecEnvWrapper
    from pdegym.burgers.burgers import BurgersBatchedVecEnv
    from pdegym.kuramoto.batched import KSBatchedVecEnv
    env = stack.envs
    above, below, astore = [], [], None
    while True:
        if type(env) is vw.StoreNActionsVecWrapper:
            if astore is not None:
                raise Unrecognized("two action stores")
            action_store(env, stack, "an action store that is not the stack's astore")
            astore = env
        elif type(env) is vw.TransformActionWrapper:
            if is_forcing(env.transform) is not None:
                raise Unrecognized("a forcing in the action stack")
            if updates_statistics(env):
                raise Unrecognized("an action transform that updates its statistics")
            (above if astore is None else below).append(env.transform)
        else:
            break
        env = env.env
    if astore is None:
        raise Unrecognized(f"a {type(env).__name__} in place of the action store")
    chains = []                                           # (steps, wrapper frozen, bare scaling or None), outermost first
    while type(env) in (vw.TransformObsWrapper, BaseWorldVecEnvWrapper):
        if type(env) is vw.TransformObsWrapper:
            chains.append((flatten(env.transform), bool(env.frozen), _bare_scale(env.transform)))
        env = env.env
    ks = observation_store(env, stack)
    if type(ks) not in (KSBatchedVecEnv, BurgersBatchedVecEnv):
        raise Unrecognized(f"a {type(ks).__name__} in place of the KSBatchedVecEnv")
    N, A = one_channel_each(ks, "an env")

    action = field_map(tr.Operation(above + below), A)
    if (action.start, action.stride, action.width) != (0, 1, A):
        raise Unrecognized("a sensor on the agent's actions")
    scaled_above = any(step[0] == "scale" for t in above for step in flatten(t))
    record_raw = action.coef is not None and not scaled_above

    scaling, update, strides = None, 0, []
    for steps, frozen, bare in reversed(chains):          # innermost first: the order the observations pass them
        for step in steps:
            if step[0] == "sensor":
                strides.append(step[1])
                continue
            _, scale, inverse = step
            if scaling is not None:
                raise Unrecognized("two observation scalings")
            if inverse:
                raise Unrecognized("an inverse scaling on the observations")
            if not (scale.aggregate and scale.batched):
                raise Unrecognized("an observation scaling with per-column running bounds (aggregate and batched are not both set)")
            stats = [torch.as_tensor(s) for s in (scale.vmin, scale.vmax, scale.lower, scale.upper)]
            if any(s.numel() != 1 or s.dtype != torch.float32 or s.is_cuda for s in stats):
                raise Unrecognized("an observation scaling whose bounds are not scalar fp32 host values")
            scaling = scale
            if not frozen and not scale.frozen:
                if bare is not scale:
                    raise Unrecognized("a running scaling inside a composite transform")
                if strides:
                    raise Unrecognized("a sensor under the running scaling")
                update = 1
    agent_obs = field_map(tr.Operation([tr.SensorTransform(r) for r in strides]), N)
    return RealStackGeometry(ks, action, record_raw, scaling, update, agent_obs,
                             "burgers" if type(ks) is BurgersBatchedVecEnv else "ks")


# ----------------------------------------------------------------------------------------------------------------------
# 2. the plan
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class PhasePlan:
    """``K`` steps; ``truncations``: the steps (0-based) at which some env truncates; ``steps`` [K, E]: the ``steps``
    column of every sample (``infos["step"]``: the env counter after the step, before an autoreset zeroes it);
    ``timestep``: the env counters after the phase."""
    K: int
    truncations: List[int]
    steps: np.ndarray
    timestep: np.ndarray


def plan_phase(timestep0, max_episode_steps, E, stop):
    """The phase ``Worker.rollout`` runs from env counters ``timestep0``, from host integers only: ``stop`` is called
    with the loop's arguments ``(k * E, nstopped_k)``, k = 0, 1, ..., until it holds, exactly as often as the loop calls
    it.  An env truncates at the step that brings its counter to ``max_episode_steps`` and restarts at 0."""
    ts = np.asarray(timestep0, dtype=np.int64).copy()
    assert ts.shape == (E,), (ts.shape, E)
    k, nstopped, truncations, steps = 0, 0, [], []
    while not stop(k * E, nstopped):
        ts += 1
        steps.append(ts.copy())
        cut = ts >= max_episode_steps
        if cut.any():
            truncations.append(k)
            nstopped += int(cut.sum())
            ts[cut] = 0
        k += 1
    return PhasePlan(k, truncations, np.asarray(steps, dtype=np.int64).reshape(k, E), ts)


def segment_steps(E, N, A, budget=None):
    """Most steps of one segment: its block (trajectory rows, actions, fp64 sums, status) stays under ``budget`` bytes."""
    budget = SEGMENT_BYTES if budget is None else budget
    per_step = E * (4 * N + 4 * A + 8 + 4)
    return max(1, (int(budget) - 4 * E * N) // per_step)


def segments(plan, limit):
    """The plan as ("kernel", first step, steps) runs without a truncation, at most ``limit`` steps each, and
    ("host", step, 1) entries for the steps at which an env truncates."""
    out, k, cuts = [], 0, set(plan.truncations)
    while k < plan.K:
        if k in cuts:
            out.append(("host", k, 1))
            k += 1
            continue
        n = 1
        while n < limit and k + n < plan.K and k + n not in cuts:
            n += 1
        out.append(("kernel", k, n))
        k += n
    return out


# ----------------------------------------------------------------------------------------------------------------------
# 3. the replay
# ----------------------------------------------------------------------------------------------------------------------
def build_replay(pieces, E):
    """The ``ExperienceReplay`` that ``Sample.split`` + ``ExperienceReplay.add`` build step by step, from the phase's
    pieces in time order, with one deque per episode and field.  A piece is a segment ``(traj [T + 1, E, N], actions
    [T, E, A], rewards [T, E] fp64, steps [T, E] int64)`` without a truncation, or one host step as the ``Sample`` of
    ``[E, ...]`` arrays the loop hands to ``split``.  Items are what ``split`` yields: ``[1, N]`` / ``[1, A]`` fp32
    rows, fp64 rewards, numpy bools, int64 steps; the observation a step ends with and the next step starts with are one
    view of the segment's block.  Episode keys and ``vindex`` follow ``add``: an env moves to the next free key the moment
    its sample truncates, in env order."""
    # hundreds of thousands of containers that all stay alive: the cyclic collector would walk them again and again
    # (150 ms against 35 ms at 4096 x 256 x 8 steps on the host this was written on)
    paused = gc.isenabled()
    gc.disable()
    try:
        return _build_replay(pieces, E)
    finally:
        if paused:
            gc.enable()


def _build_replay(pieces, E):
    replay = ExperienceReplay()
    vindex, columns = replay.vindex, {}                  # columns[key][field] = list of per-piece columns, in time order
    free = [0]                                           # ``_next_episode_id`` without its pass over every entry

    def slot(e):
        key = vindex.get(e)
        if key is None:
            key = vindex[e] = free[0]
            free[0] += 1
        cols = columns.get(key)
        if cols is None:
            cols = columns[key] = [[] for _ in range(7)]
        return cols

    for piece in pieces:
        if isinstance(piece, Sample):
            fields = tuple(piece)
            ended = np.logical_or(fields[4], fields[5])
            for e in range(E):
                for col, value in zip(slot(e), fields):
                    col.append(value[e:e + 1])
                if ended[e]:
                    vindex[e] = free[0]
                    free[0] += 1
            continue
        traj, actions, rewards, steps = piece
        T = actions.shape[0]
        # every item once, step by step (numpy hands out the E rows of a step in one pass), then regrouped per env
        rows = [list(traj[t][:, None, :]) for t in range(T + 1)]
        per_env = lambda per_step: list(zip(*per_step))
        obs, nxt = per_env(rows[:T]), per_env(rows[1:])
        act = per_env([list(actions[t][:, None, :]) for t in range(T)])
        rew, stp = per_env([list(rewards[t]) for t in range(T)]), per_env([list(steps[t]) for t in range(T)])
        flags = tuple(np.zeros(T, dtype=np.bool_))
        for e, column in enumerate(zip(obs, act, nxt, rew, stp)):
            cols = slot(e)
            for i, value in zip((0, 1, 2, 3, 6), column):
                cols[i].append(value)
            cols[4].append(flags)
            cols[5].append(flags)
    for key, cols in columns.items():
        for store, col in zip(replay._stores(), cols):
            store[key] = deque(col[0]) if len(col) == 1 else deque(chain.from_iterable(col))
    return replay


# ----------------------------------------------------------------------------------------------------------------------
# 4. the phase
# ----------------------------------------------------------------------------------------------------------------------
def _notice(reason, expected=False):
    notice("the device-resident collection step does not implement %s: the collection phase runs the per-step loop of "
           "Worker.rollout", reason, expected)


def _is_scripted(agent):
    """The agent's class IS one of the two scripted agents of pdecontrol/mbrl/utils.py (no subclass, no namesake)."""
    from pdecontrol.mbrl import utils
    return type(agent) in (utils.RandomAgent, utils.ActionRepeatAgent)


def _scripted_refusal(agent, E, A, steps):
    """Why the scripted tier cannot take this agent's actions for a phase of ``steps()`` steps, or None.  Reads shapes
    and dtypes only: nothing is drawn from the agent."""
    from pdecontrol.mbrl import utils
    if type(agent) is utils.RandomAgent:
        space = agent.action_space
        shape, dtype = getattr(space, "shape", None), getattr(space, "dtype", None)
        if shape is None or tuple(shape) != (E, 1, A) or dtype != np.float32:
            return f"a RandomAgent over an action space of shape {shape} and dtype {dtype} (float32 {(E, 1, A)} is expected)"
        return None
    table = agent.actions
    if not isinstance(table, np.ndarray) or table.dtype != np.float32 or table.ndim != 4 \
            or (table.shape[0], table.shape[2], table.shape[3]) != (E, 1, A):
        return (f"an ActionRepeatAgent whose table is not a float32 array of [{E}, steps, 1, {A}] "
                f"({type(table).__name__} {getattr(table, 'dtype', None)} {tuple(getattr(table, 'shape', ()))})")
    need = int(agent.nstep) + steps()
    if table.shape[1] < need:
        return f"an ActionRepeatAgent whose table holds {table.shape[1]} steps where the phase ends at step {need}"
    return None


def _kernel_tier(worker, agent, stop=None):
    """(RealStackGeometry, FusedSAC, None) when this phase runs on the kernels (FusedSAC is None for a scripted agent,
    which needs ``stop`` to be recognised and runs on the span kernels, include/collect/span.h), else (None, None, reason).
    One chain of checks for both agent families: the scripted one skips the agent's own (the device is the env's) and
    adds, before anything is drawn, the shape of what it will draw."""
    from pdecontrol.sac.sac import SAC

    def loop(reason, expected=False):
        _notice(reason, expected)
        return None, None, reason

    scripted = stop is not None and _is_scripted(agent)
    if not scripted:
        if not isinstance(agent, SAC):
            return loop(f"a {type(agent).__name__} agent (not a SAC)", True)
        if agent.device.type != "cuda":
            return loop("a SAC agent on the CPU", True)
    if not ops.fused_enabled():
        return loop("PDECONTROL_FUSED=0", True)
    try:
        geo = recognize_real_stack(worker.stack)
    except Unrecognized as e:
        return loop(str(e))
    env = geo.env
    E, A = env.num_envs, geo.action.width
    if scripted:
        def steps():                                      # the phase's length, from host integers (a fresh worker resets first)
            start = env.timestep if worker._last_obs is not None else np.zeros(E, dtype=np.int64)
            return plan_phase(start, env.max_episode_steps, E, stop).K

        reason = _scripted_refusal(agent, E, A, steps)
        if reason is not None:
            return loop(reason)
    if env.stepper.device < 0:
        return loop("the CPU twin of the KS stepper")
    if not scripted and not same_device(torch.device("cuda", env.stepper.device), agent.device):
        return loop("an agent and an env on different devices")
    from pdecontrol.mbrl import collect_hip as co
    if env.stepper.n_act != A:
        return loop(f"a stepper with {env.stepper.n_act} actuators under {A} action columns")
    reason = co.supported(co.Geometry(E, 1, env.N, A, geo.agent_obs.start, geo.agent_obs.stride))
    if reason is not None:
        return loop(reason)
    if scripted:
        return geo, None, None
    from pdecontrol.sac import sac_hip
    obs = torch.empty((E, 1, geo.agent_obs.width), dtype=torch.float32, device=agent.device)
    if not sac_hip.use_kernels(agent, obs):                 # announces its own reason
        return loop("a SAC geometry the fused kernels refuse")
    return geo, agent._fused_for(obs), None


def _built_for(geo, agent):
    """What a ``_Buffers`` is built for: the device (a scripted agent, ``agent`` None, stands on the env's) and the key
    ((E, N, A, O, sensor), the shape of the policy's noise or None)."""
    env, obs = geo.env, geo.agent_obs
    shape = (env.num_envs, env.N, geo.action.width, obs.width, (obs.start, obs.stride))
    if agent is None:
        return torch.device("cuda", env.stepper.device), (shape, None)
    return agent.device, (shape, (agent.policy.achannels, agent.policy.aheight))


class _Buffers:
    """Device and pinned host memory of the kernel tier, kept on the worker between phases: the segment block and a
    sink's index block (both grown on demand) and the action coefficients; built for a SAC (``agent``), the agent-side
    buffers and the per-step workspace; for a scripted agent (``agent`` None), the segment's action table and the span
    workspace, grown on demand by ``span``."""

    def __init__(self, geo, agent=None):
        device, self.key = _built_for(geo, agent)
        self.device = torch.empty(0, device=device).device
        (self.E, self.N, self.A, self.O, self.sensor), policy = self.key
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=self.device)
        self.coef = f32(4, self.A)
        self.block = self.block_host = None
        self.capacity = 0
        self.index = self.index_host = None               # a sink's [dst int64 TE | steps int32 TE], grown on demand
        self.table = self.table_host = self.env_actions = self.span_workspace = None
        if agent is not None:
            from pdecontrol.mbrl import collect_hip as co
            self.noise = f32(self.E, *policy)
            self.action, self.env_action = f32(self.E, self.A), f32(self.E, self.A)
            self.workspace = f32(co.workspace_floats(co.Geometry(self.E, 1, self.N, self.A, *self.sensor)))

    def matches(self, geo, agent=None):
        device, key = _built_for(geo, agent)
        return same_device(self.device, device) and self.key == key

    def layout(self, T):
        """Offsets (in floats) of [traj (T+1)EN | actions TEA | policy_obs EO | bounds 4 | pad | ssq TE fp64 | status TE]."""
        E, N, A, O = self.E, self.N, self.A, self.O
        sizes = [(T + 1) * E * N, T * E * A, E * O, 4]
        sizes.append(sum(sizes) % 2)                      # the fp64 sums start 8-byte aligned
        sizes += [2 * T * E, T * E]
        return np.concatenate(([0], np.cumsum(sizes)))

    def views(self, T):
        """(device views, host views) of a segment of ``T`` steps: traj, actions, policy_obs, bounds, ssq, status."""
        off = self.layout(T)
        if off[-1] > self.capacity:
            self.capacity = int(off[-1])
            self.block = torch.empty(self.capacity, dtype=torch.float32, device=self.device)
            self.block_host = torch.empty(self.capacity, dtype=torch.float32).pin_memory()
        E, N, A, O = self.E, self.N, self.A, self.O

        def cut(block):
            part = lambda i: block[int(off[i]):int(off[i + 1])]
            return (part(0).view(T + 1, E, N), part(1).view(T, E, A), part(2).view(E, 1, O), part(3),
                    part(5).view(torch.float64).view(T, E), part(6).view(torch.int32).view(T, E))

        return cut(self.block), cut(self.block_host), int(off[-1])

    def index_views(self, T):
        """(device, pinned host) pairs of a segment's ``dst`` (int64 [T, E]) and ``steps`` (int32 [T, E]): one block, so
        that one copy uploads both."""
        n = T * self.E
        words = n + (n + 1) // 2
        if self.index is None or self.index.numel() < words:
            self.index = torch.empty(words, dtype=torch.int64, device=self.device)
            self.index_host = torch.empty(words, dtype=torch.int64).pin_memory()
        cut = lambda block: (block[:n].view(T, self.E), block[n:words].view(torch.int32)[:n].view(T, self.E))
        return cut(self.index), cut(self.index_host), words

    def span(self, T):
        """(device table, pinned host table, stepper action rows) of ``[T, E, A]`` and the workspace of a ``T``-step span."""
        from pdecontrol.mbrl import collect_hip as co
        n = T * self.E * self.A
        if self.table is None or self.table.numel() < n:
            self.table = torch.empty(n, dtype=torch.float32, device=self.device)
            self.env_actions = torch.empty(n, dtype=torch.float32, device=self.device)
            self.table_host = torch.empty(n, dtype=torch.float32).pin_memory()
        floats = co.span_workspace_floats(co.Geometry(self.E, T, self.N, self.A, *self.sensor))
        if self.span_workspace is None or self.span_workspace.numel() < floats:
            self.span_workspace = torch.empty(co.SPAN_MAX_PARTS * 2, dtype=torch.float32, device=self.device)
        shape = (T, self.E, self.A)
        return (self.table[:n].view(shape), self.table_host[:n].view(shape), self.env_actions[:n].view(shape),
                self.span_workspace)


class _SinkPhase:
    """The ``StagedRollout`` one ``collect(..., sink=)`` call fills on the kernel tier: ``_build_replay``'s keys and
    ``vindex`` (its ``slot()`` rule, an env moving to the next free key the moment its sample truncates) over rows
    reserved in the sink's slabs."""

    def __init__(self, sink, E, N, A, expect):
        self.sink, self.E = sink, E
        self.staged = sink.stage(E, N, A, expect=expect)
        self.free = 0

    def _episode(self, e):
        vindex, eps = self.staged.vindex, self.staged._eps
        key = vindex.get(e)
        if key is None:
            key = vindex[e] = self.free
            self.free += 1
        ep = eps.get(key)
        if ep is None:
            ep = eps[key] = _Episode()
        return ep

    def reserve(self, T):
        """Rows of one segment: int64 ``dst`` [T, E]; env e's T rows are consecutive and join its current episode."""
        extents = self.sink._reserve(T * self.E)
        for e, piece in enumerate(_carve(extents, T, self.E)):
            ep = self._episode(e)
            ep.extents += piece
            ep.length += T
            ep.stopped = False
        return np.ascontiguousarray(_rows_of(extents).reshape(self.E, T).T)

    def slabs(self):
        """The sink's slabs as they stand (after the segment's reservation: a reservation may grow them)."""
        return self.sink.slab()

    def host_step(self, sample):
        """One host step's ``Sample`` of E rows, packed, uploaded and placed with ``index_copy_`` (``_stage_host``'s
        way); an env whose row ends its episode moves to the next free key."""
        sink, E = self.sink, self.E
        rows = _rows_of(sink._reserve(E))
        index = torch.from_numpy(rows).to(sink.device)
        packed = [np.asarray(field, dtype=dt).reshape((E,) + tuple(slab.shape[1:]))
                  for field, dt, slab in zip(sample, _DTYPES, sink.tensors)]
        for slab, block in zip(sink.tensors, packed):
            slab.index_copy_(0, index, torch.from_numpy(block).to(sink.device))
        terminated, truncated = packed[4], packed[5]
        for e in range(E):
            ep = self._episode(e)
            ep.extents.append((int(rows[e]), 1))
            ep.length += 1
            ep.stopped = bool(truncated[e])
            if terminated[e] or truncated[e]:
                ep.done = True
                self.staged.vindex[e] = self.free
                self.free += 1


def _host_step(worker, agent, deterministic):
    """One pass of the loop body of ``Worker.rollout``: the ``Sample`` of ``[E, ...]`` arrays it hands to ``split``."""
    envs, ostore, astore = worker.stack.envs, worker.stack.ostore, worker.stack.astore
    with torch.no_grad():
        actions = agent.select_action(worker._last_obs, deterministic=deterministic)
    worker._last_obs, rewards, terminated, truncated, infos = envs.step(actions)
    obs = worker._last_stored_obs.copy()
    worker._last_stored_obs = _stored(ostore, ostore.obs)
    nxtobs = worker._last_stored_obs.copy()
    actions = _stored(astore, astore.actions)
    if "final_observation" in infos:
        index = infos["_final_observation"]
        nxtobs[index] = ostore.finals[index].copy()[ostore.mask[index]]
    return Sample(obs, actions, nxtobs, rewards, terminated, truncated, infos["step"])


class _Segment:
    """``T`` steps without a truncation, from the state the worker and the stack hold: the shared prologue (``__init__``)
    and the shared finish around a tier's launch sequence.  ``dev`` and ``host`` are the block's device and pinned views
    (traj, actions, policy_obs, bounds, ssq, status), ``coef`` the action coefficients on the device or None,
    ``current`` torch's current stream, which the stepper is bound to."""

    def __init__(self, worker, geo, buf, T, policy_obs):
        """Slot 0 and the running bounds (``policy_obs``: and the policy's observation) written to the pinned block and
        uploaded, the action coefficients uploaded, the stepper bound."""
        from pdecontrol.mbrl import collect_hip as co
        scaling, E, N = geo.scaling, buf.E, buf.N
        self.worker, self.geo, self.buf, self.T = worker, geo, buf, T
        self.dev, self.host, self.used = buf.views(T)
        (traj, _, pobs, bounds, _, _), (h_traj, _, h_pobs, h_bounds, _, _) = self.dev, self.host
        h_traj[0].copy_(torch.from_numpy(np.ascontiguousarray(worker._last_stored_obs, dtype=np.float32).reshape(E, N)))
        uploads = [(traj[0], h_traj[0])]
        if policy_obs:
            h_pobs.copy_(torch.from_numpy(np.ascontiguousarray(worker._last_obs, dtype=np.float32).reshape(h_pobs.shape)))
            uploads.append((pobs, h_pobs))
        if scaling is not None:
            h_bounds[0] = h_bounds[2] = float(scaling.vmin)
            h_bounds[1] = h_bounds[3] = float(scaling.vmax)
        uploads.append((bounds, h_bounds))
        for dst, src in uploads:
            dst.copy_(src, non_blocking=True)
        self.geometry = co.Geometry(E, T, N, buf.A, *buf.sensor)
        self.coef = None
        if geo.action.coef is not None:
            buf.coef.copy_(geo.action.coef)
            self.coef = buf.coef
        self.current = torch.cuda.current_stream(buf.device)
        geo.env.bind_stream(self.current)

    def observe_args(self, workspace):
        from pdecontrol.mbrl import collect_hip as co
        scaling, (traj, _, pobs, bounds, _, _) = self.geo.scaling, self.dev
        if scaling is None:
            return co.observe_args(traj, pobs, None, 0.0, 0.0, self.geo.update, workspace)
        return co.observe_args(traj, pobs, bounds, float(scaling.lower), float(scaling.upper), self.geo.update, workspace)

    def finish(self, steps, phase, cell=None):
        """The segment's replay piece after its one synchronisation, the worker and the stack written back; with a
        ``_SinkPhase``, the transitions recorded in the sink by one launch instead, and None.  ``cell``: ``_restore``'s."""
        worker, geo, buf, T = self.worker, self.geo, self.buf, self.T
        (traj, actions, _, _, ssq, _), (h_traj, h_actions, h_pobs, h_bounds, h_ssq, h_status) = self.dev, self.host
        if phase is None:
            buf.block_host[:self.used].copy_(buf.block[:self.used], non_blocking=True)
            self.current.synchronize()                    # the segment's one synchronisation
            return _write_back(worker, geo, T, h_traj.numpy(), h_actions.numpy(), h_pobs.numpy(), h_bounds.numpy(),
                               h_ssq.numpy(), h_status.numpy(), steps, cell)
        E, N, A = buf.E, buf.N, buf.A
        dst = phase.reserve(T)
        (d_dst, d_steps), (h_dst, h_steps), words = buf.index_views(T)
        h_dst.copy_(torch.from_numpy(dst))
        h_steps.copy_(torch.from_numpy(np.asarray(steps, dtype=np.int32)))
        buf.index[:words].copy_(buf.index_host[:words], non_blocking=True)
        geo.env.stepper.record_device(traj.data_ptr(), actions.data_ptr(), A, ssq.data_ptr(), d_steps.data_ptr(), T,
                                      geo.env.cfg_steps, d_dst.data_ptr(), dst, phase.slabs())
        # what the write-back needs, nothing else: the last observation row, the last action row, the policy's
        # observation with the bounds behind it, the status
        off = buf.layout(T)
        for a, b in ((off[0] + T * E * N, off[1]), (off[1] + (T - 1) * E * A, off[2]), (off[2], off[4]), (off[6], off[7])):
            buf.block_host[int(a):int(b)].copy_(buf.block[int(a):int(b)], non_blocking=True)
        self.current.synchronize()                        # the segment's one synchronisation
        _restore(worker, geo, T, h_traj[T].numpy(), h_actions[T - 1].numpy(), h_pobs.numpy(), h_bounds.numpy(),
                 h_status.numpy(), cell)
        return None


def _run_segment(worker, agent, fused, geo, buf, T, steps, phase=None):
    """A segment of the SAC tier: per step, eagerly on torch's current stream,
    noise.normal_() -> sac_policy_forward -> co_act -> the stepper -> co_observe  (5 T launches).
    Returns the segment's replay piece, or, with a ``_SinkPhase``, records the transitions in the sink and returns None."""
    from pdecontrol.mbrl import collect_hip as co
    env, E = geo.env, buf.E
    seg = _Segment(worker, geo, buf, T, policy_obs=True)
    traj, actions, pobs, _, ssq, status = seg.dev
    geometry = seg.geometry
    act_args = co.act_args(buf.action, seg.coef, buf.env_action, actions, geo.record_raw)
    obs_args = seg.observe_args(buf.workspace)
    fused.refresh_current()
    stream, forward = co.stream(), fused.forward_launcher(E, pobs, buf.noise, buf.action)
    d_env_action, substeps = buf.env_action.data_ptr(), env.cfg_steps
    row, slot = E * buf.N * 4, traj.data_ptr()
    d_ssq, d_status = ssq.data_ptr(), status.data_ptr()
    for t in range(T):                                    # eager launches, ``t`` by value, no host synchronisation
        buf.noise.normal_()                               # the draw of ``SAC.act``: same call, shape and device
        forward()
        co.act(stream, geometry, act_args, t)
        env.stepper.step_device(d_actions=d_env_action, n_substeps=substeps, d_obs=slot + (t + 1) * row,
                                d_ssq=d_ssq + t * E * 8, d_status=d_status + t * E * 4)
        co.observe(stream, geometry, obs_args, t)
    return seg.finish(steps, phase)


def _run_span(worker, agent, geo, buf, T, steps, deterministic, phase=None):
    """A segment of the scripted tier: the agent's ``T`` actions are drawn on the host first, in the loop's order, and
    uploaded once; then  co_act_span -> the stepper's ``step_span`` -> co_observe_span  (KS: T step launches, T + 3 in
    all, T + 1 with a frozen or absent scaling; Burgers: one), with the bounds taken from cell 2."""
    from pdecontrol.mbrl import collect_hip as co
    table, h_table, env_actions, workspace = buf.span(T)
    for t in range(T):                                    # the loop's draws, in the loop's order
        drawn = agent.select_action(worker._last_obs, deterministic=deterministic)
        h_table[t].copy_(torch.from_numpy(np.ascontiguousarray(drawn, dtype=np.float32).reshape(buf.E, buf.A)))
    seg = _Segment(worker, geo, buf, T, policy_obs=False)
    traj, actions, _, _, ssq, status = seg.dev
    table.copy_(h_table, non_blocking=True)
    stream = co.stream()
    co.act_span(stream, seg.geometry, co.act_span_args(table, seg.coef, env_actions, actions, geo.record_raw))
    geo.env.stepper.step_span(env_actions.data_ptr(), T, geo.env.cfg_steps, traj.data_ptr(), ssq.data_ptr(), status.data_ptr())
    co.observe_span(stream, seg.geometry, seg.observe_args(workspace))
    return seg.finish(steps, phase, cell=2)


def _write_back(worker, geo, T, traj, actions, policy_obs, bounds, ssq, status, steps, cell=None):
    """A segment's host block (views of the pinned staging: copied here) into the state the loop would hold after these
    ``T`` steps -- stores, bounds, ``env.timestep``, the worker's two observations -- and the segment's replay piece."""
    env = geo.env
    _restore(worker, geo, T, traj[T], actions[T - 1], policy_obs, bounds, status, cell)
    traj, actions = traj.copy(), actions.copy()
    return traj, actions, env.rewards_of(ssq), steps      # the env's own reward expression, every step at once


def _restore(worker, geo, T, last_obs, last_actions, policy_obs, bounds, status, cell=None):
    """The state the loop would hold after these ``T`` steps, from views of the pinned staging (copied here): ``last_obs``
    [E, N] the observations the last step ends with, ``last_actions`` [E, A] its recorded actions.  ``cell``: the offset
    in ``bounds`` of the cell the segment's last launch wrote (a span: 2; default: the per-step ping-pong's)."""
    env, scaling = geo.env, geo.scaling
    ostore, astore = worker.stack.ostore, worker.stack.astore
    bad = np.nonzero(status.any(axis=1))[0]
    if bad.size:
        env._raise_on(status[bad[0]])                     # the first step that shows an overflow, as the loop raises it
    ostore.obs[:, -1] = last_obs[:, None, :]
    ostore.mask[:, -1] = True
    astore.actions[:, -1] = last_actions[:, None, :]
    astore.mask[:, -1] = True
    if geo.update:
        if cell is None:
            cell = 2 * (T & 1)                            # step T - 1 wrote cell T & 1
        as_stat = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float32).reshape(1, 1, 1).copy())
        scaling.vmin, scaling.vmax = as_stat(bounds[cell]), as_stat(bounds[cell + 1])
    env.timestep += T
    worker._last_obs = policy_obs.copy()
    worker._last_stored_obs = _stored(ostore, ostore.obs)


def _check_sink(sink, agent, kernel, env_device=None):
    """The sink is a ``DeviceExperienceReplay`` on the agent's device, or (loop tier only) on the CPU.  An agent without
    a device (a scripted one) stands on the env's, ``env_device``, on the kernel tier."""
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    if not isinstance(sink, DeviceExperienceReplay):
        raise ValueError(f"collect() takes a DeviceExperienceReplay as its sink, not a {type(sink).__name__}")
    device = getattr(agent, "device", None)
    if kernel:
        if device is None:
            if not _same_device(sink.device, env_device):
                raise ValueError(f"the sink is on {sink.device} and the env on {env_device}: the kernels write the env's device")
        elif not _same_device(sink.device, device):
            raise ValueError(f"the sink is on {sink.device} and the agent on {device}: the kernels write the agent's device")
    elif sink.device.type != "cpu" and device is not None and not _same_device(sink.device, device):
        raise ValueError(f"the sink is on {sink.device} and the agent on {device}: a sink is on the agent's device or on "
                         f"the CPU")


def collect(worker, agent, stop, deterministic=False, sink=None):
    """The ``ExperienceReplay`` ``worker.rollout(agent, stop, deterministic)`` returns, with everything the loop mutates
    left where the loop leaves it (module docstring).  The result carries ``tier`` ("loop" or "kernel"), ``tier_reason``
    (why the loop ran; None on the kernel tier) and ``host_steps`` (steps that went through the stack on the host: all of
    them on the loop tier, the truncation steps on the kernel tier).  ``deterministic`` reaches ``agent.select_action``,
    which a ``SAC`` ignores as the reference's does: both tiers sample.

    ``sink``: a ``DeviceExperienceReplay`` on the agent's device (or on the CPU, for the loop tier).  The result is then,
    on either tier, a ``StagedRollout`` whose rows are in the sink's slabs and which ``sink.extend(result)`` commits
    (``result.to_host()`` is the host replay); the worker's callbacks receive ``result.to_host()``.  A step that
    overflows discards the staged rows before it raises."""
    geo, fused, reason = _kernel_tier(worker, agent, stop)
    scripted = geo is not None and fused is None
    if sink is not None:
        _check_sink(sink, agent, geo is not None, None if geo is None else torch.device("cuda", geo.env.stepper.device))
    if geo is None:
        replay = worker.rollout(agent, stop, deterministic)
        result = replay if sink is None else sink._stage_host(replay)
        result.tier, result.tier_reason = "loop", reason
        result.host_steps = replay.ntimesteps // max(len(replay.vindex), 1)
        return result
    env = geo.env
    E = env.num_envs
    with torch.cuda.device(env.stepper.device):
        if worker._last_obs is None:                      # the loop's first act on a fresh worker
            worker._last_obs = worker.stack.envs.reset()
            worker._last_stored_obs = _stored(worker.stack.ostore, worker.stack.ostore.obs)
        plan = plan_phase(env.timestep, env.max_episode_steps, E, stop)
        # one ``_Buffers`` per agent family on the worker: warm-up, collection and evaluation alternate between them
        sac, slot = (None, "_span_buffers") if scripted else (agent, "_collect_buffers")
        buf = getattr(worker, slot, None)
        if buf is None or not buf.matches(geo, sac):
            buf = _Buffers(geo, sac)
            setattr(worker, slot, buf)
        pieces, host_steps = [], 0
        phase = None if sink is None else _SinkPhase(sink, E, env.N, buf.A, plan.K * E)
        try:
            for kind, first, n in segments(plan, segment_steps(E, env.N, buf.A)):
                steps = plan.steps[first:first + n]
                if kind == "host":
                    piece = _host_step(worker, agent, deterministic)
                    host_steps += 1
                    if phase is not None:
                        phase.host_step(piece)
                elif scripted:
                    piece = _run_span(worker, agent, geo, buf, n, steps, deterministic, phase)
                else:
                    piece = _run_segment(worker, agent, fused, geo, buf, n, steps, phase)
                if phase is None:
                    pieces.append(piece)
        except BaseException:
            if phase is not None and phase.staged.state == "open":
                sink.discard(phase.staged)                # the rows of a phase that raised are never committed
            raise
        assert np.array_equal(env.timestep, plan.timestep), "the env counters left the plan"
    result = build_replay(pieces, E) if phase is None else phase.staged
    result.tier, result.tier_reason, result.host_steps = "kernel", None, host_steps
    if worker.callbacks:
        seen = result if phase is None else result.to_host()
        for callback in worker.callbacks:
            callback.on_rollout_end(seen)
    return result
