"""The controller's imagined-rollout phase (reference ``pdecontrol/mbrl/mbrl.py:415-435``) behind one call.

The reference runs, per controller iteration,

    world.setup(starting); rollout = world_worker.rollout(agent, world_stop); world_replay.extend(rollout); world_worker.reset()

where every imagined step crosses the host four times: ``select_action`` (H2D, launch, D2H), the five action wrappers in
numpy, the world step (H2D, graph replay, reward, D2H) and ``Sample.split`` + ``ExperienceReplay.add`` (7 appends per env).
``imagine(agent, stack, num_rollouts)`` returns the ``ExperienceReplay`` a fresh ``Worker(stack)`` returns for the stop
condition ``eps >= num_rollouts``, on one of two tiers (chosen per call, announced once per reason):

loop tier     ``Worker.rollout`` (pdecontrol/mbrl/worker.py): CPU agents, ``PDECONTROL_FUSED=0``, any stack
              ``recognize_stack`` does not reduce to the controller's, worlds that are not device-resident.
kernel tier   the closed loop stays in HBM for a whole round (one reset plus the steps up to the joint truncation of
              ``WorldVecEnv.step_wait``, whose number is known on the host once the reset has drawn its windows).  One
              step is ``noise.normal_()`` plus one hipGraph replay of
                  sac_policy_forward -> ro_act_chain -> every member's fused one-step rollout -> ro_settle
              (csrc/rollout.hip; under the KS env's dissipation objective the last launch is ro_settle_dissipation,
              which recomputes the forcing of the recorded action for the reward's u * phi term, and under the Burgers
              env's ro_settle_burgers_dissipation, which does the same for that env's reward; an ensemble of FNO
              members, which carry no hidden state, is stepped as ro_act_chain -> fno_forward_select -> ro_settle over
              the one buffer of picked rows: one evaluation per env in place of one per member and env); the per-step elite
              draws are made on the host in the loop's order and uploaded once per round; one D2H copy and one
              synchronisation per round bring the trajectory block back, and the replay is built from it with one deque
              per episode and field.

In both tiers the replay is the loop's (bit for bit but the rewards of the kernel tier, which are the fp64 row sums of
``ro_settle`` where the loop squares an fp32 ``vector_norm``, and under dissipation the fp64 sums of
``ro_settle_dissipation`` over the forcing of the recorded action, where the loop forces the action it recovers from the
world's action row), numpy's global generator and torch's CPU and device
generators are left where the loop leaves them, and so are the world's ``timesteps``, ``simulated``, state and hidden
tensors.  ``deterministic`` reaches ``agent.select_action``, which ignores it as the reference's does: both tiers sample.
The host-side stores of the wrapper stack are not written by the kernel tier: the controller drops them with
``world_worker.reset()`` right after the phase.

``imagine(...).device_rollout`` (kernel tier; None otherwise) keeps the phase's samples packed on the device in
``DeviceSubSeqStore.tensors`` order and dtypes, episodes contiguous in the replay's key order, with the ``starts`` of
every episode.  With ``sink=`` (a ``DeviceExperienceReplay``, pdecontrol/mbrl/device_replay.py) the kernel tier
writes the samples into the sink's slabs instead, one ``rp_append`` launch per round, and returns the ``StagedRollout`` that
``sink.extend`` commits: nothing is copied back and nothing is built on the host.
"""
import os
import time
from collections import deque
from dataclasses import dataclass

import numpy as np
import torch

from pdecontrol.mbrl.device_replay import DeviceExperienceReplay, episode_keys
from pdecontrol.mbrl.recognition import (FieldMap, Unrecognized, action_maps, action_store, field_map, notice, observation_store,
                                         one_channel_each, same_device, split_at_forcing, updates_statistics)
from pdecontrol.mbrl.replay import ExperienceReplay
from pdecontrol.mbrl.worker import Worker
from pdecontrol.surrogates import ops
from pdegym.common import transforms as tr
from pdegym.common import vec_wrappers as vw


# ----------------------------------------------------------------------------------------------------------------------
# 1. stack recognition
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class StackGeometry:
    """What a recognised stack does between the agent and the world.

    ``act_in``      the scaling of the agent's action columns before the forcing (identity sensor)
    ``forcing``     the ``GaussianForcing`` matrix [A, L] (fp32, host)
    ``act_out``     sensor and scaling of the forcing columns: the world's action row
    ``agent_obs``   the agent sensor over the world's observation columns
    ``reward``      the rescaling of the world's observation before the reward
    ``objective``   the reward owner's objective, "l2control" or "dissipation": the KS env's
                    ``KuramotoSivashinskyEnv.step_objective``, the Burgers env's ``scenario["objective"]``
    ``dx``          the env's grid spacing L / N (read by the dissipation rewards)
    ``owner``       the reward owner's kind, "ks" or "burgers": the two dissipation rewards are different expressions
    ``nu``          the Burgers env's viscosity (read by its dissipation reward; 0.0 for a KS owner)
    """
    world: object
    act_in: FieldMap
    forcing: torch.Tensor
    act_out: FieldMap
    agent_obs: FieldMap
    reward: FieldMap
    objective: str = "l2control"
    dx: float = 0.0
    owner: str = "ks"
    nu: float = 0.0


def recognize_stack(stack, objectives=("l2control",)):
    """``StackGeometry`` of the controller's imagined-rollout stack (mbrl.py:321-329), or raises ``Unrecognized``:
    ``StoreNActionsVecWrapper`` outermost, then ``TransformActionWrapper``s that flatten to at most one scaling, exactly
    one ``GaussianForcing``, at most one scaling and sensors; ``TransformObsWrapper``s holding only sensors over a
    ``StoreNObsVecWrapper``; a ``WorldVecEnv`` whose observation connector is a stride-1 sensor and at most one scaling
    and whose batched reward is a ``KuramotoSivashinskyEnv``'s, under one of ``objectives`` (the kernel tier passes
    both; the dissipation reward reads the forcing at every grid point, so its forcing must be as wide as the state), or a
    ``BurgersBatchedVecEnv``'s (what ``BurgersEnv.batched_reward_func`` forwards to), whose scenario names l2control or
    dissipation, the latter on the same two conditions."""
    from pdecontrol.mbrl.world.world import WorldVecEnv
    from pdegym.burgers.burgers import BurgersBatchedVecEnv
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    env = stack.envs
    action_store(env, stack, f"a {type(env).__name__} in place of the action store on top of the stack")
    env = env.env
    transforms = []
    while type(env) is vw.TransformActionWrapper:
        if updates_statistics(env):
            raise Unrecognized("an action transform that updates its statistics")
        transforms.append(env.transform)
        split_at_forcing(transforms)         # a second forcing is refused where the walk meets it
        env = env.env
    before, forcing, after = split_at_forcing(transforms)
    if forcing is None:
        raise Unrecognized("an action stack without a GaussianForcing")
    sensors = []
    while type(env) is vw.TransformObsWrapper:
        sensors.append(env.transform)
        env = env.env
    world = observation_store(env, stack)
    if not isinstance(world, WorldVecEnv):
        raise Unrecognized(f"a {type(world).__name__} in place of the WorldVecEnv")
    N, W = one_channel_each(world, "a world")
    act_in, matrix, act_out = action_maps(before, forcing, after)
    if act_out.width != W:
        raise Unrecognized(f"an action stack that yields {act_out.width} columns for a world that takes {W}")
    agent_obs = field_map(tr.Operation(list(reversed(sensors))), N)
    if agent_obs.coef is not None:
        raise Unrecognized("a scaling on the agent's observations")
    reward = field_map(world.stransf.otransf, N)
    if (reward.start, reward.stride) != (0, 1):
        raise Unrecognized("a world whose observation connector carries a sensor of stride above 1")
    owner = getattr(world.batched_reward_func, "__self__", None)
    if isinstance(owner, BurgersBatchedVecEnv):
        # its batched reward is the l2control expression -(1/N) * |obs|^2 that ro_settle forms, or the dissipation
        # expression of ro_settle_burgers_dissipation; the scenario names it
        objective = owner.scenario["objective"]
        if objective not in ("l2control", "dissipation"):
            raise Unrecognized(f"a BurgersBatchedVecEnv whose scenario names the {objective} objective (its batched reward "
                               f"is l2control's)")
        kind, nu = "burgers", float(owner.nu)
    elif not isinstance(owner, KuramotoSivashinskyEnv):
        raise Unrecognized("a world without the batched reward of a KuramotoSivashinskyEnv")
    else:
        objective, kind, nu = owner.step_objective, "ks", 0.0
    if objective not in objectives:
        raise Unrecognized(f"the {objective} objective")
    if owner.N != N:
        raise Unrecognized(f"a reward over {owner.N} grid points for observations of {N}")
    if objective == "dissipation" and int(matrix.shape[1]) != N:
        raise Unrecognized(f"a forcing over {int(matrix.shape[1])} columns under the dissipation reward of {N} grid points")
    return StackGeometry(world, act_in, matrix, act_out, agent_obs, reward, objective, owner.L / owner.N, kind, nu)


def round_length(timesteps0, horizon, max_episode_steps):
    """Steps of the round that starts at env counters ``timesteps0``: the first ``s`` at which ``WorldVecEnv.step_wait``
    truncates, that is ``s >= horizon`` or every ``timesteps0 + s >= max_episode_steps``."""
    timesteps0 = np.asarray(timesteps0)
    s = 1
    while not (s >= horizon or np.all(timesteps0 + s >= max_episode_steps)):
        s += 1
    return s


# ----------------------------------------------------------------------------------------------------------------------
# 2. the captured step
# ----------------------------------------------------------------------------------------------------------------------
class DeviceRollout:
    """The phase's samples packed on the device: ``tensors`` in ``DeviceSubSeqStore.tensors`` order and dtypes, episodes
    contiguous in key order, ``starts[key]`` the first row of each."""

    def __init__(self, tensors, starts, device):
        self.tensors, self.starts, self.device = tuple(tensors), dict(starts), device
        self.total = int(self.tensors[0].shape[0])


def _coef(fmap, device):
    return None if fmap.coef is None else fmap.coef.to(device=device, dtype=torch.float32).contiguous()


def _same_coef(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and torch.equal(a, b))


def _select_wanted():
    """``PDECONTROL_FNO_SELECT=0`` keeps the generic member loop for an ensemble of FNO members (every member's one-step
    rollout, then ``ro_settle`` over all outputs): the A/B partner of the select kernel, and its fallback."""
    return os.environ.get("PDECONTROL_FNO_SELECT", "1") != "0"


class _CapturedStep:
    """Static buffers and the hipGraph of one imagined step for one (world state, agent, stack geometry, horizon)."""

    def __init__(self, agent, fused, geo):
        from pdecontrol.mbrl import rollout_hip as ro
        from pdecontrol.surrogates import fno_hip
        from pdecontrol.surrogates.graph_step import capture_graph
        from pdecontrol.surrogates.hipops import pooled_streams
        world = geo.world
        dev = world._dev
        device = dev.device
        self.dev, self.fused, self.version = dev, fused, fused.version
        B, N, T = dev.b, dev.n, max(int(world.horizon), 1)
        A, L = (int(v) for v in geo.forcing.shape)
        O = geo.agent_obs.width
        self.B, self.N, self.T, self.A, self.O = B, N, T, A, O
        self.geometry = ro.Geometry(B, T, N, A, L, geo.act_out.start, geo.act_out.stride, geo.agent_obs.start,
                                    geo.agent_obs.stride, len(dev.members))
        self.maps = (geo.act_in, geo.act_out, geo.agent_obs, geo.reward)
        self.objective, self.dx, self.owner, self.nu = geo.objective, float(geo.dx), geo.owner, float(geo.nu)
        self.forcing_host = geo.forcing
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=device)
        self.forcing = geo.forcing.to(device)
        self.coefs = [_coef(m, device) for m in (geo.act_in, geo.act_out, geo.reward)]
        self.coefs_host = [m.coef for m in (geo.act_in, geo.act_out, geo.reward)]
        # the trajectory block of one round, one D2H copy: [traj (T+1)BN | actions TBA | rewards TB | steps TB (int32)]
        sizes = ((T + 1) * B * N, T * B * A, T * B, T * B)
        self.block = f32(sum(sizes))
        traj, actions, rewards, steps = torch.split(self.block, sizes)
        self.traj, self.actions = traj.view(T + 1, B, N), actions.view(T, B, A)
        self.rewards, self.steps = rewards.view(T, B), steps.view(torch.int32).view(T, B)
        self.sizes = sizes
        self.block_host = torch.empty(self.block.shape, dtype=torch.float32).pin_memory()
        # per round one upload: [chosen T*B | steps0 B] int32
        self.ints_host = torch.zeros(T * B + B, dtype=torch.int32).pin_memory()
        self.ints = torch.zeros(T * B + B, dtype=torch.int32, device=device)
        self.chosen, self.steps0 = self.ints[:T * B].view(T, B), self.ints[T * B:]
        self.step = torch.zeros(2, dtype=torch.int32, device=device)
        self.policy_obs = f32(B, 1, O)
        self.action = f32(B, A)
        shape = (B, agent.policy.achannels, agent.policy.aheight)
        self.noise = f32(*shape)          # always drawn: ``select_action`` samples whatever ``deterministic`` says
        assert dev.act.numel() == B * geo.act_out.width and dev.state.numel() == B * N and dev.state.is_contiguous()
        act_args = ro.act_args(self.action, self.actions, self.coefs[0], self.forcing, self.coefs[1], dev.act, self.step)
        self.keep = []
        tstep = world.tstep
        # An ensemble of FNO members is stateless: env b needs the evaluation of member chosen[t][b] alone, which
        # fno_forward_select makes in one launch for all envs; ro_settle then sees that buffer as its single member.
        # The world's action row must span the state row (the FNO reads the action field at every grid point).
        self.select_wanted = _select_wanted()
        self.select = (self.select_wanted and geo.act_out.width == N
                       and all(fno_hip.world_supported(m, N) for m in dev.members))
        settle_geometry, sel_args = self.geometry, None
        if self.select:
            settle_geometry = ro.Geometry(B, T, N, A, L, geo.act_out.start, geo.act_out.stride, geo.agent_obs.start,
                                          geo.agent_obs.stride, 1)
            self.picked = f32(B, N)
            sel_args = fno_hip.select_args(dev.members, self.chosen if len(dev.members) > 1 else None, self.step, T,
                                           dev.state, dev.act, self.picked)

        def step():
            fused.forward_launcher(B, self.policy_obs, self.noise, self.action)()
            stream = ro.stream()
            ro.act_chain(stream, self.geometry, act_args)
            if self.select:
                fno_hip.forward_select(stream, N, B, sel_args)
                outs = [self.picked]
            else:
                outs = []
                for sur, hid in zip(dev.members, dev.hidden):
                    r = sur.rollout(states=dev.state, actions=dev.act, times=0.0, targets=tstep, hidden=hid)
                    outs.append(r.outputs.reshape(B, N).contiguous())
                    for h, new in zip(hid, r.hidden):
                        h.copy_(new)
            self.keep = outs
            settle_args = ro.settle_args(outs, self.chosen if len(outs) > 1 else None, dev.state, self.traj, self.policy_obs,
                                         self.steps0, self.steps, self.rewards, self.coefs[2], self.step)
            if self.objective == "dissipation" and self.owner == "burgers":
                ro.settle_burgers_dissipation(stream, settle_geometry, settle_args,
                                              ro.burgers_dissipation_args(self.actions, self.coefs[0], self.forcing, self.dx,
                                                                          self.nu))
            elif self.objective == "dissipation":
                ro.settle_dissipation(stream, settle_geometry, settle_args,
                                      ro.dissipation_args(self.actions, self.coefs[0], self.forcing, self.dx))
            else:
                ro.settle(stream, settle_geometry, settle_args)

        saved = (dev.state.clone(), [tuple(h.clone() for h in hid) for hid in dev.hidden])
        (stream,) = pooled_streams(device, 1, "capture")
        stream.wait_stream(torch.cuda.current_stream(device))
        world.surrogate.eval()
        with torch.cuda.stream(stream), torch.no_grad():
            step()                                                         # warm-up (kernels, allocator)
        self.graph = torch.cuda.CUDAGraph()

        def step_nograd():
            with torch.no_grad():
                step()

        capture_graph(self.graph, step_nograd, stream)
        world.surrogate.train()
        torch.cuda.current_stream(device).wait_stream(stream)
        dev.state.copy_(saved[0])
        for hid, old in zip(dev.hidden, saved[1]):
            for h, sv in zip(hid, old):
                h.copy_(sv)

    def valid(self, fused, geo):
        """The graph still describes this world state, agent and stack; coefficient VALUES that changed are re-uploaded
        into the tensors the graph reads (the controller's observation scaling keeps learning between iterations)."""
        world = geo.world
        if (world._dev is not self.dev or not self.dev.valid() or fused is not self.fused or fused.version != self.version
                or max(int(world.horizon), 1) != self.T or geo.objective != self.objective or float(geo.dx) != self.dx
                or geo.owner != self.owner or float(geo.nu) != self.nu
                or _select_wanted() != self.select_wanted):
            return False
        now = (geo.act_in, geo.act_out, geo.agent_obs, geo.reward)
        if any((a.start, a.stride, a.width, a.coef is None) != (b.start, b.stride, b.width, b.coef is None)
               for a, b in zip(self.maps, now)):
            return False
        if geo.forcing.shape != self.forcing_host.shape:
            return False
        if not torch.equal(geo.forcing, self.forcing_host):
            self.forcing.copy_(geo.forcing)
            self.forcing_host = geo.forcing
        for i, m in enumerate((geo.act_in, geo.act_out, geo.reward)):
            if not _same_coef(m.coef, self.coefs_host[i]):
                self.coefs[i].copy_(m.coef)
                self.coefs_host[i] = m.coef
        self.maps = now
        return True


# ----------------------------------------------------------------------------------------------------------------------
# 3. the phase
# ----------------------------------------------------------------------------------------------------------------------
def _notice(reason):
    notice("the fused imagined-rollout step does not implement %s: the imagined-rollout phase runs the per-step loop of "
           "Worker.rollout", reason)


def _kernel_tier(agent, stack):
    """(StackGeometry, FusedSAC) when this phase runs on the kernels, else (None, None)."""
    from pdecontrol.mbrl import rollout_hip as ro
    from pdecontrol.sac import sac_hip
    if getattr(agent, "device", None) is None:            # a scripted agent (pdecontrol/mbrl/utils.py): no policy to fuse
        _notice(f"a {type(agent).__name__} agent (not a SAC)")
        return None, None
    if agent.device.type != "cuda" or not ops.fused_enabled():
        return None, None
    try:
        geo = recognize_stack(stack, objectives=("l2control", "dissipation"))
    except Unrecognized as e:
        _notice(str(e))
        return None, None
    world = geo.world
    if not world._use_device_path() or world._dev_starting is None:
        _notice("a world that does not keep its trajectories on the device (members the device world path refuses, "
                "no batched reward, or a starting-state dataset it cannot pack)")
        return None, None
    from pdecontrol.mbrl.world.world import _members, _surrogate_device
    if not same_device(_surrogate_device(world.surrogate), agent.device):
        _notice("an agent and a world on different devices")
        return None, None
    A, L = (int(v) for v in geo.forcing.shape)
    geometry = ro.Geometry(world.num_envs, max(int(world.horizon), 1), geo.reward.width, A, L, geo.act_out.start,
                           geo.act_out.stride, geo.agent_obs.start, geo.agent_obs.stride, len(_members(world.surrogate)[0]))
    reason = ro.supported(geometry)
    if reason is not None:
        _notice(reason)
        return None, None
    obs = torch.empty((world.num_envs, 1, geo.agent_obs.width), dtype=torch.float32, device=agent.device)
    if not sac_hip.use_kernels(agent, obs):                 # announces its own reason
        return None, None
    return geo, agent._fused_for(obs)


def _build_replay(rounds, B):
    """(the loop's ``ExperienceReplay``, the episode keys of every round) from the rounds' host blocks: one deque per
    episode and field.  Items are what ``Sample.split`` yields: [1, N] / [1, A] fp32 rows, fp32 rewards, numpy bools,
    int32 steps.  The keys are the ones ``ExperienceReplay.add`` hands out (``device_replay.episode_keys``): rounds of
    several steps get the keys r * B + b and a first round of ONE step interleaves them (0, 2, 4, ... then 1, 3, 5, ...)."""
    replay = ExperienceReplay()
    stores, keys = replay._stores(), []
    for traj, actions, rewards, steps in rounds:
        T = actions.shape[0]
        obs, nxt, act = traj[:T, :, None, :], traj[1:T + 1, :, None, :], actions[:, :, None, :]
        terminated = np.zeros(T, dtype=np.bool_)
        truncated = np.zeros(T, dtype=np.bool_)
        truncated[-1] = True
        keys.append(episode_keys(replay.vindex, B, T))
        for b, key in enumerate(keys[-1]):
            for store, column in zip(stores, (obs[:, b], act[:, b], nxt[:, b], rewards[:, b], terminated, truncated,
                                              steps[:, b])):
                store[key] = deque(column)
    return replay, keys


def _device_rollout(blocks, keys, B, device):
    """``DeviceRollout`` from the rounds' device blocks (traj, actions, rewards, steps): episodes in the replay's key
    order (the order of their first sample), ``keys[r][b]`` the episode of env b in round r."""
    cols, starts, off = [[] for _ in range(7)], {}, 0
    for (traj, actions, rewards, steps), round_keys in zip(blocks, keys):
        T = actions.shape[0]
        major = lambda t: t.transpose(0, 1).reshape((B * T, 1) + tuple(t.shape[2:]))
        flags = torch.zeros((B, T), dtype=torch.bool, device=device)
        last = flags.clone()
        last[:, -1] = True
        for col, t in zip(cols, (major(traj[:T]), major(actions), major(traj[1:T + 1]), rewards.t().reshape(-1),
                                 flags.reshape(-1), last.reshape(-1), steps.t().reshape(-1))):
            col.append(t)
        for b, key in enumerate(round_keys):
            starts[key] = off + b * T
        off += B * T
    return DeviceRollout([torch.cat(c) for c in cols], starts, device)


class _SinkBuffers:
    """Per-round staging of a phase that writes into a sink: without a synchronisation per round every round needs pinned
    host memory of its own for the ints and the destination rows it uploads."""

    def __init__(self, cap, num_rounds):
        self.num_rounds = num_rounds
        self.ints_host = torch.zeros((num_rounds, cap.ints.numel()), dtype=torch.int32).pin_memory()
        self.dst_host = torch.zeros((num_rounds, cap.T * cap.B), dtype=torch.int64).pin_memory()
        self.dst = torch.zeros(cap.T * cap.B, dtype=torch.int64, device=cap.ints.device)


def imagine(agent, stack, num_rollouts, deterministic=False, timings=None, noise=None, sink=None):
    """The ``ExperienceReplay`` ``Worker(stack).rollout(agent, lambda ts, eps: eps >= num_rollouts, deterministic)`` returns
    on a fresh worker (module docstring).  ``deterministic`` is passed to the loop's ``agent.select_action``, which accepts
    and ignores it as the reference's does; the kernel tier therefore samples and draws its noise whatever it says.
    ``timings`` (tools/imagination_phase_bench.py) is an optional dict that receives
    the host seconds of the resets, the steps, the copies back and the replay build, and the tier that ran; on the kernel
    tier each of the four then ends in a device synchronisation, which the phase otherwise does once per round.
    ``noise`` (tests; kernel tier only, like the ``noise`` of ``SAC.update``) is an optional iterable of standard-normal
    tensors [num_envs, achannels, aheight], one per step, used in place of the draws.
    ``sink`` (a ``DeviceExperienceReplay`` on the agent's device): on the kernel tier the samples are placed into the
    sink's slabs by one ``rp_append`` launch per round, reading the round's block in place -- no clone, no copy to the
    host, no deques, one synchronisation at the end of the phase -- and the call returns the ``StagedRollout`` that
    ``sink.extend`` commits (``sink.discard`` frees); ``timings`` then receives ``append_s`` in place of ``copy_s`` and
    ``build_s``.  On the loop tier the host replay is returned as without a sink and ``sink.extend`` uploads it.
    Generators, the world's end state and ``simulated`` / ``timesteps`` do not depend on ``sink``."""
    if sink is not None and not isinstance(sink, DeviceExperienceReplay):
        raise TypeError(f"sink is a {type(sink).__name__}, not a DeviceExperienceReplay")
    geo, fused = (None, None) if num_rollouts <= 0 else _kernel_tier(agent, stack)
    if geo is None:
        if noise is not None:
            raise ValueError("stored noise is a hook of the kernel tier; this call runs the loop tier")
        t0 = time.perf_counter()
        replay = Worker(stack).rollout(agent, lambda ts, eps: eps >= num_rollouts, deterministic)
        replay.device_rollout = None
        if timings is not None:
            timings["loop_s"] = timings.get("loop_s", 0.0) + time.perf_counter() - t0
            timings["tier"] = "loop"
        return replay

    world, device = geo.world, agent.device
    B = world.num_envs
    clock = time.perf_counter

    def lap(name, t0):
        if timings is not None:
            torch.cuda.synchronize(device)
            timings[name] = timings.get(name, 0.0) + clock() - t0
        return clock()

    t = clock()
    fused.refresh_current()
    world._reset_state()                         # the fresh worker's reset; (re)builds the device world state if stale
    cap = getattr(world, "_imagination", None)
    if cap is None or not cap.valid(fused, geo):
        cap = world._imagination = _CapturedStep(agent, fused, geo)
    dev = world._dev
    elite = None if dev.ensemble is None else dev.ensemble.elite_idx
    start, stride, O = geo.agent_obs.start, geo.agent_obs.stride, geo.agent_obs.width
    stream = torch.cuda.current_stream(device)
    rounds, blocks = [], []
    stored = None if noise is None else iter(noise)
    num_rounds = -(-int(num_rollouts) // B)
    staged = buffers = None
    if sink is not None:
        from pdecontrol.mbrl import replay_hip
        import hipbind
        replay_hip.load()
        if not same_device(sink.device, device):
            raise ValueError(f"the sink lives on {sink.device}, the imagined rollouts on {device}")
        staged = sink.stage(B, cap.N, cap.A, expect=num_rounds * B * cap.T)
        buffers = getattr(cap, "sink_buffers", None)
        if buffers is None or buffers.num_rounds < num_rounds:
            buffers = cap.sink_buffers = _SinkBuffers(cap, num_rounds)
    try:
        t = lap("reset_s", t)
        for r in range(num_rounds):
            T = round_length(world.timesteps, world.horizon, world.max_episode_steps)
            ints_host = cap.ints_host if staged is None else buffers.ints_host[r]
            ints = ints_host.numpy()
            if elite is not None:                    # the draw of every step of the round, in the loop's order
                for s in range(T):
                    ints[s * B:(s + 1) * B] = np.random.choice(elite, size=B)
            ints[cap.T * B:] = world.timesteps
            cap.ints.copy_(ints_host, non_blocking=True)
            if staged is not None:                   # the rows of this round's samples, uploaded with its ints
                dst_host = buffers.dst_host[r, :T * B]
                dst_host.copy_(torch.from_numpy(staged.reserve(T).reshape(-1)))
                buffers.dst[:T * B].copy_(dst_host, non_blocking=True)
            state = dev.state.view(B, cap.N)
            cap.traj[0].copy_(state)
            cap.policy_obs.view(B, O).copy_(state[:, start::stride][:, :O])
            cap.step.zero_()
            world.surrogate.eval()
            t = lap("reset_s", t)
            for _s in range(T):
                if stored is not None:
                    cap.noise.copy_(next(stored).reshape(cap.noise.shape), non_blocking=True)
                else:
                    cap.noise.normal_()              # the draw of ``SAC.act``: same call, shape and device
                cap.graph.replay()
            world.surrogate.train()
            world.simulated += T
            world.timesteps += T
            t = lap("steps_s", t)
            if staged is not None:
                replay_hip.append(hipbind.stream(), cap.block.data_ptr(), T, cap.T, B, cap.N, cap.A, buffers.dst.data_ptr(),
                                  dst_host.numpy(), sink.slab())
                t = lap("append_s", t)
                world._reset_state()                 # the reset ``step_wait`` makes at the joint truncation
                assert world._dev is dev and cap.valid(fused, geo), "the world changed inside the phase"
                t = lap("reset_s", t)
                continue
            blocks.append(cap.block.clone())
            cap.block_host.copy_(cap.block, non_blocking=True)
            stream.synchronize()                     # the round's one synchronisation
            host = cap.block_host.numpy()
            traj, actions, rewards, steps = np.split(host, np.cumsum(cap.sizes)[:-1])
            rounds.append((traj.reshape(cap.T + 1, B, cap.N)[:T + 1].copy(), actions.reshape(cap.T, B, cap.A)[:T].copy(),
                           rewards.reshape(cap.T, B)[:T].copy(), steps.view(np.int32).reshape(cap.T, B)[:T].copy()))
            t = lap("copy_s", t)
            world._reset_state()                     # the reset ``step_wait`` makes at the joint truncation
            assert world._dev is dev and cap.valid(fused, geo), "the world changed inside the phase"
            t = lap("reset_s", t)
    except BaseException:
        if staged is not None:
            sink.discard(staged)             # a phase that did not finish leaves no rows behind
        raise
    if staged is not None:
        stream.synchronize()                     # the phase's one synchronisation: the pinned staging may be reused
        if timings is not None:
            timings["tier"] = "kernel"
        return staged
    replay, keys = _build_replay(rounds, B)
    views = []
    for block, (_, actions, _, _) in zip(blocks, rounds):
        T = actions.shape[0]
        traj, act, rew, steps = torch.split(block, cap.sizes)
        views.append((traj.view(cap.T + 1, B, cap.N)[:T + 1], act.view(cap.T, B, cap.A)[:T], rew.view(cap.T, B)[:T],
                      steps.view(torch.int32).view(cap.T, B)[:T]))
    replay.device_rollout = _device_rollout(views, keys, B, device)
    lap("build_s", t)
    if timings is not None:
        timings["tier"] = "kernel"
    return replay
