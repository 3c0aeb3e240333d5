"""``PDEModelBasedController`` over ``pdegym.burgers`` on the GPU, built through the controller's own default factories
(``env_id = pdegym.burgers.ENV_ID``, ``env_config``): the toy run of tests/test_controller_gpu.py on the second PDE path
-- N = 64, two sub-steps per step, four steps per episode, five envs, two ``BurgersFNO`` members, ``max_steps = 2``, a
patience early stopping cannot reach -- once with every phase on its kernel tier and once with ``phase_tiers="loop"``, from
the same seeds.

What the two runs must share bit for bit: everything up to and including the first iteration's collection, and at every
later snapshot what does not depend on a value computed by a phase whose own GPU test pins a tolerance: generators,
metadata, env counters.  What lies behind such a phase is held to that phase's constants, named below with their source
lines as tests/test_controller_gpu.py names them.  The FNO route of these phases had not been measured against the
constants at controller level: every comparison prints the observed fraction of its tolerance, and with
``PDECONTROL_PARITY_JSON`` set to a path the fractions are written there (profiles/burgers_controller_parity.json is such
a record)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _controller_scenario as cs  # noqa: E402
import _collect_scenario as sc  # noqa: E402

pytestmark = pytest.mark.gpu

HSTEP_RTOL = 1e-4                          # tests/test_surrogate_phase_gpu.py:154
ROWS_RTOL, ROWS_ATOL = 1e-4, 1e-5          # tests/test_imagination_phase_gpu.py:224
DELTA_ULPS = 2 + 2                         # each tier within 2 ulp of the fp64 twin, tests/test_delta_phase_gpu.py:275
ENV_CONFIG = dict(N=64, cfg_steps=2, Tmax=0.0079)       # Tmax / (dt * cfg_steps) with dt = 1e-3, rounded up: 4 steps
OBSERVED = {}


def _fraction(name, x, y, rtol, atol=0.0):
    """The largest |x - y| in units of the tolerance ``atol + rtol |y|``; printed and kept for the record."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    worst = float(np.max(np.abs(x - y) / (atol + rtol * np.abs(y)))) if x.size else 0.0
    OBSERVED[name] = max(OBSERVED.get(name, 0.0), worst)
    print(f"burgers controller parity, {name}: {worst:.3g} of the tolerance")
    return worst


def _generators(c):
    space = c.envs.action_space
    rng = getattr(space, "_rng", None)
    rng = space.np_random if rng is None else rng
    states = [r.get_state() for r in c.stack.ostore.env._rngs]
    rec = {"numpy": np.random.get_state(), "torch_cpu": torch.get_rng_state().clone(), "space": rng.bit_generator.state,
           "env_keys": np.stack([s[1] for s in states]), "env_pos": np.asarray([s[2:] for s in states], dtype=np.float64),
           "torch_cuda": torch.cuda.get_rng_state(0).clone()}
    return rec


def _snapshot(c):
    env = c.stack.ostore.env
    rows, meta = cs.slabs(c.replay)
    return dict(rows=rows, meta=meta, vmin=c.oscaling.vmin.clone(), vmax=c.oscaling.vmax.clone(), timestep=env.timestep.copy(),
                u=env.u.cpu().numpy(), generators=_generators(c), iteration=c.iteration)


def _run(log_dir, phase_tiers):
    from pdecontrol import architectures
    from pdecontrol.mbrl.mbrl import PDEModelBasedController, RunLog
    from pdegym import burgers
    from pdegym.burgers.burgers import BurgersBatchedVecEnv
    args = cs.toy_args(cuda=True, env_id=burgers.ENV_ID, cpus=5, learning_starts=40, total_timesteps=50, model_rollouts_batch_size=5,
                       surrogate_train_freq=5)
    config = cs.toy_config(max_steps=2, patience=1000)
    config.factory = "BurgersFNO"
    cs.seed()
    c = PDEModelBasedController(burgers.ENV_ID, architectures.BurgersFNO(), config, args, log=RunLog(log_dir),
                                env_config=dict(ENV_CONFIG), phase_tiers=phase_tiers)
    env = c.stack.ostore.env
    assert isinstance(env, BurgersBatchedVecEnv) and isinstance(c.env.unwrapped, burgers.BurgersEnv)
    assert (env.num_envs, env.N, env.max_episode_steps, env.device.type) == (5, 64, 4, "cuda")
    assert len(c.modules) == 2 and all(type(m.surrogate).__name__ == "FNOAutoRegSurrogate" for m in c.modules)
    cs.seed_spaces(c)
    snapshots, extend = [], c.replay.extend

    def recorded(rollout):                 # after the warm-up and after each iteration's collection
        extend(rollout)
        torch.cuda.synchronize()
        snapshots.append(_snapshot(c))

    c.replay.extend = recorded
    c.learn()
    torch.cuda.synchronize()
    return c, snapshots


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    kernel = _run(tmp_path_factory.mktemp("kernel"), "kernel")
    loop = _run(tmp_path_factory.mktemp("loop"), "loop")
    yield kernel, loop
    path = os.environ.get("PDECONTROL_PARITY_JSON")
    if path:
        with open(path, "w") as f:
            json.dump({"unit": "largest observed difference between the kernel-tier run and the loop-tier run, as a fraction "
                               "of the tolerance the test holds it to", "observed": OBSERVED}, f, indent=1, sort_keys=True)


def test_every_phase_runs_on_its_kernel_tier(runs):
    (c, snapshots), (loop, _) = runs
    assert c.iteration == 2 and len(snapshots) == 3
    tiers = {}
    for name, _, tier in c.tiers:
        tiers.setdefault(name, set()).add(tier)
    assert tiers.pop("evaluate_surrogate") == {"loop"}        # one env, a scripted agent: the loop, by design
    assert tiers == {name: {"kernel"} for name in ("warmup", "evaluate", "collect", "update_delta_transform",
                                                   "update_surrogate", "imagine", "update_policy")}, c.tiers
    assert c.tiers[0] == ("warmup", 0, "kernel")
    assert all(t.tier == "kernel" for t in c.trainers), [t.tier_reason for t in c.trainers]
    assert {tier for name, _, tier in loop.tiers if name != "update_surrogate"} == {"loop"}, loop.tiers
    assert all(t.tier == "loop" for t in loop.trainers)
    assert c.replay.device.type == "cuda" and c.world_replay.device.type == "cuda"
    assert loop.replay.device.type == "cuda" and loop.world_replay.device.type == "cuda"
    assert c.replay.ntimesteps == loop.replay.ntimesteps == 40 + 2 * 5
    assert c.world_replay.ntimesteps == loop.world_replay.ntimesteps == 2 * 10 * 2


def _same_generators(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        if k == "numpy":
            assert a[k][0] == b[k][0] and np.array_equal(a[k][1], b[k][1]) and a[k][2:] == b[k][2:], (what, k)
        elif k == "space":
            assert a[k] == b[k], (what, k)
        elif isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k], b[k]), (what, k)
        else:
            assert np.array_equal(a[k], b[k]), (what, k)


def _value_free(a, b, what):
    assert a["meta"] == b["meta"], what
    assert np.array_equal(a["timestep"], b["timestep"]), what
    _same_generators(a["generators"], b["generators"], what)
    for x, y in zip(a["rows"][4:], b["rows"][4:]):            # the flags and the step counters
        assert x.tobytes() == y.tobytes(), what


def _bitwise(a, b, what):
    for name, x, y in zip(sc.FIELDS, a["rows"], b["rows"]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, name)
    assert torch.equal(a["vmin"], b["vmin"]) and torch.equal(a["vmax"], b["vmax"]), what
    assert a["u"].tobytes() == b["u"].tobytes(), (what, "stepper state")


def test_the_collection_equals_the_loop_bit_for_bit(runs):
    """After the warm-up (scripted tier against ``Worker.rollout``) and after the first iteration's collection (SAC tier):
    slabs, metadata, bounds, ``env.timestep``, the stepper's state and all generators.  After the second iteration's
    collection the agent has been through one policy update on imagined rows that the two routes share only to 1e-4:
    generators, metadata, counters and flags are still equal bit for bit, the float rows to that tolerance."""
    (_, kernel), (_, loop) = runs
    for i, (a, b) in enumerate(zip(kernel, loop)):
        _value_free(a, b, i)
    for i in (0, 1):
        _bitwise(kernel[i], loop[i], i)
    a, b = kernel[2], loop[2]
    assert kernel[1]["meta"]["ntimesteps"] == 45
    for name, x, y in zip(sc.FIELDS[:4], a["rows"], b["rows"]):
        _fraction(f"rows after the second collection, {name}", x, y, ROWS_RTOL, ROWS_ATOL)
        np.testing.assert_allclose(x, y, rtol=ROWS_RTOL, atol=ROWS_ATOL, err_msg=name)
    for name in ("vmin", "vmax"):
        _fraction(f"observation bounds after the second collection, {name}", a[name].numpy(), b[name].numpy(), ROWS_RTOL, ROWS_ATOL)
        np.testing.assert_allclose(a[name].numpy(), b[name].numpy(), rtol=ROWS_RTOL, atol=ROWS_ATOL)


def _ulps(a, b):
    a, b = (np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    return np.abs(a - b)


def test_what_lies_behind_a_pinned_tolerance_agrees_to_it(runs):
    """The delta statistics to the ulp bound of their phase's test, the members' validation losses to ``HSTEP_RTOL``, the
    imagined rows and, for want of a constant of their own, the parameters trained on them to the imagined rows' 1e-4
    relative and 1e-5 absolute."""
    (a, _), (b, _) = runs
    mean_a, mean_b = (float(c.undscaling.mean.reshape(())) for c in (a, b))
    var_a, var_b = (float(c.undscaling.var.reshape(())) for c in (a, b))
    print(f"burgers controller parity, undscaling: mean {mean_a!r} / {mean_b!r}, var {var_a!r} / {var_b!r}, count {b.undscaling.count}")
    ulps = int(_ulps(np.float32(var_a), np.float32(var_b)).max())
    OBSERVED["undscaling var"] = ulps / DELTA_ULPS
    print(f"burgers controller parity, undscaling var: {ulps} ulp of {DELTA_ULPS}")
    assert ulps <= DELTA_ULPS, "var"
    # The mean does not hold DELTA_ULPS here, and the yardstick -- the loop tier -- is the reason: it is torch.mean in fp32
    # over n = count * N deltas whose mean is small against their spread, so its rounding error is relative to sum |x| / n
    # <= rms, not to the mean (the kernel tier sums in fp64 and is within 2 ulp of the fp64 twin whatever the cancellation,
    # tests/test_delta_phase_gpu.py:275).  A tree sum of n fp32 terms is off by at most depth * 2^-24 * sum |x|; the depth is
    # taken as 2 ceil(log2 n), twice a balanced tree's, for the short sequential run each thread makes before the tree.
    # Observed on gfx950: 15 ulp of the mean (profiles/burgers_controller_parity.json has the fraction of this bound);
    # nothing in the bound is taken from that figure.
    n = int(b.undscaling.count) * ENV_CONFIG["N"]
    rms = float(np.sqrt(var_b + mean_b ** 2))
    bound = DELTA_ULPS * float(np.spacing(np.float32(abs(mean_b)))) + 2 * int(np.ceil(np.log2(n))) * 2.0 ** -24 * rms
    OBSERVED["undscaling mean"] = abs(mean_a - mean_b) / bound
    print(f"burgers controller parity, undscaling mean: {int(_ulps(np.float32(mean_a), np.float32(mean_b)).max())} ulp, "
          f"{abs(mean_a - mean_b) / bound:.3g} of the summation bound {bound:.3g} (n = {n}, rms {rms:.3g})")
    assert abs(mean_a - mean_b) <= bound, "mean"
    assert a.undscaling.count == b.undscaling.count
    for m, (fa, fb) in enumerate(zip(a.trainers, b.trainers)):
        assert fa.global_step == fb.global_step == 4 and fa.current_epoch == fb.current_epoch
        va, vb = [h["Val. Loss"] for h in fa.history], [h["Val. Loss"] for h in fb.history]
        print("validation losses", va, vb)
        _fraction(f"validation losses, member {m}", va, vb, HSTEP_RTOL)
        np.testing.assert_allclose(va, vb, rtol=HSTEP_RTOL)
    (rows_a, meta_a), (rows_b, meta_b) = cs.slabs(a.world_replay), cs.slabs(b.world_replay)
    assert meta_a == meta_b
    for name, x, y in zip(sc.FIELDS, rows_a, rows_b):
        if x.dtype == np.float32:
            _fraction(f"imagined rows, {name}", x, y, ROWS_RTOL, ROWS_ATOL)
            np.testing.assert_allclose(x, y, rtol=ROWS_RTOL, atol=ROWS_ATOL, err_msg=name)
        else:
            assert x.tobytes() == y.tobytes(), name
    nets = [("policy", a.agent.policy, b.agent.policy), ("critic", a.agent.critic, b.agent.critic),
            ("critic target", a.agent.critic_target, b.agent.critic_target)]
    nets += [(f"member {m}", x, y) for m, (x, y) in enumerate(zip(a.modules, b.modules))]
    for what, x, y in nets:
        worst = 0.0
        for (k, u), (_, v) in zip(x.state_dict().items(), y.state_dict().items()):
            worst = max(worst, _fraction(f"parameters, {what}", u.cpu().numpy(), v.cpu().numpy(), ROWS_RTOL, ROWS_ATOL))
        for (k, u), (_, v) in zip(x.state_dict().items(), y.state_dict().items()):
            np.testing.assert_allclose(u.cpu().numpy(), v.cpu().numpy(), rtol=ROWS_RTOL, atol=ROWS_ATOL, err_msg=f"{what} {k}")
    for k in ("obs", "opred", "actions", "rewards", "rpred"):
        _fraction(f"surrogate evaluation, {k}", a.last_surrogate_eval[k], b.last_surrogate_eval[k], ROWS_RTOL, ROWS_ATOL)
        np.testing.assert_allclose(a.last_surrogate_eval[k], b.last_surrogate_eval[k], rtol=ROWS_RTOL, atol=ROWS_ATOL, err_msg=k)
