"""``PDEModelBasedController`` on the GPU: the toy run of tests/_controller_scenario.py (N = 64, five envs, two members,
``max_steps = 2``, a patience early stopping cannot reach, every member an elite) once with every phase on its kernel
tier and once with ``phase_tiers="loop"`` -- the loop each phase replaces, over the same replays and the same fused
surrogate and SAC kernels -- from the same seeds.

What the two runs must share bit for bit: everything up to and including the first iteration's collection (the warm-up
on the scripted span kernels against ``Worker.rollout``, the SAC collection tier against it), and at every later
snapshot everything that does not depend on a value computed by a phase whose own GPU test pins a tolerance: generators,
metadata, env counters.  The phases behind the first collection are pinned by their own tests to tolerances, not bits
(the delta statistics to 2 ulp of the fp64 twin, tests/test_delta_phase_gpu.py:275; the imagined rows to 1e-4 relative and
1e-5 absolute, tests/test_imagination_phase_gpu.py:224; the validation loss to ``HSTEP_RTOL``,
tests/test_surrogate_phase_gpu.py:154), and those constants are used here for what lies behind them."""
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


def _snapshot(c):
    ks = c.stack.ostore.env
    rows, meta = cs.slabs(c.replay)
    return dict(rows=rows, meta=meta, vmin=c.oscaling.vmin.clone(), vmax=c.oscaling.vmax.clone(), timestep=ks.timestep.copy(),
                stepper=ks.stepper.get_state(), generators=cs.generators(c), iteration=c.iteration)


def _run(log_dir, phase_tiers):
    args = cs.toy_args(cuda=True, cpus=5, learning_starts=40, total_timesteps=50, model_rollouts_batch_size=5, surrogate_train_freq=5)
    c = cs.build(log_dir, args=args, config=cs.toy_config(max_steps=2, patience=1000), device=0, phase_tiers=phase_tiers)
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
    return kernel, loop


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
    assert all(t.tier == "kernel" for t in c.trainers)
    assert {tier for name, _, tier in loop.tiers if name != "update_surrogate"} == {"loop"}, loop.tiers
    assert all(t.tier == "loop" for t in loop.trainers)
    assert c.replay.device.type == "cuda" and c.world_replay.device.type == "cuda"
    assert c.replay.ntimesteps == loop.replay.ntimesteps == 40 + 2 * 5
    assert c.world_replay.ntimesteps == loop.world_replay.ntimesteps == 2 * 10 * 2


def _value_free(a, b, what):
    assert a["meta"] == b["meta"], what
    assert np.array_equal(a["timestep"], b["timestep"]), what
    cs.same_generators(a["generators"], b["generators"], what)
    for x, y in zip(a["rows"][4:], b["rows"][4:]):            # the flags and the step counters
        assert x.tobytes() == y.tobytes(), what


def _bitwise(a, b, what):
    for name, x, y in zip(sc.FIELDS, a["rows"], b["rows"]):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, name)
    assert torch.equal(a["vmin"], b["vmin"]) and torch.equal(a["vmax"], b["vmax"]), what
    assert np.array_equal(np.asarray(a["stepper"]), np.asarray(b["stepper"])), (what, "stepper state")


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
    n = kernel[1]["meta"]["ntimesteps"]
    worst = 0.0
    for name, x, y in zip(sc.FIELDS[:4], a["rows"], b["rows"]):
        diff = float(np.max(np.abs(x.astype(np.float64) - y) / (ROWS_ATOL + ROWS_RTOL * np.abs(y)))) if x.size else 0.0
        worst = max(worst, diff)
        print(f"rows after the second collection, {name}: {diff:.3g} of the tolerance")
        np.testing.assert_allclose(x, y, rtol=ROWS_RTOL, atol=ROWS_ATOL, err_msg=name)
    np.testing.assert_allclose(a["vmin"].numpy(), b["vmin"].numpy(), rtol=ROWS_RTOL, atol=ROWS_ATOL)
    np.testing.assert_allclose(a["vmax"].numpy(), b["vmax"].numpy(), rtol=ROWS_RTOL, atol=ROWS_ATOL)
    assert n == 45


def _ulps(a, b):
    a, b = (np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    return np.abs(a - b)


def test_what_lies_behind_a_pinned_tolerance_agrees_to_it(runs):
    """The delta statistics to the ulp bound of their phase's test, the members' validation losses to ``HSTEP_RTOL``, the
    imagined rows and, for want of a constant of their own, the parameters trained on them to the imagined rows' 1e-4
    relative and 1e-5 absolute."""
    (a, _), (b, _) = runs
    for name in ("mean", "var"):
        x, y = getattr(a.undscaling, name).cpu().numpy(), getattr(b.undscaling, name).cpu().numpy()
        print(f"undscaling {name}: {int(_ulps(x, y).max())} ulp")
        assert _ulps(x, y).max() <= DELTA_ULPS, name
    assert a.undscaling.count == b.undscaling.count
    for fa, fb in zip(a.trainers, b.trainers):
        assert fa.global_step == fb.global_step == 4 and fa.current_epoch == fb.current_epoch
        va, vb = [h["Val. Loss"] for h in fa.history], [h["Val. Loss"] for h in fb.history]
        print("validation losses", va, vb)
        np.testing.assert_allclose(va, vb, rtol=HSTEP_RTOL)
    (rows_a, meta_a), (rows_b, meta_b) = cs.slabs(a.world_replay), cs.slabs(b.world_replay)
    assert meta_a == meta_b
    for name, x, y in zip(sc.FIELDS, rows_a, rows_b):
        if x.dtype == np.float32:
            np.testing.assert_allclose(x, y, rtol=ROWS_RTOL, atol=ROWS_ATOL, err_msg=name)
        else:
            assert x.tobytes() == y.tobytes(), name
    nets = [(a.agent.policy, b.agent.policy), (a.agent.critic, b.agent.critic), (a.agent.critic_target, b.agent.critic_target)]
    nets += list(zip(a.modules, b.modules))
    for x, y in nets:
        for (k, u), (_, v) in zip(x.state_dict().items(), y.state_dict().items()):
            np.testing.assert_allclose(u.cpu().numpy(), v.cpu().numpy(), rtol=ROWS_RTOL, atol=ROWS_ATOL, err_msg=k)
    for k in ("obs", "opred", "actions", "rewards", "rpred"):
        np.testing.assert_allclose(a.last_surrogate_eval[k], b.last_surrogate_eval[k], rtol=ROWS_RTOL, atol=ROWS_ATOL, err_msg=k)
