"""The controller's phases with the latent ConvLSTM ablation (``--factory KSLatentConvolutionalLSTM``) on an MI355X:
``update_surrogate`` on its kernel tier against its loop tier, one fold of the offline evaluation, and a three-member latent
ensemble in the device-resident world, ``imagine()`` against ``Worker.rollout``.  The scenarios, helpers and bounds are the
ones the autoregressive model is held to (tests/test_surrogate_clip_gpu.py, tests/test_offline_eval_gpu.py,
tests/test_imagination_phase_gpu.py); only the factory differs."""
import numpy as np
import pytest
import torch

import _offline_eval_scenario as osc
import _rollout_scenario as rsc
import _surrogate_phase_scenario as psc
from test_imagination_phase_gpu import (DEVICE_REWARD, _assert_same_generators, _compare_replays, _generator_states,
                                        _host_forcing_is_the_fma_chain, _same, _world_state)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LOSS_RTOL, HSTEP_RTOL = 1e-5, 1e-4            # the kernel-versus-loop tolerances of tests/test_surrogate_phase_gpu.py


def latent_namespace():
    """tests/_rollout_scenario.py's namespace with the latent factories in the autoregressive ones' place."""
    from pdecontrol.architectures import KSLatentConvolutionalLSTM, KSLatentConvolutionalLSTMN
    M = rsc.repo_namespace()
    M.factory_cls, M.factory_n_cls = KSLatentConvolutionalLSTM, KSLatentConvolutionalLSTMN
    return M


# ----------------------------------------------------------------------------------------------------------------------
# the surrogate-update phase
# ----------------------------------------------------------------------------------------------------------------------
def _datamodule(M, env, tf):
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.surrogates.common.datamodule import PDEDataModule
    sink = DeviceExperienceReplay(device="cuda")
    for part in psc.split_replay(M, psc.scripted_episodes(env.N)):
        sink.extend(part)
    keys = list(sink.episodes)
    return PDEDataModule(data=sink.data, curriculum=psc.curriculum(), device_data="cuda", train=keys[:4], val=keys[4:],
                         bootstrapping=True, stransf=tf.replay_to_world, tau=5, batch_size=8)


def _phase(M, env, tf, tier):
    from pdecontrol.mbrl import surrogate_phase as sp
    from pdecontrol.surrogates import hipops
    module, fit = psc.training_module(M, env, tf, "cuda", seed=5), sp.FitState()
    assert hipops.fused_latent_supported(module.surrogate) and not hipops.fused_supported(module.surrogate)
    np.random.seed(17)
    torch.manual_seed(17)
    value = sp.update_surrogate(module, _datamodule(M, env, tf), fit, max_steps=7, min_steps=2, patience=1, tier=tier)
    torch.cuda.synchronize(DEV)
    return module, fit, value, _generator_states()


def test_update_surrogate_takes_the_latent_module_on_the_kernel_tier():
    M = latent_namespace()
    env = M.Env()
    tf = rsc.transforms(M, env)
    kernel, kfit, kvalue, kgen = _phase(M, env, tf, None)
    assert kfit.tier == "kernel", kfit.tier_reason
    loop, lfit, lvalue, lgen = _phase(M, env, tf, "loop")
    assert lfit.tier == "loop"
    for m in (kernel, loop):                              # both trained through captured latent steps, and only those
        steps = list(m.__dict__["_graphed_steps"].values())
        assert steps and all(s.used_latent and s.adam_in_flush for s in steps)
    print("kernel", [(h["epoch"], h["global_step"], h["Val. Loss"]) for h in kfit.history])
    print("loop  ", [(h["epoch"], h["global_step"], h["Val. Loss"]) for h in lfit.history])
    assert (kfit.current_epoch, kfit.global_step, kfit.wait_count) == (lfit.current_epoch, lfit.global_step, lfit.wait_count)
    assert kfit.global_step >= 2 and len(kfit.history) == len(lfit.history)
    for g, w in zip(kfit.history, lfit.history):
        for name in ("Val. Loss", "Val. Scaled Loss", "Val. Delta Loss"):
            assert abs(g[name] - w[name]) <= LOSS_RTOL * abs(w[name]), (name, g[name], w[name])
        np.testing.assert_allclose(g["hsteploss"], w["hsteploss"], rtol=HSTEP_RTOL)
        assert g["hsteploss"][0] == 0.0
    assert abs(kvalue - lvalue) <= LOSS_RTOL * abs(lvalue)
    (kp, ka), (lp, la) = psc.optimizer_state(kernel), psc.optimizer_state(loop)
    assert len(kp) == len(lp) and all(a.tobytes() == b.tobytes() for a, b in zip(kp, lp)), "parameters differ"
    assert len(ka) == len(la) and all(a.tobytes() == b.tobytes() for a, b in zip(ka, la)), "Adam state differs"
    _assert_same_generators(kgen, lgen)


def test_validation_on_the_kernel_tier_reads_time_major_latent_deltas():
    """Under no_grad the latent rollout's deltas are a view of time-major storage (``sur_latent_deltas``), which is what
    ``sur_val_loss`` needs; with gradients on the torch spelling runs and validation keeps its torch ops."""
    M = latent_namespace()
    env = M.Env()
    module = psc.training_module(M, env, rsc.transforms(M, env), "cuda", seed=5)
    rs = np.random.RandomState(2)
    states = torch.from_numpy(rs.uniform(-0.4, 0.4, (3, 6, 1, 64)).astype(np.float32)).cuda()
    actions = torch.from_numpy(rs.uniform(-1, 1, (3, 6, 1, 64)).astype(np.float32)).cuda()
    with torch.no_grad():
        out = module._full_rollout(states, actions)
        assert out.deltas.transpose(0, 1).is_contiguous() and out.outputs.transpose(0, 1).is_contiguous()
        fused = module._fused_validation_loss(out, states)
    assert fused is not None
    graded = module._full_rollout(states, actions)
    assert not graded.deltas.transpose(0, 1).is_contiguous()
    assert torch.equal(out.outputs, graded.outputs.detach())
    torch.testing.assert_close(out.deltas, graded.deltas.detach(), rtol=1e-6, atol=1e-6)
    with torch.no_grad():
        assert module._fused_validation_loss(graded, states) is None
        want = module.undscaling(torch.diff(torch.cat((states[:, :1], out.outputs), dim=1), dim=1) / module.delta)
    # (torch divides by a host scalar through its reciprocal, so not bit for bit; tests/test_sur_decoded_gpu.py pins the bits)
    torch.testing.assert_close(out.deltas, want, rtol=1e-6, atol=1e-6)
    loss, hstep, scalars, deltas, decoded = fused
    ref = psc.val_loss_fp64(states.cpu().numpy(), out.outputs.transpose(0, 1).cpu().numpy(), out.deltas.transpose(0, 1).cpu().numpy(),
                            module.delta, *module._latent_constants(), module._inverse_scaling(64, states.device).cpu().numpy())
    assert abs(float(loss) - ref["loss"]) <= LOSS_RTOL * ref["loss"]
    assert abs(float(scalars[0]) - ref["scaled"]) <= LOSS_RTOL * ref["scaled"]
    assert abs(float(scalars[1]) - ref["delta"]) <= LOSS_RTOL * ref["delta"]


def test_one_offline_fold_with_the_latent_factory_reports_kernel_tiers():
    from pdecontrol import architectures
    from pdecontrol.mbrl import replay_hip
    from pdecontrol.surrogates.evaluation import evaluate as ev
    replay_hip.load()
    env = osc.toy_env(device=0)
    data = osc.toy_dataset(device="cuda")
    fields = tuple(data.tensors)
    factory = architectures.KSLatentConvolutionalLSTM()
    sections = {"model": {}, "surrogate": {}, "curriculum": {}, "trainer": dict(max_epochs=1, gradient_clip_val=0.5),
                "training": dict(tau=osc.TAU, tbtt=10, batch_size=4, patience=5)}
    config = ev.merged_config(factory, "KSLatentConvolutionalLSTM", sections, "MSELoss", osc.TARGET)
    torch.manual_seed(3)
    np.random.seed(3)
    train_idx, test_idx = ev.kfold_indices(osc.EPISODES, 2, 3)[0]
    train_idx, val_idx = ev.fold_split(train_idx, 0.34)
    result = ev.evaluate_fold(fields, train_idx, val_idx, test_idx, env, factory, config, target_length=osc.TARGET, device=DEV)
    assert result.tiers == {"fit": "kernel", "training": "kernel", "training_reason": None, "test": "kernel"}, result.tiers
    assert np.isfinite(result.val_loss) and np.isfinite(result.test.scalars["MSE"])
    steps = list(result.module.__dict__["_graphed_steps"].values())
    assert steps and all(s.used_latent and s.clip == 0.5 for s in steps)


# ----------------------------------------------------------------------------------------------------------------------
# the device-resident world and the imagined-rollout phase
# ----------------------------------------------------------------------------------------------------------------------
def _run_both(members=3):
    """(loop scene, loop replay, loop end, phase scene, phase replay, phase end) from equal generator states, as
    tests/test_imagination_phase_gpu.py's ``_run_both`` with a latent ensemble."""
    from pdecontrol.mbrl import imagination_phase as ip
    out = []
    for phase in (False, True):
        M = latent_namespace()
        s = rsc.build(M, DEV, members=members, world_kwargs=DEVICE_REWARD)
        s.world.setup(s.starting)
        rsc.seed()
        if phase:
            timings = {}
            replay = ip.imagine(s.agent, s.stack, rsc.NUM_ROLLOUTS, False, timings=timings)
            assert timings["tier"] == "kernel", timings
        else:
            replay = M.Worker(s.stack).rollout(s.agent, rsc.stop(rsc.NUM_ROLLOUTS), False)
        torch.cuda.synchronize()
        out += [s, replay, (_generator_states(), _world_state(s.world))]
    return out


def test_a_latent_ensemble_gets_the_device_world_and_imagine_equals_the_loop():
    from pdecontrol.surrogates import hipops
    ls, loop, lend, ps, phase, pend = _run_both()
    for s in (ls, ps):
        members = [m.surrogate for m in s.ensemble.modules]
        assert len(members) == 3 and all(hipops.fused_latent_supported(m) and not hipops.fused_supported(m) for m in members)
        assert s.world._use_device_path() and s.world._dev is not None, "a latent ensemble keeps its trajectories on the device"
    exact = _host_forcing_is_the_fma_chain(ls)            # the loop's forcing is the host's matmul
    assert loop.nepisodes == 2 * ls.world.num_envs and loop.ntimesteps == 6 * ls.world.num_envs
    _compare_replays(loop, phase, 64, exact)
    _assert_same_generators(lend[0], pend[0])
    (lt, lsim, lstate, lhid), (pt, psim, pstate, phid) = lend[1], pend[1]
    np.testing.assert_array_equal(lt, pt)
    assert lsim == psim == 0
    _same(lstate.cpu(), pstate.cpu(), exact, "world state")
    for x, y in zip(lhid, phid):
        for a, b in zip(x, y):
            _same(a.cpu(), b.cpu(), exact, "hidden state")


def test_a_mixed_ensemble_keeps_the_host_world():
    """One kernel family per ensemble: a latent member beside an autoregressive one does not get the device path."""
    from pdecontrol.architectures import KSAutoRegConvolutionalLSTM
    M = latent_namespace()
    s = rsc.build(M, DEV, members=2, world_kwargs=DEVICE_REWARD)
    f = KSAutoRegConvolutionalLSTM()
    m0 = s.ensemble.modules[0]
    torch.manual_seed(1)
    sur = f.surrogate(delta=m0.delta, dscaling=None, tau=m0.tau, **f.model())
    s.ensemble.modules[1] = M.TrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=m0.tstep, delta=m0.delta,
                                             tau=m0.tau, tbtt=10).to(DEV)
    assert not s.world._use_device_path()
