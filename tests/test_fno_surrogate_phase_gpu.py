"""The surrogate-update phase over an FNO member on the GPU: ``update_surrogate`` on its kernel tier -- one
``sur_gather_windows`` launch into the captured step's static buffers and one replay per training step; per validation
batch one gather, the fused rollout (with ``PDECONTROL_FNO_CHAIN=1`` the teacher-forced launch and one
``fno_forward_chain``) and ``sur_val_loss`` -- against
the hand-written loop of tests/_surrogate_phase_scenario.py fed from the gather's numpy twin, as
tests/test_surrogate_phase_gpu.py::test_kernel_tier_against_the_hand_written_loop does for the ConvLSTM.

The scene is the Burgers path's: a seeded ``BurgersFNO`` at N = 64 whose ``dscaling`` and ``undscaling`` share one
``Normalize``, scripted ragged episodes in a ``DeviceExperienceReplay``, the controller's connector with a
``GaussianForcing`` over 64 columns (4 actuators)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _burgers_world_scenario as bw  # noqa: E402
import _rollout_scenario as rsc  # noqa: E402
import _surrogate_phase_scenario as sc  # noqa: E402

pytestmark = pytest.mark.gpu

LOSS_RTOL, HSTEP_RTOL = 1e-5, 1e-4            # tests/test_surrogate_phase_gpu.py:154
N, TAU = 64, 5
_SCENE = {}


def scene():
    """(namespace, the host side of a Burgers env at N = 64, the controller's transforms over its forcing), built once."""
    if not _SCENE:
        M = bw.repo_namespace()
        env = bw.bare_env(E=1, N=N, cfg_steps=50)                  # tstep = 0.05, the Burgers default
        tf = rsc.transforms(M, types.SimpleNamespace(action_space=env.single_action_space, forcing=env.forcing))
        assert tuple(env.forcing.forcing.shape) == (4, N)
        _SCENE["scene"] = (M, env, tf)
    return _SCENE["scene"]


def fno_module(M, env, stransf, seed, training_mode="delta", **model_kwargs):
    """The controller's training module over a seeded ``BurgersFNO``: tau 5, tbtt 10, delta statistics in a ``Normalize``
    the surrogate's ``dscaling`` and the module's ``undscaling`` share (as ``sc.training_module``)."""
    torch.manual_seed(seed)
    norm = M.T.Normalize(aggregate=True, batched=True)
    norm.mean, norm.var, norm.count = torch.full((1, 1, 1), 0.01), torch.full((1, 1, 1), 0.5), 100
    und = M.T.BatchTransform(norm)
    f = M.factory_cls()
    tstep = env.cfg_steps * env.dt
    sur = f.surrogate(delta=tstep, dscaling=und.Inverse, tau=TAU, training_mode=training_mode, **f.model(**model_kwargs))
    return M.TrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=tstep, delta=tstep, undscaling=und,
                            stransf=stransf, tau=TAU, tbtt=10).to("cuda")


def phase_setup(M, tf, stransf=None, batch_size=8):
    """(kernel-side datamodule over a device replay, reference-side host datamodule, packed host replay, the device replay)"""
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.surrogates.common.datamodule import PDEDataModule
    episodes = sc.scripted_episodes(N)
    host, sink = M.Replay(), DeviceExperienceReplay(device="cuda")
    for part in sc.split_replay(M, episodes):
        host.extend(part)
    for part in sc.split_replay(M, episodes):
        sink.extend(part)
    keys = list(host.episodes)
    assert list(sink.episodes) == keys and len(keys) == 6
    common = dict(train=keys[:4], val=keys[4:], bootstrapping=True, stransf=tf.replay_to_world if stransf is None else stransf,
                  tau=TAU, batch_size=batch_size)
    kernel_dm = PDEDataModule(data=sink.data, curriculum=sc.curriculum(), device_data="cuda", **common)
    ref_dm = PDEDataModule(data=host.data, curriculum=sc.curriculum(), **common)
    return kernel_dm, ref_dm, sc.packed(host), sink


def optimizer_state(module):
    """Parameters and the state of the captured step's torch Adam (capturable: its step counters are device tensors)."""
    params = [p.detach().cpu().numpy() for p in module.surrogate.parameters()]
    opt = module.__dict__["_graph_state"].opt
    assert isinstance(opt, torch.optim.Adam) and len(opt.state) == len(params), "the FNO's captured step keeps torch's Adam"
    adam = [opt.state[p][k].detach().cpu().numpy() for p in module.surrogate.parameters() for k in ("step", "exp_avg", "exp_avg_sq")]
    return params, adam


def same_history(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g["epoch"], g["global_step"]) == (w["epoch"], w["global_step"])
        for name in ("Val. Loss", "Val. Scaled Loss", "Val. Delta Loss"):
            print(f"epoch {g['epoch']} {name}: {abs(g[name] - w[name]) / (LOSS_RTOL * abs(w[name])):.3g} of LOSS_RTOL")
            assert abs(g[name] - w[name]) <= LOSS_RTOL * abs(w[name]), (name, g[name], w[name])
        np.testing.assert_allclose(g["hsteploss"], w["hsteploss"], rtol=HSTEP_RTOL)
        assert g["hsteploss"][0] == 0.0


def robust(history):
    """Every early-stopping decision has a margin of 100 tolerances: consecutive epochs' "Val. Loss" differ by that."""
    values = [h["Val. Loss"] for h in history]
    for a, b in zip(values, values[1:]):
        assert abs(a - b) >= 100 * LOSS_RTOL * max(abs(a), abs(b)), f"scenario unsuitable: epochs at {a} and {b}"


def rng_state():
    return np.random.get_state()[1].tobytes(), np.random.get_state()[2], torch.get_rng_state().numpy().tobytes()


class Spies:
    """During a kernel-tier call: no ``index_select`` on a slab, no pack of the replay; and what validated a batch."""

    def __init__(self, sink):
        from pdecontrol.surrogates import hipops
        from pdecontrol.surrogates.common import dataset as ds
        self.slabs = {t.data_ptr() for t in sink.tensors}
        self.seen, self.val_launches, self.ds, self.hipops = [], 0, ds, hipops

    def install(self, m):
        real_select, real_init, real_val = torch.Tensor.index_select, self.ds.DeviceSubSeqStore.__init__, self.hipops.fused_val_loss

        def select_spy(tensor, *a, **k):
            if tensor.data_ptr() in self.slabs:
                self.seen.append("index_select on a slab")
            return real_select(tensor, *a, **k)

        def init_spy(store, *a, **k):
            self.seen.append("DeviceSubSeqStore.__init__")
            return real_init(store, *a, **k)

        def val_spy(*a, **k):
            self.val_launches += 1
            return real_val(*a, **k)

        m.setattr(torch.Tensor, "index_select", select_spy)
        m.setattr(self.ds.DeviceSubSeqStore, "__init__", init_spy)
        m.setattr(self.hipops, "fused_val_loss", val_spy)


def test_fno_kernel_tier_against_the_hand_written_loop(monkeypatch):
    from pdecontrol.mbrl import surrogate_phase as sp
    from pdecontrol.mbrl.recognition import world_connector
    from pdecontrol.surrogates import fno_hip
    M, env, tf = scene()
    monkeypatch.setenv("PDECONTROL_FNO_CHAIN", "1")       # the validation rollouts as two launches (the other tests: the default)
    kernel_dm, ref_dm, packed, sink = phase_setup(M, tf)
    maps = world_connector(tf.replay_to_world, N, 4)
    assert maps[0].width == maps[1][2].width == N, "the forcing puts the action row on the state's grid"
    kernel, ref = fno_module(M, env, tf.replay_to_world, seed=5), fno_module(M, env, tf.replay_to_world, seed=5)
    assert fno_hip.world_supported(kernel.surrogate, N)
    monkeypatch.setattr(ref, "_fused_validation_loss", lambda *a, **k: None)     # the reference validates on the torch ops
    spies = Spies(sink)
    chains, real_chain = [], fno_hip.forward_chain

    def both(kernel_fit, ref_fit, **kw):
        np.random.seed(17)
        torch.manual_seed(17)
        before = spies.val_launches
        with monkeypatch.context() as m:
            spies.install(m)
            m.setattr(fno_hip, "forward_chain", lambda *a, **k: (chains.append(a[1:3]), real_chain(*a, **k))[1])
            got = sp.update_surrogate(kernel, kernel_dm, kernel_fit, **kw)
        assert kernel_fit.tier == "kernel", kernel_fit.tier_reason
        assert not spies.seen, spies.seen
        assert spies.val_launches > before, "no validation batch went through sur_val_loss"
        after = rng_state()
        np.random.seed(17)
        torch.manual_seed(17)
        want = sc.reference_fit(ref, ref_dm, ref_fit, packed, maps, **kw)
        assert after == rng_state()
        torch.cuda.synchronize()
        print("kernel", [(h["epoch"], h["global_step"], h["Val. Loss"]) for h in kernel_fit.history])
        print("loop  ", [(h["epoch"], h["global_step"], h["Val. Loss"]) for h in ref_fit.history])
        robust(ref_fit.history)
        assert (kernel_fit.current_epoch, kernel_fit.global_step, kernel_fit.wait_count) == \
               (ref_fit.current_epoch, ref_fit.global_step, ref_fit.wait_count)
        same_history(kernel_fit.history, ref_fit.history)
        assert abs(got - want) <= LOSS_RTOL * abs(want) and abs(kernel_fit.best_score - ref_fit.best_score) <= LOSS_RTOL * abs(want)
        (kp, ka), (rp, ra) = optimizer_state(kernel), optimizer_state(ref)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(kp, rp)), "parameters differ"
        assert all(a.tobytes() == b.tobytes() for a, b in zip(ka, ra)), "Adam state differs"

    kernel_fit, ref_fit = sp.FitState(), sp.FitState()
    both(kernel_fit, ref_fit, max_steps=7, min_steps=2, patience=1)
    first_epochs = kernel_fit.current_epoch
    assert kernel_fit.global_step >= 2 and first_epochs >= 2                    # the curriculum changed T between epochs
    shapes = {k[0][:2] for k in kernel.__dict__["_graphed_steps"]}
    assert any(b < 8 for b, _ in shapes) and len({t for _, t in shapes}) == 2   # ragged last batches, two window lengths
    assert chains and all(c[0] == N for c in chains), "the validation rollouts ran their free-running steps as one chain"

    # the delta statistics are re-fitted between iterations (update_delta_transform): the captured steps are re-captured
    steps_before = dict(kernel.__dict__["_graphed_steps"])
    for m in (kernel, ref):
        norm = m.undscaling.transform
        norm.reset()
        norm.update(torch.linspace(-0.6, 0.9, 64).reshape(64, 1, 1))
    both(kernel_fit, ref_fit, max_steps=3, min_steps=0, patience=1, max_epochs=1)
    assert kernel_fit.current_epoch == first_epochs + 1
    assert any(kernel.__dict__["_graphed_steps"][k] is not v for k, v in steps_before.items()), "nothing was re-captured"


def test_a_decoded_mode_fno_trains_on_the_tier_and_validates_through_validation_step(monkeypatch):
    """``sur_val_loss`` is the delta-mode loss: a ``training_mode="decoded"`` member keeps the gather and the captured step
    and sends every validation batch through ``validation_step`` into the meter."""
    from pdecontrol.mbrl import surrogate_phase as sp
    from pdecontrol.mbrl.recognition import world_connector
    M, env, tf = scene()
    kernel_dm, ref_dm, packed, sink = phase_setup(M, tf)
    maps = world_connector(tf.replay_to_world, N, 4)
    kernel = fno_module(M, env, tf.replay_to_world, seed=6, training_mode="decoded")
    ref = fno_module(M, env, tf.replay_to_world, seed=6, training_mode="decoded")
    assert kernel.training_mode == "decoded"
    spies, steps = Spies(sink), []
    real_step = kernel.validation_step
    kw = dict(max_steps=3, min_steps=0, patience=1, max_epochs=1)
    kernel_fit, ref_fit = sp.FitState(), sp.FitState()
    np.random.seed(4)
    torch.manual_seed(4)
    with monkeypatch.context() as m:
        spies.install(m)
        m.setattr(kernel, "validation_step", lambda batch, bidx: (steps.append(bidx), real_step(batch, bidx))[1])
        got = sp.update_surrogate(kernel, kernel_dm, kernel_fit, **kw)
    assert kernel_fit.tier == "kernel", kernel_fit.tier_reason
    assert not spies.seen and spies.val_launches == 0 and steps == list(range(len(steps))) and len(steps) >= 1
    np.random.seed(4)
    torch.manual_seed(4)
    want = sc.reference_fit(ref, ref_dm, ref_fit, packed, maps, **kw)
    torch.cuda.synchronize()
    assert np.isfinite(got) and kernel_fit.global_step == ref_fit.global_step == 3
    same_history(kernel_fit.history, ref_fit.history)
    assert abs(got - want) <= LOSS_RTOL * abs(want)
    (kp, ka), (rp, ra) = optimizer_state(kernel), optimizer_state(ref)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(kp, rp)) and all(a.tobytes() == b.tobytes() for a, b in zip(ka, ra))


def test_what_the_tier_does_not_take_runs_the_loop_tier_with_its_reason():
    from pdecontrol.mbrl import surrogate_phase as sp
    from pdecontrol.surrogates import ops
    M, env, tf = scene()
    # an FNO of another width: the whole-network kernels are built for width 32, the member runs operator by operator
    kernel_dm, _, _, _ = phase_setup(M, tf, batch_size=16)
    other = fno_module(M, env, tf.replay_to_world, seed=7, width=16)
    fit = sp.FitState()
    np.random.seed(3)
    value = sp.update_surrogate(other, kernel_dm, fit, max_steps=1, min_steps=0, patience=1, max_epochs=1)
    assert fit.tier == "loop" and fit.global_step == 1 and np.isfinite(value)
    assert fit.tier_reason.startswith(f"an FNO the whole-network kernels do not take at a state row of {N} points"), fit.tier_reason
    # a connector without the forcing: the action row keeps the replay's 4 columns.  The FNO reads the action field at every
    # grid point, so the member cannot evaluate such a batch on any tier (its lift concatenates state and action rows); the
    # phase picks the loop tier and says why before the first batch
    narrow = M.T.SampleTransform([tf.oscaling, tf.world_sensor], [tf.world_sensor])
    narrow_dm, _, _, _ = phase_setup(M, tf, stransf=narrow, batch_size=16)
    member = fno_module(M, env, narrow, seed=7)
    tier, reason = sp._pick_tier(member, narrow_dm)
    assert tier is None
    assert reason == f"an action row of 4 columns beside a state row of {N}: the FNO reads the action field at every grid point"
    fit = sp.FitState()
    ops._NOTIFIED.discard(reason)
    with pytest.raises(Exception):
        sp.update_surrogate(member, narrow_dm, fit, max_steps=1, min_steps=0, patience=1, max_epochs=1)
    assert (fit.tier, fit.tier_reason, fit.global_step) == ("loop", reason, 0)
