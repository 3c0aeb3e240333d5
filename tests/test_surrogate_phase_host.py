"""The surrogate-update phase without a GPU: the refusals of ``sur_gather_windows``, ``recognition.world_connector``, the
numpy twin of the gather against the host loader, and the fit rule of ``update_surrogate`` on its loop tier."""
import ctypes
import logging
import math
import os

import numpy as np
import pytest
import torch

import _rollout_scenario as rsc
import _surrogate_phase_scenario as sc
from pdecontrol._compat.lightning import pl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "model-based-pde-control_amd", "lib", "libsurrogate_hip.so")
LOG = logging.getLogger("tests.surrogate_phase")


# ----------------------------------------------------------------------------------------------------------------------
# sur_gather_windows: every refusal, with no device
# ----------------------------------------------------------------------------------------------------------------------
def _source(**changes):
    from pdecontrol.surrogates import hipops
    p = ctypes.c_void_p(16)
    fields = dict(obs=p, actions=p, rowmap=None, total=100, rows=0, obs_width=64, obs_start=0, obs_stride=1, obs_coef=None,
                  act_width=4, act_in_coef=None, forcing=p, forcing_width=64, act_start=0, act_stride=1, act_out_coef=None)
    fields.update(changes)
    return hipops.WindowSource(**fields)


def _call(src, first=16, b=2, l=3, states=16, sw=64, sstr=(192, 64), actions=16, aw=64, astr=(192, 64)):
    from pdecontrol.surrogates import hipops
    lib = hipops.load()
    vp = lambda v: None if v is None else ctypes.c_void_p(v)
    rc = lib.sur_gather_windows(None, None if src is None else ctypes.byref(src), vp(first), b, l, vp(states), sw, sstr[0],
                                sstr[1], vp(actions), aw, astr[0], astr[1])
    return rc, lib.sur_last_error().decode()


REFUSALS = [
    ("no source", -1, lambda: _call(None)),
    ("no first", -1, lambda: _call(_source(), first=None)),
    ("no states", -1, lambda: _call(_source(), states=None)),
    ("no actions out", -1, lambda: _call(_source(), actions=None)),
    ("no obs", -1, lambda: _call(_source(obs=None))),
    ("no action field", -1, lambda: _call(_source(actions=None))),
    ("B = 0", -2, lambda: _call(_source(), b=0)),
    ("L = 0", -2, lambda: _call(_source(), l=0)),
    ("obs width 0", -3, lambda: _call(_source(obs_width=0))),
    ("obs width 1025", -3, lambda: _call(_source(obs_width=1025), sw=1025)),
    ("A = 0", -4, lambda: _call(_source(act_width=0))),
    ("A = 17", -4, lambda: _call(_source(act_width=17))),
    ("obs stride 0", -5, lambda: _call(_source(obs_stride=0))),
    ("action stride 0", -5, lambda: _call(_source(act_stride=0))),
    ("obs start -1", -6, lambda: _call(_source(obs_start=-1))),
    ("obs start past the row", -6, lambda: _call(_source(obs_start=64))),
    ("action start past the forcing", -6, lambda: _call(_source(act_start=64))),
    ("action start past the action row", -6, lambda: _call(_source(forcing=None, act_start=4), aw=4)),
    ("states width", -7, lambda: _call(_source(obs_stride=2), sw=64)),
    ("actions width", -7, lambda: _call(_source(forcing=None), aw=64)),
    ("forcing width 0", -8, lambda: _call(_source(forcing_width=0))),
    ("no rows", -9, lambda: _call(_source(total=0))),
    ("no slab rows", -9, lambda: _call(_source(rowmap=ctypes.c_void_p(16), rows=0))),
    ("batch stride", -10, lambda: _call(_source(), sstr=(63, 64))),
    ("time stride", -10, lambda: _call(_source(), astr=(192, 8))),
]


@pytest.mark.parametrize("what,code,call", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_gather_refuses_before_any_hip_call(what, code, call):
    if not os.path.exists(LIB):
        pytest.skip("libsurrogate_hip.so not built")
    rc, message = call()
    assert rc == code, (what, rc, message)
    assert message.startswith("sur_gather_windows:"), message


def test_gather_probe_names_the_refusal_and_passes_a_sound_geometry():
    if not os.path.exists(LIB):
        pytest.skip("libsurrogate_hip.so not built")
    from pdecontrol.surrogates import hipops
    c = sc.gather_case(0, 64, 4, 2, 3, True, 1, 0, True, False)
    gather = hipops.WindowGather(torch.from_numpy(c.obs), torch.from_numpy(c.actions), None, c.total, c.obs_map, c.act_maps)
    assert gather.refused() is None
    wide = sc.gather_case(0, 1028, 4, 2, 3, True, 1, 0, False, False)
    gather = hipops.WindowGather(torch.from_numpy(wide.obs), torch.from_numpy(wide.actions), None, wide.total, wide.obs_map,
                                 wide.act_maps)
    assert "observation width 1028" in gather.refused()


def test_val_loss_refuses_bad_arguments_before_any_hip_call():
    if not os.path.exists(LIB):
        pytest.skip("libsurrogate_hip.so not built")
    from pdecontrol.surrogates import hipops
    lib, p = hipops.load(), ctypes.c_void_p(16)
    good = dict(states=p, sb=6 * 64, st=64, out_all=p, d_all=p, b=3, t=6, n=64, delta=0.25, mean=0.0, stdv=1.0, inv=None, deltas=None,
                decoded=None, hstep=p, loss=p, scalars=p, accum=None, partial=p, ticket=p)
    for change in (dict(states=None), dict(out_all=None), dict(d_all=None), dict(hstep=None), dict(loss=None), dict(scalars=None),
                   dict(partial=None), dict(ticket=None), dict(b=0), dict(t=1), dict(n=0), dict(sb=63), dict(st=8), dict(delta=0.0),
                   dict(stdv=0.0), dict(stdv=float("nan"))):
        a = dict(good, **change)
        rc = lib.sur_val_loss(None, a["states"], a["sb"], a["st"], a["out_all"], a["d_all"], a["b"], a["t"], a["n"], a["delta"],
                              a["mean"], a["stdv"], a["inv"], a["deltas"], a["decoded"], a["hstep"], a["loss"], a["scalars"],
                              a["accum"], a["partial"], a["ticket"])
        assert rc == -1 and lib.sur_last_error().decode().startswith("sur_val_loss:"), (change, rc)


# ----------------------------------------------------------------------------------------------------------------------
# recognition.world_connector
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    M = rsc.repo_namespace()
    env = M.Env()
    return M, env, rsc.transforms(M, env)


def test_world_connector_on_the_controllers_replay_to_world(scene):
    from pdecontrol.mbrl.recognition import world_connector
    M, env, tf = scene
    obs, (act_in, F, act_out) = world_connector(tf.replay_to_world, env.N, 4)
    assert (obs.start, obs.stride, obs.width) == (0, 1, env.N) and obs.coef.shape == (4, env.N)
    assert torch.equal(obs.coef[0], torch.full((env.N,), -3.0)) and torch.equal(obs.coef[1], torch.full((env.N,), 6.0))
    assert (act_in.start, act_in.stride, act_in.width, act_in.coef) == (0, 1, 4, None)
    assert F.dtype == torch.float32 and tuple(F.shape) == (4, env.N) and torch.equal(F, env.forcing.forcing)
    assert (act_out.start, act_out.stride, act_out.width) == (0, 1, env.N) and act_out.coef.shape == (4, env.N)
    # a scaling in front of the forcing and a stride-2 world sensor behind it
    T = M.T
    stransf = T.SampleTransform([tf.oscaling, T.BatchTransform(T.SensorTransform(stride=2))],
                                [tf.ascaling, tf.forcing, tf.pdescaling, T.BatchTransform(T.SensorTransform(stride=2))])
    obs, (act_in, F, act_out) = world_connector(stransf, env.N, 4)
    assert (obs.start, obs.stride, obs.width) == (1, 2, env.N // 2)
    assert act_in.coef.shape == (4, 4) and (act_out.start, act_out.stride, act_out.width) == (1, 2, env.N // 2)
    assert act_out.coef.shape == (4, env.N // 2)


def test_world_connector_without_a_forcing(scene):
    from pdecontrol.mbrl.recognition import world_connector
    M, env, tf = scene
    world_replay_to_agent = M.T.SampleTransform(atransf=tf.ascaling.Inverse)
    obs, (act_in, F, act_out) = world_connector(world_replay_to_agent, env.N, 4)
    assert (obs.start, obs.stride, obs.width, obs.coef) == (0, 1, env.N, None)
    assert F is None and act_in.coef is None and (act_out.start, act_out.stride, act_out.width) == (0, 1, 4)
    assert act_out.coef.shape == (4, 4)
    replay_to_agent = M.T.SampleTransform([tf.oscaling, tf.agent_sensor], tf.ascaling.Inverse)
    obs, (_, F, act_out) = world_connector(replay_to_agent, env.N, 4)
    assert F is None and obs.coef is not None and act_out.coef is not None
    obs, (_, F, act_out) = world_connector(M.T.SampleTransform(), env.N, 4)
    assert F is None and obs.coef is None and act_out.coef is None and act_out.width == 4


def test_world_connector_refuses_what_the_gather_does_not_do(scene):
    from pdecontrol.mbrl.recognition import Unrecognized, world_connector
    M, env, tf = scene
    T = M.T
    sensor2 = T.BatchTransform(T.SensorTransform(stride=2))
    cases = {
        "two scalings in a row": T.SampleTransform([tf.oscaling, tf.oscaling], [tf.forcing]),
        "a Normalize": T.SampleTransform([T.Normalize(aggregate=True, batched=True)], [tf.forcing]),
        "a sensor on the agent's actions": T.SampleTransform([tf.oscaling], [sensor2, tf.forcing, tf.pdescaling]),
        "two forcings": T.SampleTransform([tf.oscaling], [tf.forcing, tf.forcing]),
    }
    for reason, stransf in cases.items():
        with pytest.raises(Unrecognized) as e:
            world_connector(stransf, env.N, 4)
        assert reason in str(e.value), (reason, str(e.value))
    with pytest.raises(Unrecognized):
        world_connector(T.SampleTransform([tf.oscaling], [tf.ascaling, tf.ascaling, tf.forcing]), env.N, 4)
    with pytest.raises(Unrecognized):
        world_connector(tf.replay_to_world, env.N, 3)          # the forcing takes four actuators
    with pytest.raises(Unrecognized):
        world_connector(tf.oscaling, env.N, 4)                 # not a SampleTransform


# ----------------------------------------------------------------------------------------------------------------------
# the numpy twin against the host loader
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,bootstrapping", ((1, False), (6, True), (25, True)))
def test_the_twin_is_the_host_loaders_batch(scene, length, bootstrapping):
    """obs bit for bit for every window; actions bit for bit for every window whose host matmul is the fma chain on this
    CPU (torch's matmul is not the chain for every shape: the count is logged, and zero is not a skip -- the twin is the
    contract, the host loader's actions a report)."""
    from pdecontrol.mbrl.recognition import world_connector
    M, env, tf = scene
    rp = sc.host_replay(M, sc.scripted_episodes(env.N))
    obs, acts, starts = sc.packed(rp)
    obs_map, act_maps = world_connector(tf.replay_to_world, env.N, 4)
    np.random.seed(4)
    dataset = M.ds.SubSeqDataset(rp.data, length=length, stride=3, bootstrapping=bootstrapping, stransf=tf.replay_to_world)
    loader = M.ds.PDEDataLoader(dataset, batch_size=8, shuffle=False, num_workers=0,
                                collate_fn=M.ds.PDEDataLoader.sample_collate)
    twin = sc.twin_batches(dataset, 8, obs, acts, starts, obs_map, act_maps)
    first = sc.firsts(dataset, starts)
    F = act_maps[1].numpy()
    assert len(twin) == len(loader) and len(first) == len(dataset) > 8
    compared = windows = 0
    for k, ((states, actions), batch) in enumerate(zip(twin, loader)):
        assert states.tobytes() == batch[0].numpy().tobytes(), ("obs", k)
        assert actions.shape == tuple(batch[1].shape)
        for i in range(len(states)):
            windows += 1
            r0 = first[8 * k + i]
            if rsc.host_matmul_is_fma_chain(F, acts[r0:r0 + length][:, None, :]):
                compared += 1
                assert actions[i].tobytes() == batch[1][i].numpy().tobytes(), ("actions", k, i)
    LOG.warning("twin against the host loader (length %d): actions compared on %d of %d windows", length, compared, windows)
    print(f"actions compared on {compared} of {windows} windows")


# ----------------------------------------------------------------------------------------------------------------------
# the fit rule, on the loop tier
# ----------------------------------------------------------------------------------------------------------------------
class TinyModule(pl.LightningModule):
    """A one-weight training module with ``PDETrainingModule``'s surface; validation losses come from a script."""
    lr_gamma, step_size, lr = 1.0, 25, 1e-2

    def __init__(self, script):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))
        self.script, self.seen, self.val_batches = list(script), [], 0

    def _frozen_parameters(self):
        return []

    def training_step(self, batch, bidx):
        self.seen.append(("train", tuple(batch[0].shape)))
        return {"loss": (self.w * batch[0].mean()) ** 2}

    def validation_step(self, batch, bidx):
        self.seen.append(("val", tuple(batch[0].shape)))
        if bidx == 0:
            self.val_batches += 1
        value = self.script[min(self.val_batches - 1, len(self.script) - 1)]
        return {"loss": torch.tensor(value), "hsteploss": torch.full((batch[0].shape[1],), value)}

    def configure_optimizers(self):
        opt = torch.optim.SGD([self.w], lr=self.lr)
        return [opt], [{"scheduler": torch.optim.lr_scheduler.StepLR(opt, step_size=self.step_size), "interval": "epoch"}]


def _datamodule(scene, curriculum=None, batch_size=8):
    from pdecontrol.surrogates.common.datamodule import PDEDataModule
    M, env, tf = scene
    rp = sc.host_replay(M, sc.scripted_episodes(env.N))
    return PDEDataModule(data=rp.data, train=[0, 1, 2, 3], val=[4, 5], bootstrapping=True, stransf=tf.replay_to_world,
                         curriculum=curriculum, tau=5, batch_size=batch_size)


def _fit(scene, script, state=None, **kwargs):
    from pdecontrol.mbrl.surrogate_phase import FitState, update_surrogate
    module, dm = TinyModule(script), _datamodule(scene, kwargs.pop("curriculum", None))
    state = FitState() if state is None else state
    np.random.seed(11)
    value = update_surrogate(module, dm, state, **kwargs)
    return value, state, module, dm


def _train_batches(dm):
    """Training batches of one epoch of ``dm`` at its default curriculum (T = tau + 1): 144 - 4 * 5 windows of stride 6."""
    class Probe:
        current_epoch = global_step = 0
    state = np.random.get_state()
    dm.trainer = Probe()
    n = len(dm.train_dataloader())
    np.random.set_state(state)
    return n


def test_fit_stops_by_patience(scene):
    value, fit, module, dm = _fit(scene, [1.0, 0.5, 0.7, 0.6, 0.1], max_steps=10 ** 6, min_steps=0, patience=2)
    per_epoch = _train_batches(dm)
    assert per_epoch >= 2
    assert (value, fit.best_score, fit.wait_count, fit.current_epoch) == (pytest.approx(0.6), 0.5, 2, 4)
    assert fit.global_step == 4 * per_epoch and fit.tier == "loop"
    assert [h["Val. Loss"] for h in fit.history] == pytest.approx([1.0, 0.5, 0.7, 0.6])
    assert [h["epoch"] for h in fit.history] == [0, 1, 2, 3] and fit.history[0]["hsteploss"].shape == (6,)


def test_an_equal_value_is_no_improvement(scene):
    value, fit, _, _ = _fit(scene, [0.5, 0.5], max_steps=10 ** 6, min_steps=0, patience=1)
    assert (value, fit.wait_count, fit.current_epoch) == (0.5, 1, 2)


def test_patience_is_held_back_by_min_steps(scene):
    probe = _train_batches(_datamodule(scene))
    value, fit, _, _ = _fit(scene, [1.0, 2.0, 3.0, 4.0, 5.0], max_steps=10 ** 6, min_steps=3 * probe + 1, patience=1)
    assert fit.current_epoch == 4 and fit.wait_count == 3 and value == pytest.approx(4.0) and fit.best_score == 1.0


def test_fit_stops_mid_epoch_at_max_steps(scene):
    probe = _train_batches(_datamodule(scene))
    value, fit, module, _ = _fit(scene, [1.0, 0.9, 0.8], max_steps=probe + 2, min_steps=0, patience=5)
    assert fit.global_step == probe + 2 and fit.current_epoch == 2 and value == pytest.approx(0.9)
    assert sum(1 for kind, _ in module.seen if kind == "train") == probe + 2
    assert module.seen[-1][0] == "val"                 # the cut epoch is validated too


def test_best_score_is_carried_over_and_wait_count_resets(scene):
    _, fit, _, _ = _fit(scene, [1.0, 0.25, 0.5], max_steps=10 ** 6, min_steps=0, patience=1)
    assert (fit.best_score, fit.wait_count, fit.current_epoch) == (0.25, 1, 3)
    steps = fit.global_step
    value, fit, _, _ = _fit(scene, [0.375, 0.3125], state=fit, max_steps=10 ** 6, min_steps=0, patience=2)
    # neither beats the 0.25 of the first call: two waits from zero, not from one
    assert (value, fit.best_score, fit.wait_count, fit.current_epoch) == (0.3125, 0.25, 2, 5)
    assert fit.global_step > steps and len(fit.history) == 5


def test_a_nan_stops(scene):
    value, fit, _, _ = _fit(scene, [1.0, float("nan"), 0.1], max_steps=10 ** 6, min_steps=0, patience=50)
    assert math.isnan(value) and fit.current_epoch == 2 and fit.best_score == 1.0


def test_max_epochs(scene):
    value, fit, _, _ = _fit(scene, [1.0, 0.9, 0.8, 0.7], max_steps=10 ** 6, min_steps=0, patience=50, max_epochs=3)
    assert fit.current_epoch == 3 and value == pytest.approx(0.8)


def test_the_curriculum_sees_the_fit_state(scene):
    from pdecontrol.surrogates.common.schedulers import FuncScheduler
    calls = []

    class Spy(FuncScheduler):
        def __call__(self, iteration=None, epoch=None, step=None):
            calls.append((epoch, step))
            return 1 if epoch == 0 else 4

    _, fit, module, dm = _fit(scene, [1.0, 0.9, 0.8], curriculum=Spy(steptype="epoch", func=None), max_steps=10 ** 6,
                              min_steps=0, patience=50, max_epochs=3)
    assert [e for e, _ in calls] == [0, 0, 1, 1, 2, 2]                       # train and val loader of each epoch
    assert calls[0][1] == 0 and calls[1][1] == calls[2][1] > 0 and calls[5][1] == fit.global_step
    assert {s[1] for kind, s in module.seen if kind == "train"} == {6, 9}    # T = tau + K changed between epochs
    assert [h["hsteploss"].shape[0] for h in fit.history] == [6, 9, 9]


def test_numpys_generator_is_consumed_as_by_a_hand_written_loop(scene):
    from pdecontrol.surrogates.common.schedulers import StepScheduler
    curriculum = lambda: StepScheduler(steptype="epoch", steps=[0], values=[1, 3])
    _, fit, module, _ = _fit(scene, [1.0, 0.9, 0.8], curriculum=curriculum(), max_steps=10 ** 6, min_steps=0, patience=50,
                             max_epochs=3)
    after = np.random.randint(0, 2 ** 31 - 1, 4)

    class Trainer:
        current_epoch = global_step = 0
    dm, seen = _datamodule(scene, curriculum()), []
    dm.trainer = Trainer()
    np.random.seed(11)
    for _ in range(3):
        for batch in dm.train_dataloader():
            seen.append(("train", tuple(batch[0].shape)))
            dm.trainer.global_step += 1
        for batch in dm.val_dataloader():
            seen.append(("val", tuple(batch[0].shape)))
        dm.trainer.current_epoch += 1
    assert module.seen == seen and dm.trainer.global_step == fit.global_step
    assert np.array_equal(after, np.random.randint(0, 2 ** 31 - 1, 4))


def test_the_loop_tier_on_the_real_module(scene, caplog):
    """``PDETrainingModule`` on the CPU: the optimizer of ``configure_optimizers`` is kept on the fit state, the three
    validation metrics are sample-weighted means of ``validation_step``'s, the tier is announced once."""
    from pdecontrol.mbrl.surrogate_phase import FitState, update_surrogate
    from pdecontrol.surrogates import ops
    M, env, tf = scene
    torch.manual_seed(0)
    f = M.factory_cls()
    tstep = env.cfg_steps * env.dt
    module = M.TrainingModule(surrogate=f.surrogate(delta=tstep, dscaling=None, tau=5, **f.model(N=env.N)),
                              loss=torch.nn.MSELoss(reduction="none"), tstep=tstep, delta=tstep, tau=5, tbtt=10,
                              stransf=tf.replay_to_world)
    dm, fit = _datamodule(scene, batch_size=16), FitState()
    before = [p.detach().clone() for p in module.parameters()]
    ops._NOTIFIED.discard("a module that is not on a GPU")
    np.random.seed(2)
    with caplog.at_level(logging.INFO, logger="pdecontrol.surrogates"):
        value = update_surrogate(module, dm, fit, max_steps=2, min_steps=0, patience=1)
        value2 = update_surrogate(module, dm, fit, max_steps=1, min_steps=0, patience=1)
    assert sum("loop tier" in r.getMessage() for r in caplog.records) == 1
    assert isinstance(value, float) and math.isfinite(value) and value == fit.history[0]["Val. Loss"]
    assert (fit.global_step, fit.current_epoch, fit.tier) == (3, 2, "loop") and value2 == fit.history[1]["Val. Loss"]
    assert isinstance(fit.optimizers[0], torch.optim.Adam) and fit.optimizers[0].state
    assert any(not torch.equal(a, b) for a, b in zip(before, module.parameters()))
    for h in fit.history:
        assert all(math.isfinite(h[name]) for name in ("Val. Loss", "Val. Scaled Loss", "Val. Delta Loss"))
        assert h["hsteploss"].shape == (6,) and h["hsteploss"][0] == 0.0
        assert h["Val. Loss"] == pytest.approx(float(h["hsteploss"].mean()), rel=1e-5)


def test_a_cuda_module_without_the_training_modules_surface_lands_on_the_loop_tier():
    """Tier selection reads ``surrogate`` / ``_frozen_parameters`` / the captured step only where they exist: a module
    without them is a reason for the loop tier, not an AttributeError."""
    import types
    from pdecontrol.mbrl import surrogate_phase as sp
    bare = types.SimpleNamespace(device=torch.device("cuda", 0))
    assert sp._fused_step_ok(bare) is False
    tier, reason = sp._pick_tier(bare, types.SimpleNamespace())
    assert tier is None and "without the captured TBPTT step" in reason
