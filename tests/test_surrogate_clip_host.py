"""Gradient-norm clipping of the surrogate step without a GPU: every refusal of ``sur_flush_block_count``,
``sur_flush_all_grads_sumsq`` and ``sur_clip_adam_apply`` (include/surrogate_hip.h) through the loaded library -- each is
turned away on the host before any launch --, the block count of the synthetic layouts, ``update_surrogate``'s
``gradient_clip_val`` on the loop tier of a CPU module against a hand-written loop, and the controller's trainer key."""
import ctypes
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import _rollout_scenario as rsc
import _sur_tail_oracle as so
import _surrogate_phase_scenario as sc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _controller_scenario as cs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "model-based-pde-control_amd", "lib", "libsurrogate_hip.so")


# ----------------------------------------------------------------------------------------------------------------------
# the three entry points: refusals on the host
# ----------------------------------------------------------------------------------------------------------------------
class Args:
    """A complete, valid argument set of the two launches over host memory (nothing here is ever launched: every call
    made with it carries exactly one bad argument)."""

    def __init__(self):
        from pdecontrol.surrogates import hipops
        self.packs = [so.synthetic_pack(kind, so.layout(name, kind), 3, 4, "cpu")
                      for kind, name in (("enc", "odd"), ("enc", "tiny"), ("chunk", "wide"))]
        self.adam = [so.AdamState(p, 1e-3, 0.9, 0.999, 1e-8, "cpu") for p in self.packs]
        self.count = sum(so.flush_blocks(p.psize) for p in self.packs)
        self.sumsq = torch.zeros(self.count, dtype=torch.float64)
        self.norm = torch.zeros(1)
        self.clip = hipops.ClipParams(self.sumsq.data_ptr(), self.count, 0.5, self.norm.data_ptr())

    def pack_refs(self):
        return [p.ref() for p in self.packs]

    def adam_refs(self):
        return [a.ref() for a in self.adam]


def _lib():
    from pdecontrol.surrogates import hipops
    assert os.path.exists(LIB), "libsurrogate_hip.so not built (run __graft_entry__.build())"
    return hipops.load()


def _refused(rc, who):
    msg = _lib().sur_last_error().decode()
    assert rc < 0 and msg.startswith(who), (rc, msg)
    return msg


def _sumsq(a, packs=None, sumsq="own"):
    packs = a.pack_refs() if packs is None else packs
    return _lib().sur_flush_all_grads_sumsq(None, packs[0], packs[1], packs[2], a.sumsq.data_ptr() if sumsq == "own" else sumsq)


def _clip(a, packs=None, adam=None, clip="own"):
    packs = a.pack_refs() if packs is None else packs
    adam = a.adam_refs() if adam is None else adam
    return _lib().sur_clip_adam_apply(None, packs[0], adam[0], packs[1], adam[1], packs[2], adam[2],
                                      ctypes.byref(a.clip) if clip == "own" else clip)


@pytest.mark.parametrize("j", (0, 1, 2))
def test_a_null_pack_is_refused_by_all_three(j):
    a = Args()
    packs = a.pack_refs()
    packs[j] = None
    assert _lib().sur_flush_block_count(*packs) <= 0
    assert _lib().sur_last_error().decode().startswith("sur_flush_block_count")
    _refused(_sumsq(a, packs), "sur_flush_all_grads_sumsq")
    _refused(_clip(a, packs), "sur_clip_adam_apply")


@pytest.mark.parametrize("j", (0, 1, 2))
def test_the_reduction_refuses_a_null_partial_buffer_sumsq_and_gradient(j):
    who = "sur_flush_all_grads_sumsq"
    a = Args()
    a.packs[j].c.partial = None
    assert "partial" in _refused(_sumsq(a), who)
    a = Args()
    a.packs[j].c.g[so.nparam(a.packs[j].kind) - 1] = None
    assert "gradient" in _refused(_sumsq(a), who)
    assert "sumsq" in _refused(_sumsq(Args(), sumsq=None), who)


def test_clip_adam_refuses_a_null_clip_and_a_null_sumsq():
    who = "sur_clip_adam_apply"
    assert "clip" in _refused(_clip(Args(), clip=None), who)
    a = Args()
    a.clip.sumsq = None
    assert "sumsq" in _refused(_clip(a), who)


@pytest.mark.parametrize("j", (0, 1, 2))
def test_clip_adam_refuses_a_null_partial_buffer(j):
    a = Args()
    a.packs[j].c.partial = None
    assert "partial" in _refused(_clip(a), "sur_clip_adam_apply")


@pytest.mark.parametrize("bad", (lambda n: n - 1, lambda n: n + 1, lambda n: 0, lambda n: -n),
                         ids=("one short", "one over", "zero", "negative"))
def test_clip_adam_refuses_a_count_that_is_not_the_block_count(bad):
    a = Args()
    assert _lib().sur_flush_block_count(*a.pack_refs()) == a.count
    a.clip.count = bad(a.count)
    assert "count" in _refused(_clip(a), "sur_clip_adam_apply")


@pytest.mark.parametrize("max_norm", (0.0, -0.5, math.inf, -math.inf, math.nan))
def test_clip_adam_refuses_a_bound_that_is_not_finite_and_positive(max_norm):
    a = Args()
    a.clip.max_norm = max_norm
    assert "max_norm" in _refused(_clip(a), "sur_clip_adam_apply")


@pytest.mark.parametrize("field", ("m", "v", "step", "ticket", "lr"))
@pytest.mark.parametrize("j", (0, 1, 2))
def test_clip_adam_refuses_an_incomplete_descriptor(j, field):
    a = Args()
    setattr(a.adam[j].desc, field, None)
    assert f"descriptor {j}" in _refused(_clip(a), "sur_clip_adam_apply")


@pytest.mark.parametrize("j", (0, 1, 2))
def test_clip_adam_refuses_a_null_gradient_and_a_null_weight_under_a_descriptor(j):
    who = "sur_clip_adam_apply"
    a = Args()
    a.packs[j].c.g[0] = None
    assert "tensor 0" in _refused(_clip(a), who)
    a = Args()
    a.packs[j].c.w[1] = None
    assert "weight tensor 1" in _refused(_clip(a), who)
    # ... and the gradient is asked for without a descriptor too (the pack is still scaled)
    a = Args()
    a.packs[j].c.g[1] = None
    adam = a.adam_refs()
    adam[j] = None
    assert "gradient tensor 1" in _refused(_clip(a, adam=adam), who)


@pytest.mark.parametrize("names", [(x, y, z) for x in so.LAYOUTS for y in so.LAYOUTS for z in so.LAYOUTS])
def test_block_count_is_the_sum_of_the_packs_blocks(names):
    packs = [so.synthetic_pack(kind, so.layout(name, kind), 1, 2, "cpu") for kind, name in zip(("enc", "enc", "chunk"), names)]
    want = sum(-(-p.psize // 32) for p in packs)
    assert _lib().sur_flush_block_count(*(p.ref() for p in packs)) == want


# ----------------------------------------------------------------------------------------------------------------------
# update_surrogate, loop tier, CPU module
# ----------------------------------------------------------------------------------------------------------------------
STEPS = 3


@pytest.fixture(scope="module")
def scene():
    M = rsc.repo_namespace()
    env = M.Env()
    return M, env, rsc.transforms(M, env)


def _datamodule(scene):
    from pdecontrol.surrogates.common.datamodule import PDEDataModule
    M, env, tf = scene
    rp = sc.host_replay(M, sc.scripted_episodes(env.N))
    return PDEDataModule(data=rp.data, train=[0, 1, 2, 3], val=[4, 5], bootstrapping=True, stransf=tf.replay_to_world, tau=5,
                         batch_size=4)


def _module(scene):
    M, env, tf = scene
    return sc.training_module(M, env, tf, "cpu", seed=4)


def _seed():
    np.random.seed(2)
    torch.manual_seed(2)


def _phase(scene, **clip):
    from pdecontrol.mbrl.surrogate_phase import FitState, update_surrogate
    module, dm, fit = _module(scene), _datamodule(scene), FitState()
    _seed()
    update_surrogate(module, dm, fit, max_steps=STEPS, min_steps=0, patience=1, **clip)
    assert (fit.tier, fit.global_step) == ("loop", STEPS)
    return [p.detach().clone() for p in module.parameters()]


def _by_hand(scene, clip):
    """training_step -> zero_grad -> backward -> clip_grad_norm_ -> step over the first STEPS batches of the same loader;
    returns the parameters and every step's gradient norm before clipping."""
    module, dm = _module(scene), _datamodule(scene)
    _seed()
    dm.trainer = types.SimpleNamespace(current_epoch=0, global_step=0)
    loader = dm.train_dataloader()
    assert len(loader) > STEPS
    optimizers, _ = module.configure_optimizers()
    opt, norms = optimizers[0], []
    module.train()
    for bidx, batch in enumerate(loader):
        if bidx >= STEPS:
            break
        out = module.training_step(batch, bidx)
        opt.zero_grad(set_to_none=True)
        out["loss"].backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(module.surrogate.parameters(), math.inf if clip is None else clip)))
        opt.step()
    return [p.detach().clone() for p in module.parameters()], norms


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_the_loop_tier_clips_as_a_hand_written_loop_does(scene):
    plain, norms = _by_hand(scene, None)
    assert all(math.isfinite(n) and n > 0 for n in norms)
    clip = 0.25 * norms[0]                       # below the first step's norm: that step is clipped for certain
    want, clipped_norms = _by_hand(scene, clip)
    assert clipped_norms[0] == norms[0] > clip
    print("gradient norms before clipping:", norms, "clipped run:", clipped_norms, "bound:", clip)
    today = _phase(scene)
    assert _same(today, plain), "the unclipped phase is not the hand-written loop"
    got = _phase(scene, gradient_clip_val=clip)
    assert _same(got, want), "the clipped phase is not the hand-written clipped loop"
    assert not _same(got, today), "clipping changed nothing: Adam's first update is scale-free, later ones are not"
    assert _same(_phase(scene, gradient_clip_val=None), today)
    assert _same(_phase(scene, gradient_clip_val=0), today)
    assert _same(_phase(scene, gradient_clip_val=0.0), today)


# ----------------------------------------------------------------------------------------------------------------------
# the controller
# ----------------------------------------------------------------------------------------------------------------------
def _controller(tmp_path, monkeypatch, **trainer_keys):
    from pdecontrol.mbrl import mbrl
    config = cs.toy_config()
    for phase in ("initial", "iterations"):
        config.trainer[phase].update(trainer_keys)
    c = cs.build(tmp_path, config=config)
    c.replay = types.SimpleNamespace(episodes=[0, 1, 2, 3], data=("data", "replay"))
    calls = []

    def spy(module, datamodule, fit, **kwargs):
        fit.tier = "stub"
        calls.append(kwargs)
        return 0.25

    monkeypatch.setattr(mbrl, "update_surrogate", spy)
    monkeypatch.setattr(mbrl, "split_episodes", lambda items, test_size: ([0, 1, 2], [3]))
    return c, calls


def test_the_controller_hands_the_trainers_clip_value_to_the_phase(tmp_path, monkeypatch):
    c, calls = _controller(tmp_path / "a", monkeypatch, gradient_clip_val=0.5, gradient_clip_algorithm="norm")
    assert c.update_surrogate(c.modules[0], c.trainers[0]) == 0.25
    assert calls[0]["gradient_clip_val"] == 0.5 and calls[0]["max_steps"] == 2
    c, calls = _controller(tmp_path / "b", monkeypatch)
    c.update_surrogate(c.modules[0], c.trainers[0])
    assert calls[0].get("gradient_clip_val") is None            # no key: the call as it has always been


def test_the_controller_refuses_value_clipping(tmp_path, monkeypatch):
    c, calls = _controller(tmp_path, monkeypatch, gradient_clip_val=0.5, gradient_clip_algorithm="value")
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        c.update_surrogate(c.modules[0], c.trainers[0])
    assert not calls


# ----------------------------------------------------------------------------------------------------------------------
# the Trainer shim
# ----------------------------------------------------------------------------------------------------------------------
def test_the_shim_trainer_leaves_its_clip_value_for_a_module_under_manual_optimization():
    from pdecontrol._compat.lightning import IS_SHIM, pl
    if not IS_SHIM:
        pytest.skip("pytorch-lightning is installed: its Trainer is not the shim")

    class Tiny(pl.LightningModule):
        def __init__(self, manual):
            super().__init__()
            self.automatic_optimization = not manual
            self.w = torch.nn.Parameter(torch.ones(2))
            self.norms = []

        def training_step(self, batch, bidx):
            return {"loss": (self.w * batch).sum()}

        def configure_optimizers(self):
            opt = torch.optim.SGD([self.w], lr=0.0)
            return [opt], [{"scheduler": torch.optim.lr_scheduler.StepLR(opt, step_size=1)}]

    data = [torch.tensor([3.0, 4.0])]
    manual = Tiny(True)
    pl.Trainer(max_steps=1, gradient_clip_val=0.5).fit(manual, train_dataloaders=data)
    assert manual.__dict__["_trainer_gradient_clip_val"] == 0.5
    manual = Tiny(True)
    pl.Trainer(max_steps=1).fit(manual, train_dataloaders=data)
    assert manual.__dict__["_trainer_gradient_clip_val"] is None
    auto = Tiny(False)                            # the automatic branch clips by itself, as before, and leaves nothing
    pl.Trainer(max_steps=1, gradient_clip_val=0.5).fit(auto, train_dataloaders=data)
    assert "_trainer_gradient_clip_val" not in auto.__dict__
    assert float(torch.linalg.vector_norm(auto.w.grad)) == pytest.approx(0.5, rel=1e-5)
