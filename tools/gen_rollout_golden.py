#!/usr/bin/env python3
"""Golden arrays of the imagined-rollout phase -> tests/golden/rollout_golden.npz (run in the build container).

Runs the scenario of tests/_rollout_scenario.py on the reference's own ``Worker`` (pdecontrol/mbrl/worker.py), vector
wrappers, ``WorldVecEnv``, ensemble and ``SAC`` from the reference checkout, on the CPU, behind the stubs of
oracle/gen_golden.py (gym comes from this repository's shim, ``wandb`` and ``pdecontrol.visualize`` are empty modules), and
records only numbers: per pass ("free": two rounds of three steps; "limit": the env limit cuts every round after one step)
the episode keys, ``ntimesteps``, ``nstopped`` and every field of every episode of the returned ``ExperienceReplay``.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_rollout_golden.py
"""
import importlib.util
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the reference checkout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gen_golden  # noqa: E402  (pins the CPU arithmetic before torch is imported)
import numpy as np  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rollout_golden.npz")


def _install_gym_shim():
    """gym.vector / gym.spaces from this repository's shim, so that both sets of wrappers sit on the same base classes."""
    spec = importlib.util.spec_from_file_location(
        "_gym_shim_for_ref", os.path.join(ROOT, "model-based-pde-control_amd", "pdegym", "_compat", "gym_shim.py"))
    shim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(shim)
    gym = sys.modules["gym"]
    gym.vector = types.ModuleType("gym.vector")
    gym.vector.VectorEnv, gym.vector.VectorEnvWrapper = shim.VectorEnv, shim.VectorEnvWrapper
    utils, spaces = types.ModuleType("gym.vector.utils"), types.ModuleType("gym.vector.utils.spaces")
    spaces.batch_space = shim.batch_space
    utils.spaces = spaces
    gym.vector.utils = utils
    gym.spaces.Box = shim.Box
    sys.modules.update({"gym.vector": gym.vector, "gym.vector.utils": utils, "gym.vector.utils.spaces": spaces})
    if not hasattr(np, "bool8"):
        np.bool8 = np.bool_


def main():
    if not os.path.isfile(os.path.join(gen_golden.REF, "pdecontrol", "mbrl", "worker.py")):
        sys.exit(f"reference checkout not found at {gen_golden.REF}: the rollout fixture can only be generated where it is")
    gen_golden._install_stubs()
    _install_gym_shim()
    wandb = types.ModuleType("wandb")
    wandb.log = lambda *a, **k: None
    sys.modules["wandb"] = wandb
    sys.modules["pdecontrol.visualize"] = types.ModuleType("pdecontrol.visualize")
    ks = gen_golden._load("pdegym.kuramoto.kuramoto", "pdegym/kuramoto/kuramoto.py")
    W = gen_golden._load("pdegym.common.vec_wrappers", "pdegym/common/vec_wrappers.py")
    import _rollout_scenario as sc
    import _sac_models as sm
    import pdecontrol.mbrl.replay as replay
    import pdecontrol.surrogates.common.dataset as ds
    import pdegym.common.transforms as T
    from pdecontrol.architectures.autoreg import KSAutoRegConvolutionalLSTM
    from pdecontrol.mbrl.types import Sample
    from pdecontrol.mbrl.worker import PDEEnvStack, Worker
    from pdecontrol.mbrl.world.world import WorldVecEnv
    from pdecontrol.sac.sac import SAC
    from pdecontrol.surrogates.surrogate import PDEEnsemble
    from pdecontrol.surrogates.training import PDETrainingModule
    for cls in (Worker, WorldVecEnv, SAC, PDEEnsemble, T.ScaleTransform, W.StoreNObsVecWrapper):
        assert os.path.abspath(sys.modules[cls.__module__].__file__).startswith(gen_golden.REF), cls
    M = types.SimpleNamespace(Env=ks.KuramotoSivashinskyEnv, T=T, W=W, Replay=replay.ExperienceReplay, ds=ds, Sample=Sample,
                              factory_cls=KSAutoRegConvolutionalLSTM, factory_n_cls=None, TrainingModule=PDETrainingModule,
                              Ensemble=PDEEnsemble, WorldVecEnv=WorldVecEnv, Worker=Worker, PDEEnvStack=PDEEnvStack, SAC=SAC,
                              sac_config=sm.config, sac_spaces=sm.spaces)
    fx = sc.run(M)
    assert all(np.asarray(v).dtype.kind in "fib" for v in fx.values())
    np.savez_compressed(OUT, **fx)
    print(f"{os.path.relpath(OUT, ROOT)}: {len(fx)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
