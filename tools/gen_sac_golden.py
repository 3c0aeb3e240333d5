#!/usr/bin/env python3
"""Golden vectors of the SAC agent -> tests/golden/sac_golden.npz (run in the build container).

Runs the reference's own ``SAC`` (pdecontrol/sac/sac.py) from the reference checkout, behind the stubs of
oracle/gen_golden.py plus an in-file ``wandb`` stub that records what the agent logs, through the scenario of
tests/_sac_models.py (the same function tests/test_sac_host.py drives this repository's class with), and records only
numbers.

Cases (tests/_sac_models.py CASES; Box(-1, 1, (1, 4)) actions, (1, 64) observations, one batch per case):
  h32        hidden 32, B = 16, three updates, automatic entropy tuning off
  h32_auto   the same with tuning on and target_update_interval = 2
  h256       hidden 256, B = 256, two updates

Keys per tag:
  <tag>_batch_<field>            the 7-tuple of ``update``
  <tag>_act_obs                  the observations ``select_action`` is called on, before and after the updates
  <tag>_action_before / _after   its outputs
  <tag>_u<k>_logged              what update k logged: Pol. Rew. Mean, SAC/Qloss, SAC/PolicyLoss, SAC/entropy_loss,
                                 SAC/alpha_loss (fp64 of the logged values)
  <tag>_u<k>_<net>.<param>       every parameter of critic, critic_target and policy after update k (k = 0: as built);
                                 for h256 ``..._sum`` (fp64 sum) and ``..._head`` (first 8 values) instead
  <tag>_u<k>_log_alpha           with tuning on

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_sac_golden.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True  # never write __pycache__ into the reference checkout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import gen_golden  # noqa: E402  (pins the CPU arithmetic before torch is imported)
import numpy as np  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "sac_golden.npz")
LOGS = []


def _install_wandb_stub():
    wandb = types.ModuleType("wandb")
    wandb.log = lambda entry, commit=True: LOGS.append((dict(entry), commit))
    sys.modules["wandb"] = wandb


def main():
    if not os.path.isdir(os.path.join(gen_golden.REF, "pdecontrol", "sac")):
        sys.exit(f"reference checkout not found at {gen_golden.REF}: the SAC fixtures can only be generated where it is")
    gen_golden._install_stubs()
    _install_wandb_stub()
    import _sac_models as sm
    from pdecontrol.sac.sac import SAC
    assert os.path.abspath(sys.modules[SAC.__module__].__file__).startswith(gen_golden.REF)
    fx = {}
    for tag in sm.CASES:
        fx.update(sm.scenario(tag, SAC, LOGS))
    assert all(np.asarray(v).dtype.kind in "fib" for v in fx.values())
    np.savez_compressed(OUT, **fx)
    print(f"{os.path.relpath(OUT, ROOT)}: {len(fx)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
