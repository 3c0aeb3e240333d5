"""Numpy twin of the reward of ``ro_settle_dissipation`` (csrc/rollout.hip), shared by
tests/test_imagination_dissipation_host.py and tests/test_imagination_dissipation_gpu.py:

    r = (float)((-1.0) * ((sum u_xx^2 / N + sum u_x^2 / N) + sum u * phi / N))

with u the fp64 cast of the fp32-rescaled row, u_x (the upwind derivative of u^2) and u_xx from the env's ``rhs`` (the
C oracle behind ``OracleStepper``, the reference's operation order) and phi the fp32 fma chain of the scaled action."""
import numpy as np

from _rollout_scenario import fma_chain


def dissipation_terms(rows, raw_actions, geo, env):
    """(fp64 reward [n], mean_i(|u_i| * sum_k |a_k| F_ki) [n]) of ``rows`` [n, N] (world scale) and the raw agent
    ``raw_actions`` [n, A].  ``geo`` carries ``reward`` and ``act_in`` (``FieldMap``s) and ``forcing`` (fp32 [A, N]);
    the second value is the scale of the u * phi term that the tests' tolerances are written in."""
    F = np.ascontiguousarray(np.asarray(geo.forcing, dtype=np.float32))
    A, N = F.shape
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, N)
    w = geo.reward.apply_numpy(rows)
    a = geo.act_in.apply_numpy(np.asarray(raw_actions, dtype=np.float32).reshape(-1, A))
    phi = fma_chain(a, F)
    assert w.dtype == phi.dtype == np.float32 and w.shape == phi.shape
    u = w.astype(np.float64)
    with np.errstate(invalid="ignore"):
        _, (u_x, u_xx, _) = env.rhs(u, phi)
        reward = (-1.0) * (((u_xx * u_xx).sum(axis=1) / N + (u_x * u_x).sum(axis=1) / N) + (u * phi.astype(np.float64)).sum(axis=1) / N)
        scale = (np.abs(u) * (np.abs(a).astype(np.float64) @ np.abs(F).astype(np.float64))).mean(axis=1)
    return reward, scale


def dissipation_twin(rows, raw_actions, geo, env):
    """The kernel's fp32 reward of every row."""
    return dissipation_terms(rows, raw_actions, geo, env)[0].astype(np.float32)
