#!/usr/bin/env python3
"""Golden vectors of the Burgers physics-informed loss -> tests/golden/phyloss_golden.npz (run in the build container).

Runs the reference's own ``BurgersPhyPDELoss`` (pdecontrol/surrogates/phyloss/phyloss.py:13-89) from the reference
checkout, behind the stubs of oracle/gen_golden.py, on seeded smooth fields, and records only numbers (fp32).

Cases (tag: N, B, T, dx, dt, nu):
  n512   512, 2, 6   the Burgers env's defaults (dx = 2 pi / 512, dt = 1e-3, nu = 0.01)
  n128   128, 4, 6   dx = 2 pi / 128, dt = 2e-3, nu = 0.05 (the second configuration of burgers_golden.npz)
  t1     128, 2, 1   a single time slice: slot 0 is compared with itself
  t2     128, 2, 2   two slices: slot 0 against slice 1, slot 1 against the evolved slice 0

Keys per tag:
  <tag>_params      [dx, dt, nu] fp64
  <tag>_u           the input [B, T, 1, N]: sums of four sines with seeded amplitudes and phases
  <tag>_loss_none   ``BurgersPhyPDELoss(dx, dt, nu, reduction="none")(u)``
  <tag>_loss_mean   the same with ``reduction="mean"`` (a scalar)
  <tag>_weights     seeded uniform(-1, 1) weights of the element-wise loss
  <tag>_grad        d sum(weights * loss_none) / d u

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_phyloss_golden.py
"""
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference checkout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import gen_golden  # noqa: E402  (pins the CPU arithmetic before torch is imported)
import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "phyloss_golden.npz")
CASES = (("n512", 512, 2, 6, 1e-3, 0.01, 31), ("n128", 128, 4, 6, 2e-3, 0.05, 32),
         ("t1", 128, 2, 1, 2e-3, 0.05, 33), ("t2", 128, 2, 2, 2e-3, 0.05, 34))


def smooth_fields(B, T, N, seed):
    """[B, T, 1, N] fp32: per (b, t) a sum of four sines, amplitudes uniform(-1, 1), phases uniform(0, 6)."""
    rs = np.random.RandomState(seed)
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    rows = [sum(rs.uniform(-1, 1) * np.sin((k + 1) * x + rs.uniform(0, 6)) for k in range(4)) for _ in range(B * T)]
    return np.stack(rows).astype(np.float32).reshape(B, T, 1, N)


def fixtures():
    import pdecontrol.surrogates.phyloss.phyloss as phy
    out = {}
    for tag, N, B, T, dt, nu, seed in CASES:
        dx = 2 * np.pi / N
        u = torch.from_numpy(smooth_fields(B, T, N, seed)).requires_grad_(True)
        weights = torch.from_numpy(np.random.RandomState(seed + 100).uniform(-1, 1, (B, T, 1, N)).astype(np.float32))
        loss = phy.BurgersPhyPDELoss(dx=dx, dt=dt, nu=nu, reduction="none")(u)
        (weights * loss).sum().backward()
        with torch.no_grad():
            mean = phy.BurgersPhyPDELoss(dx=dx, dt=dt, nu=nu, reduction="mean")(u)
        out[f"{tag}_params"] = np.asarray([dx, dt, nu], dtype=np.float64)
        out[f"{tag}_u"] = u.detach().numpy().copy()
        out[f"{tag}_loss_none"] = loss.detach().numpy().copy()
        out[f"{tag}_loss_mean"] = mean.numpy().copy()
        out[f"{tag}_weights"] = weights.numpy().copy()
        out[f"{tag}_grad"] = u.grad.numpy().copy()
    return out


def main():
    if not os.path.isdir(os.path.join(gen_golden.REF, "pdecontrol")):
        sys.exit(f"reference checkout not found at {gen_golden.REF}: the physics-loss fixtures can only be generated where it is")
    gen_golden._install_stubs()
    fx = fixtures()
    assert all(np.asarray(v).dtype.kind in "fib" for v in fx.values())
    np.savez_compressed(OUT, **fx)
    print(f"{os.path.relpath(OUT, ROOT)}: {len(fx)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
