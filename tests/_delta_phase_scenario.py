"""Shared pieces of the delta-phase tests (tests/test_delta_phase_host.py, tests/test_delta_phase_gpu.py): the connectors
whose ``otransf`` the phase is given, a ``DeviceExperienceReplay`` with fragmented extents, slab pairs whose scaled state
changes have a chosen mean and spread, and the comparison in units in the last place."""
import numpy as np
import torch

from _policy_phase_scenario import scripted_replay
from pdecontrol.mbrl.device_replay import DeviceExperienceReplay, _rows_of
from pdegym.common.transforms import BatchTransform, ScaleTransform, SensorTransform, SampleTransform

CONNECTORS = ("controller", "stride2", "unscaled")
# (mean, std) of the scaled state changes the moment tests draw: |mean| / std <= 100
MOMENTS = ((0.3, 2.0), (5.0, 0.05), (100.0, 1.0), (-3.0, 7.0), (0.01, 30.0))


def otransf(kind, width, seed=0):
    """``replay_to_world.otransf`` of a controller: "controller" is mbrl.py:183's ``[oscaling, world_sensor]`` (running
    extrema aggregated to scalars, stride 1), "stride2" one bound per column read through a sensor of stride 2,
    "unscaled" the sensor alone."""
    rs = np.random.RandomState(seed + 900)
    if kind == "controller":
        oscaling = ScaleTransform(batched=True, aggregate=True, frozen=False)
        oscaling.update(rs.randn(16, 1, width).astype(np.float32) * 1.7)
        chain = [oscaling, BatchTransform(SensorTransform(stride=1))]
    elif kind == "stride2":
        lo = -3.0 - rs.uniform(0, 1, (1, 1, width)).astype(np.float32)
        hi = 3.0 + rs.uniform(0, 1, (1, 1, width)).astype(np.float32)
        chain = [ScaleTransform(bounds=(lo, hi), aggregate=False, batched=True, frozen=True), BatchTransform(SensorTransform(stride=2))]
    else:
        chain = [BatchTransform(SensorTransform(stride=1))]
    return SampleTransform(otransf=chain).otransf


def reference_deltas(chain, obs, nxtobs, delta):
    """The reference's expression (mbrl.py:600-602) on whatever it is given."""
    return (chain(nxtobs) - chain(obs)) / delta


def fragmented_replay(device, width=12, act_dim=2, seed=0):
    """A ``DeviceExperienceReplay`` filled through ``extend``; a ``resize`` in between evicted episodes, so later episodes
    took the freed extents and the live rows are neither sorted nor contiguous.  Free rows are NaN-filled."""
    sink = DeviceExperienceReplay(device=device, rows=80)
    sink.extend(scripted_replay(width, act_dim, seed + 1, 14, {0: (5, 12), 1: (8,), 2: (3, 4)}))      # 42 rows
    sink.resize(25)
    sink.resize(np.inf)
    sink.extend(scripted_replay(width, act_dim, seed + 2, 9, {0: (4,), 1: (9,), 2: (2, 7)}))          # 27 rows
    sink.extend(scripted_replay(width, act_dim, seed + 3, 5, {0: (5,), 1: (2,)}))                     # 10 rows
    live = live_rows(sink)
    dead = np.setdiff1d(np.arange(sink.rows), live)
    assert dead.size and np.any(np.diff(live) != 1) and np.any(np.diff(live) < 0), "the scenario is meant to be fragmented"
    for field in (0, 2):
        sink.tensors[field][torch.from_numpy(dead).to(sink.device)] = float("nan")
    return sink


def live_rows(sink):
    return _rows_of([e for ep in sink._eps.values() for e in ep.extents])


def slab_pair(rs, rows, width, live, start, stride, coef, delta, mean, std):
    """fp32 ``obs`` and ``nxtobs`` [rows, width], NaN outside the ``live`` rows, drawn so that the scaled state changes
    of the sensor's columns have about this mean and spread under the coefficients ``coef`` ([4, obs_dim] numpy or None)."""
    obs = np.full((rows, width), np.nan, dtype=np.float32)
    nxt = np.full((rows, width), np.nan, dtype=np.float32)
    n = len(live)
    obs[live] = rs.uniform(-1, 1, (n, width)).astype(np.float32)
    change = delta * (mean + std * rs.randn(n, width))
    if coef is not None:                              # the affine map has slope (d - c) / (b - a) per output column
        slope = np.ones(width)
        cols = start + stride * np.arange(coef.shape[1])
        slope[cols] = coef[2] / coef[1]
        change = change / slope
    nxt[live] = (obs[live] + change).astype(np.float32)
    return obs, nxt


def ulps(got, want):
    """Distance in representable fp32 values, elementwise; NaN against NaN is 0, NaN against a number is huge."""
    got, want = np.asarray(got, dtype=np.float32).reshape(-1), np.asarray(want, dtype=np.float32).reshape(-1)
    key = lambda v: np.where(v.view(np.int32) < 0, np.int64(-2 ** 31) - v.view(np.int32).astype(np.int64), v.view(np.int32).astype(np.int64))
    out = np.abs(key(got) - key(want))
    both, one = np.isnan(got) & np.isnan(want), np.isnan(got) ^ np.isnan(want)
    return np.where(both, 0, np.where(one, np.int64(2) ** 40, out))
