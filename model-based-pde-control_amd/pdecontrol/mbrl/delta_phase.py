"""The controller's ``update_delta_transform`` (reference pdecontrol/mbrl/mbrl.py:597-602) behind one call (DESIGN.md
4.16): the statistics of the scaled state changes ``(otransf(nxtobs) - otransf(obs)) / delta`` over ALL transitions of the
real replay, re-fitted into ``undscaling`` before every surrogate update.

Three tiers.  The kernel tier reads the slabs of a ``DeviceExperienceReplay`` in place: the table of live extents and the
connector's coefficients go up once, the row list is expanded from the table on the device (``device_rows``),
``rpd_moments`` (csrc/replay.hip) reduces the two fields it needs to per-column fp64 sums in two or three launches, one small
copy brings the batch statistics back, and ``Normalize.merge`` folds them in on the replay's device.  No tensor of
rows x columns elements is allocated.  The torch tier is the reference's expression over
``replay.transitions()`` for every other device replay, announced once per reason (``recognition.notice``); the host tier
is the reference's four lines on a host ``ExperienceReplay``.

``delta_rows_numpy`` and ``moments_numpy`` are the numpy twin that is the contract of the kernel.
"""
import itertools
import warnings
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
from pdecontrol.mbrl.recognition import Unrecognized, field_map, notice
from pdegym.common import transforms as tr


@dataclass
class DeltaUpdate:
    """What ``update_delta_transform`` did: the tier that ran ("kernel", "torch" or "host"), why not the kernel tier
    (None on it), the transitions the statistics were fitted on, and on the kernel tier the host copy of the kernel's
    ``stats`` (fp32 [2, obs_dim + 1]: mean and unbiased variance per column, the aggregate last)."""
    tier: str
    tier_reason: Optional[str]
    rows: int
    stats: Optional[np.ndarray] = None


# ----------------------------------------------------------------------------------------------------------------------
# the numpy twin
# ----------------------------------------------------------------------------------------------------------------------
def delta_rows_numpy(obs, nxtobs, fmap, delta):
    """``(otransf(nxtobs) - otransf(obs)) / delta`` of a recognised connector in numpy: ``FieldMap.apply_numpy`` on both
    fields, one fp32 subtraction and one fp32 division by ``np.float32(delta)`` (what torch's CPU ``tensor / float``
    divides by)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((fmap.apply_numpy(nxtobs) - fmap.apply_numpy(obs)) / np.float32(delta)).astype(np.float32)


def moments_numpy(deltas):
    """(sums, stats) of rows of scaled state changes ``[n, ..., D]`` in fp64, laid out as ``rpd_moments`` lays
    them out: ``sums`` [2, D + 1] holds sum d and sum d * d per column and over all columns last, ``stats`` [2, D + 1] the
    two-pass mean and the ``ddof=1`` variance (NaN below two values)."""
    d = np.asarray(deltas, dtype=np.float64)
    d = d.reshape(-1, d.shape[-1])
    sums = np.stack([np.append(d.sum(0), d.sum()), np.append((d * d).sum(0), (d * d).sum())])
    with warnings.catch_warnings(), np.errstate(invalid="ignore", divide="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        stats = np.stack([np.append(d.mean(0), d.mean()), np.append(d.var(0, ddof=1), d.var(ddof=1))])
    return sums, stats


# ----------------------------------------------------------------------------------------------------------------------
# tiers
# ----------------------------------------------------------------------------------------------------------------------
def device_rows(extents, device):
    """``_rows_of(extents)`` as an int64 tensor on ``device``, expanded there: what goes up is one [2, extents] table (the
    offset of each extent's first row against its position in the list, and the position its last row is followed by),
    not a row per transition; position p then belongs to the first extent that ends after p (DESIGN.md 4.16 has what the
    host expansion and its upload cost).  No synchronisation."""
    ext = np.fromiter(itertools.chain.from_iterable(extents), dtype=np.int64, count=2 * len(extents)).reshape(-1, 2)
    lengths = ext[:, 1]
    ends = np.cumsum(lengths)
    n = int(ends[-1]) if ends.size else 0
    table = torch.from_numpy(np.stack([ext[:, 0] - (ends - lengths), ends])).to(device)
    position = torch.arange(n, dtype=torch.int64, device=device)
    which = torch.searchsorted(table[1], position, right=True)
    return position.add_(table[0].index_select(0, which))


def _kernel_tier(replay, otransf, undscaling):
    """(the live extents in insertion order, the connector's ``FieldMap``) where the kernel tier applies, else raises
    ``Unrecognized``."""
    if type(undscaling) is not tr.Normalize:
        raise Unrecognized(f"a {type(undscaling).__name__} in place of the Normalize")
    if undscaling.frozen:
        raise Unrecognized("a frozen Normalize")
    if not undscaling.batched:
        raise Unrecognized("a Normalize that is not batched")
    if replay.tensors is None or replay.ntimesteps < 1:
        raise Unrecognized("a replay without rows")
    fmap = field_map(otransf, replay.obs_width)
    if replay.device.type != "cuda":                    # last: the reasons above are the same on every device
        raise Unrecognized("a replay that is not on a GPU")
    return [e for ep in replay._eps.values() for e in ep.extents], fmap


def _fit_kernel(replay, extents, fmap, undscaling, delta):
    import hipbind
    from pdecontrol.mbrl import replay_hip
    replay_hip.load()
    device, n, D = replay.device, int(replay.ntimesteps), int(fmap.width)
    obs, nxtobs = replay.tensors[0], replay.tensors[2]
    need = replay_hip.delta_workspace_doubles(D, n)
    if need < 1:
        raise Unrecognized(f"{D} observation columns (1 ... {replay_hip.MAX_OBS_DIM} are supported)")
    rows = device_rows(extents, device)
    assert rows.numel() == n, "the extents of the live episodes hold the live rows"
    coef = None if fmap.coef is None else fmap.coef.to(device)
    workspace = torch.empty(need, dtype=torch.float64, device=device)
    sums = torch.empty((2, D + 1), dtype=torch.float64, device=device)
    stats = torch.empty((2, D + 1), dtype=torch.float32, device=device)
    try:
        with torch.cuda.device(device):
            replay_hip.delta_moments(hipbind.stream(), obs, nxtobs, fmap.start, fmap.stride, coef, rows, n, delta, 0, workspace,
                                     sums, stats)
    except replay_hip.ReplayHipError as e:
        if e.code == replay_hip.DELTA_LAUNCH_FAILURE:
            raise
        raise Unrecognized(replay_hip.last_error()) from None       # refused on the host: nothing was enqueued
    host = stats.cpu().numpy()                                      # the phase's one synchronisation
    columns = slice(D, D + 1) if undscaling.aggregate else slice(0, D)
    undscaling.reset()
    undscaling.merge(stats[0, columns].reshape(1, 1, -1), stats[1, columns].reshape(1, 1, -1), n)
    return host


def _fit_reference(dataset, otransf, undscaling, delta):
    """The reference's lines, on whatever ``dataset`` holds (numpy arrays or device tensors)."""
    undscaling.reset()
    deltas = otransf(dataset.nxtobs) - otransf(dataset.obs)
    undscaling.update(deltas / delta)


def update_delta_transform(replay, otransf, undscaling, delta):
    """``undscaling.reset()`` and ``undscaling.update((otransf(nxtobs) - otransf(obs)) / delta)`` over all transitions of
    ``replay``; returns a ``DeltaUpdate``.

    ``replay``: the controller's real replay, ``otransf``: ``replay_to_world.otransf``, ``undscaling``: the ``Normalize``
    of the scaled state changes, ``delta``: ``cfg_steps * dt``.

    The kernel tier applies when the replay is a ``DeviceExperienceReplay`` on CUDA with rows, ``recognition.field_map``
    accepts ``otransf``, ``undscaling`` is a non-frozen ``Normalize`` with ``batched=True`` (aggregate, statistics of shape
    [1, 1, 1], or per column, [1, 1, obs_dim]) and ``rpd_moments`` does not refuse.  ``mean`` and ``var`` are then
    fp32 tensors on the replay's device, as the torch tier leaves them, and new objects, so graph caches that compare
    ``hipops.scaling_signature`` re-capture."""
    if not isinstance(replay, DeviceExperienceReplay):
        _fit_reference(replay.dataset(), otransf, undscaling, delta)
        return DeltaUpdate("host", None, int(replay.ntimesteps))
    try:
        extents, fmap = _kernel_tier(replay, otransf, undscaling)
        host = _fit_kernel(replay, extents, fmap, undscaling, delta)
        return DeltaUpdate("kernel", None, int(replay.ntimesteps), host)
    except Unrecognized as e:
        reason = str(e)
    notice("the delta statistics are fitted on the torch tier: %s", reason, expected=replay.device.type != "cuda")
    _fit_reference(replay.transitions(), otransf, undscaling, delta)
    return DeltaUpdate("torch", reason, int(replay.ntimesteps))
