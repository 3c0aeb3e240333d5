"""The delta-statistics phase on the GPU: ``rpd_moments`` against its numpy twin over row counts,
widths, sensors, coefficients, row lists, group counts and alignments; dead rows are not read; the kernel tier of
``update_delta_transform`` on a fragmented ``DeviceExperienceReplay``; the memory condition.

Bounds.  ``stats`` is the fp32 rounding of an fp64 value that differs from the twin's two-pass value by about 1e-10
relative at the most (sum and sum of squares with |mean| / std <= 100 lose at most four of sixteen digits), so it is the
twin's fp32 value or a neighbour of it: at most 1 ulp.  ``sums`` equals the twin's fp64 sums to 1e-12 of the twin's own
value, per column and for the totals.  An fp64 sum of n terms carries an error of a few 1e-16 of the sum of their
MAGNITUDES, so that bound can hold only where a column's changes do not cancel to below about 1e-4 of their magnitudes;
the seeds are fixed and every case asserts, before anything runs, that none of its columns cancels below 1e-3
(``Case.cancellation``), so a failure of the bound is the kernel's."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _delta_phase_scenario as sc  # noqa: E402

pytestmark = pytest.mark.gpu

SENSORS = ((0, 1), (1, 2), (4, 1))
COEFS = ("none", "scalar", "columns")
ROWS = ("packed", "permuted")
GROUPS = (1, 2, 3, 0)
OFFSETS = (0, 1)                    # floats the slabs' bases are moved by: 1 breaks the 16-byte alignment
NS, WIDTHS = (1, 3, 257, 4099), (64, 98, 256, 1024)
DELTA = 0.15


def _modules():
    import hipbind
    from pdecontrol.mbrl import delta_phase, replay_hip
    replay_hip.load()
    return hipbind, replay_hip, delta_phase


def _coef(rs, kind, obs_dim):
    if kind == "none":
        return None
    u = rs.uniform(0, 1, obs_dim if kind == "columns" else 1).astype(np.float32) * np.ones(obs_dim, dtype=np.float32)
    a = (-3.0 - u).astype(np.float32)
    return np.stack([a, (3.0 + u) - a, np.full(obs_dim, 2.0, np.float32), np.full(obs_dim, -1.0, np.float32)]).astype(np.float32)


def host_case(n, width, sensor, coef, rows, moments, seed, delta=DELTA):
    """The host side of a case: slabs with NaN in every dead row, the live rows, the coefficients and the twin's rows of
    scaled state changes."""
    from pdecontrol.mbrl.delta_phase import delta_rows_numpy
    from pdecontrol.mbrl.recognition import FieldMap
    rs = np.random.RandomState(seed)
    start, stride = sensor
    obs_dim = len(range(start, width, stride))
    total = n + 37
    live = np.arange(n) if rows == "packed" else rs.permutation(total)[:n].astype(np.int64)
    coef_host = _coef(rs, coef, obs_dim)
    obs, nxt = sc.slab_pair(rs, total, width, live, start, stride, coef_host, delta, *moments)
    fmap = FieldMap(start, stride, obs_dim, None if coef_host is None else torch.from_numpy(coef_host))
    return obs, nxt, live, coef_host, delta_rows_numpy(obs[live], nxt[live], fmap, delta)


def cancellation(deltas):
    """The smallest |sum d| / sum |d| over the columns and over all of them: how far the changes of a column cancel."""
    d = np.asarray(deltas, dtype=np.float64).reshape(-1, deltas.shape[-1])
    ratio = np.append(np.abs(d.sum(0)) / np.abs(d).sum(0), abs(d.sum()) / np.abs(d).sum())
    return float(ratio.min())


class Case:
    """Slabs on the device with NaN in every dead row, the row list, and the twin's fp64 sums and statistics."""

    def __init__(self, n, width, sensor, coef, rows, offset, moments, seed, delta=DELTA):
        from pdecontrol.mbrl.delta_phase import moments_numpy
        dev = torch.device("cuda", 0)
        self.n, self.width, (self.start, self.stride), self.delta = n, width, sensor, delta
        self.obs_dim = len(range(self.start, width, self.stride))
        obs, nxt, live, coef_host, self.deltas = host_case(n, width, sensor, coef, rows, moments, seed, delta)
        self.cancellation = cancellation(self.deltas)
        assert self.cancellation >= 1e-3, ("a column of this case cancels too far for the bound on the sums", self.cancellation)
        self.sums, self.stats = moments_numpy(self.deltas)
        place = lambda a: self._place(a, offset, dev)
        self.obs, self.nxt = place(obs), place(nxt)
        self.coef = None if coef_host is None else torch.from_numpy(coef_host).to(dev)
        self.live = live
        self.rows = None if rows == "packed" else torch.from_numpy(live).to(dev)
        self.dev = dev

    @staticmethod
    def _place(a, offset, dev):
        flat = torch.empty(a.size + 4, dtype=torch.float32, device=dev)
        view = flat[offset:offset + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 16 == 4 * offset
        return view

    def run(self, groups, rows=None):
        hipbind, replay_hip, _ = _modules()
        rows = self.rows if rows is None else rows
        need = replay_hip.delta_workspace_doubles(self.obs_dim, self.n, groups)
        assert need >= 2 * self.obs_dim
        ws = torch.full((need,), float("nan"), dtype=torch.float64, device=self.dev)
        sums = torch.full((2, self.obs_dim + 1), float("nan"), dtype=torch.float64, device=self.dev)
        stats = torch.full((2, self.obs_dim + 1), float("nan"), dtype=torch.float32, device=self.dev)
        replay_hip.delta_moments(hipbind.stream(), self.obs, self.nxt, self.start, self.stride, self.coef, rows, self.n, self.delta,
                                 groups, ws, sums, stats)
        return sums.cpu().numpy(), stats.cpu().numpy()

    def check(self, sums, stats, what):
        err = np.abs(sums - self.sums)
        assert np.all(err <= 1e-12 * np.abs(self.sums)), (what, "sums", float(np.max(err / np.abs(self.sums))))
        d = sc.ulps(stats, self.stats.astype(np.float32))
        assert d.max() <= 1, (what, "stats", int(d.max()), stats.reshape(-1)[d.argmax()], self.stats.reshape(-1)[d.argmax()])
        return int(d.max())


def _moments(n, i):
    """The i-th (mean, std) pair of a case of n rows.  The bound on the sums is relative to the sum itself, which no fp64
    sum meets where a column's changes cancel below about 1e-4 of their magnitudes, so a case draws only pairs under which
    that is rare (``Case`` then asserts it did not happen): all but (0.01, 30) from four rows on, and at n <= 3, where
    three terms of either sign cancel easily, the two pairs with |mean| / std = 100.
    ``test_stats_where_the_mean_is_lost_in_the_spread`` covers (0.01, 30) at n = 4099."""
    pairs = sc.MOMENTS[1:3] if n <= 3 else sc.MOMENTS[:4]
    return pairs[i % len(pairs)]


CROSS_SEED = 200                    # a base under which no column of the 72 cases cancels below 1e-3


def _rotation():
    """Every (n, width) once; the other axes rotate with the index, each at its own period."""
    for i, (n, width) in enumerate(itertools.product(NS, WIDTHS)):
        moments = (0.0, 1.0) if n == 1 else _moments(n, i)
        yield pytest.param(n, width, SENSORS[i % 3], COEFS[(i // 3 + i) % 3], ROWS[i % 2], GROUPS[(i // 2 + i) % 4], OFFSETS[(i // 4) % 2],
                           moments, i, id=f"n{n}-N{width}")


@pytest.mark.parametrize("n,width,sensor,coef,rows,groups,offset,moments,seed", list(_rotation()))
def test_moments_against_the_twin(n, width, sensor, coef, rows, groups, offset, moments, seed):
    case = Case(n, width, sensor, coef, rows, offset, moments, seed)
    sums, stats = case.run(groups)
    worst = case.check(sums, stats, (sensor, coef, rows, groups, offset))
    again = case.run(groups)
    assert again[0].tobytes() == sums.tobytes() and again[1].tobytes() == stats.tobytes(), "two runs differ"
    assert np.isnan(stats[1, :case.obs_dim]).all() == (n == 1)
    print(f"n={n} N={width} sensor={sensor} coef={coef} rows={rows} groups={groups} offset={offset}: stats within {worst} ulp")


@pytest.mark.parametrize("n,width", [(257, 256), (3, 98)])
def test_moments_in_full_cross(n, width):
    """Every sensor x coefficients x row list x alignment x group count at a width that takes float4 loads (more than 192
    columns, where stride, start and alignment allow) and at one that keeps a lane per column; the
    group counts of one combination agree with each other within the 1-ulp rule and each is repeatable."""
    worst = 0
    for i, (sensor, coef, rows, offset) in enumerate(itertools.product(SENSORS, COEFS, ROWS, OFFSETS)):
        case = Case(n, width, sensor, coef, rows, offset, _moments(n, i), CROSS_SEED + i)
        first = None
        for groups in GROUPS:
            sums, stats = case.run(groups)
            worst = max(worst, case.check(sums, stats, (sensor, coef, rows, offset, groups)))
            again = case.run(groups)
            assert again[0].tobytes() == sums.tobytes() and again[1].tobytes() == stats.tobytes(), "two runs differ"
            if first is None:
                first = stats
            assert sc.ulps(stats, first).max() <= 1, (sensor, coef, rows, offset, groups)
    print(f"n={n} N={width}: 36 combinations x 4 group counts, stats within {worst} ulp of the twin")


def test_stats_where_the_mean_is_lost_in_the_spread():
    """(mean, std) = (0.01, 30) at n = 4099, N = 256: ``stats`` within 1 ulp in every column, sum d * d to 1e-12 of itself
    in every column, and sum d to 1e-12 of itself in every column that does not cancel below 1e-3 of its magnitudes (the
    others are counted and their ratios logged: there the twin's own fp64 sum is no better than the bound)."""
    from pdecontrol.mbrl.delta_phase import moments_numpy
    hipbind, replay_hip, _ = _modules()
    dev = torch.device("cuda", 0)
    n, width = 4099, 256
    obs, nxt, live, _, deltas = host_case(n, width, (0, 1), "none", "permuted", (0.01, 30.0), 5)
    want_sums, want_stats = moments_numpy(deltas)
    d64 = deltas.astype(np.float64).reshape(n, width)
    ratio = np.append(np.abs(d64.sum(0)) / np.abs(d64).sum(0), abs(d64.sum()) / np.abs(d64).sum())
    ws = torch.empty(replay_hip.delta_workspace_doubles(width, n), dtype=torch.float64, device=dev)
    sums = torch.empty((2, width + 1), dtype=torch.float64, device=dev)
    stats = torch.empty((2, width + 1), dtype=torch.float32, device=dev)
    replay_hip.delta_moments(hipbind.stream(), torch.from_numpy(obs).to(dev), torch.from_numpy(nxt).to(dev), 0, 1, None,
                             torch.from_numpy(live).to(dev), n, DELTA, 0, ws, sums, stats)
    sums, stats = sums.cpu().numpy(), stats.cpu().numpy()
    rel = np.abs(sums - want_sums) / np.abs(want_sums)
    kept = ratio >= 1e-3
    print(f"(0.01, 30) at n={n} N={width}: {int((~kept).sum())} of {width + 1} sums of d cancel below 1e-3 (ratios "
          f"{np.sort(ratio[~kept])[:4]}), their relative distance to the twin up to {rel[0][~kept].max() if (~kept).any() else 0:.2e}; "
          f"the others up to {rel[0][kept].max():.2e}, sums of d * d up to {rel[1].max():.2e}")
    assert kept.sum() > width // 2 and np.all(rel[0][kept] <= 1e-12) and np.all(rel[1] <= 1e-12)
    assert sc.ulps(stats, want_stats.astype(np.float32)).max() <= 1


def test_one_row_of_one_column_has_no_variance():
    case = Case(1, 64, (63, 1), "scalar", "permuted", 0, (0.0, 1.0), 7)
    assert case.obs_dim == 1
    sums, stats = case.run(0)
    case.check(sums, stats, "1 x 1")
    assert np.isnan(stats[1]).all() and np.isfinite(stats[0]).all() and stats[0, 0] == stats[0, 1] == case.deltas[0, 0]


def test_dead_rows_are_not_read():
    """The slabs hold 37 rows more than are live and those are NaN: the statistics are finite, and the same as with
    numbers in the dead rows.  One row entry outside the slab makes every statistic NaN, whichever side it is on."""
    case = Case(257, 98, (1, 2), "columns", "permuted", 0, (0.3, 2.0), 21)
    sums, stats = case.run(3)
    assert np.isfinite(sums).all() and np.isfinite(stats).all()
    dead = torch.from_numpy(np.setdiff1d(np.arange(257 + 37), case.live)).to(case.dev)
    assert torch.isnan(case.obs[dead]).all() and torch.isnan(case.nxt[dead]).all()
    case.obs[dead] = 1e6
    case.nxt[dead] = -1e6
    other = case.run(3)
    assert other[0].tobytes() == sums.tobytes() and other[1].tobytes() == stats.tobytes()
    for bad in (257 + 37, -1):
        rows = case.rows.clone()
        rows[100] = bad
        sums, stats = case.run(3, rows=rows)
        assert np.isnan(sums).all() and np.isnan(stats).all(), bad


# ----------------------------------------------------------------------------------------------------------------------
# the phase
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0.25, 0.15])
@pytest.mark.parametrize("aggregate", [True, False])
def test_the_kernel_tier_on_a_fragmented_replay(aggregate, delta):
    from types import SimpleNamespace
    from pdecontrol.mbrl.recognition import field_map
    from pdecontrol.surrogates import hipops
    from pdegym.common.transforms import BatchTransform, Normalize
    hipbind, replay_hip, dp = _modules()
    dev = torch.device("cuda", 0)
    sink = sc.fragmented_replay(dev)
    chain = sc.otransf("controller", sink.obs_width)
    live, D = sc.live_rows(sink), sink.obs_width
    n = live.size
    extents = [e for ep in sink._eps.values() for e in ep.extents]
    assert np.array_equal(dp.device_rows(extents, dev).cpu().numpy(), live)
    norm = Normalize(aggregate=aggregate, batched=True)
    norm.update(torch.ones(3, 1, D, device=dev))
    signature = hipops.scaling_signature(SimpleNamespace(dscaling=None), BatchTransform(norm))
    record = dp.update_delta_transform(sink, chain, norm, delta)
    assert (record.tier, record.tier_reason, record.rows) == ("kernel", None, n) and norm.count == n == sink.ntimesteps
    assert not hipops.same_signature(signature, hipops.scaling_signature(SimpleNamespace(dscaling=None), BatchTransform(norm)))

    # shape, dtype and device of the torch tier
    torch_norm = Normalize(aggregate=aggregate, batched=True)
    dp._fit_reference(sink.transitions(), chain, torch_norm, delta)
    for got, want in ((norm.mean, torch_norm.mean), (norm.var, torch_norm.var)):
        assert got.shape == want.shape == ((1, 1, 1) if aggregate else (1, 1, D))
        assert got.dtype == want.dtype == torch.float32 and got.device == want.device == dev

    # Normalize.merge of the kernel's own stats on that device, bit for bit
    fmap = field_map(chain, D)
    ws = torch.empty(replay_hip.delta_workspace_doubles(D, n), dtype=torch.float64, device=dev)
    sums = torch.empty((2, D + 1), dtype=torch.float64, device=dev)
    stats = torch.empty((2, D + 1), dtype=torch.float32, device=dev)
    replay_hip.delta_moments(hipbind.stream(), sink.tensors[0], sink.tensors[2], fmap.start, fmap.stride, fmap.coef.to(dev),
                             torch.from_numpy(live).to(dev), n, delta, 0, ws, sums, stats)
    cols = slice(D, D + 1) if aggregate else slice(0, D)
    merged = Normalize(aggregate=aggregate, batched=True)
    merged.merge(stats[0, cols].reshape(1, 1, -1), stats[1, cols].reshape(1, 1, -1), n)
    assert torch.equal(norm.mean, merged.mean) and torch.equal(norm.var, merged.var)
    assert np.array_equal(record.stats, stats.cpu().numpy())

    # within 2 ulp of the twin's fp64 values (one rounding of the statistics, one of b * n / n in the merge)
    obs, nxt = (sink.tensors[f].cpu().numpy()[live] for f in (0, 2))
    _, twin = dp.moments_numpy(dp.delta_rows_numpy(obs, nxt, fmap, delta))
    d_mean = sc.ulps(norm.mean.cpu().numpy(), twin[0, cols].astype(np.float32))
    d_var = sc.ulps(norm.var.cpu().numpy(), twin[1, cols].astype(np.float32))
    assert d_mean.max() <= 2 and d_var.max() <= 2, (int(d_mean.max()), int(d_var.max()))
    t_mean = sc.ulps(norm.mean.cpu().numpy(), torch_norm.mean.cpu().numpy())
    t_var = sc.ulps(norm.var.cpu().numpy(), torch_norm.var.cpu().numpy())
    tw_mean = sc.ulps(torch_norm.mean.cpu().numpy(), twin[0, cols].astype(np.float32))
    tw_var = sc.ulps(torch_norm.var.cpu().numpy(), twin[1, cols].astype(np.float32))
    print(f"aggregate={aggregate} delta={delta} n={n}: kernel tier vs twin {int(d_mean.max())} / {int(d_var.max())} ulp (mean / var), "
          f"kernel tier vs torch tier {int(t_mean.max())} / {int(t_var.max())} ulp, torch tier vs twin "
          f"{int(tw_mean.max())} / {int(tw_var.max())} ulp")


def test_the_kernel_tier_allocates_no_field():
    """n = 20 000 rows of N = 256: the kernel tier's peak allocation stays below one field of the rows (n N 4 bytes), the
    torch tier's does not."""
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdegym.common.transforms import Normalize
    _, _, dp = _modules()
    dev = torch.device("cuda", 0)
    n, N, B = 20000, 256, 80
    sink = DeviceExperienceReplay(device=dev)
    staged = sink.stage(B, N, 2, expect=n)
    staged.reserve(n // B)
    gen = torch.Generator(device=dev).manual_seed(3)
    sink.tensors[0].copy_(torch.randn(sink.tensors[0].shape, generator=gen, device=dev))
    sink.tensors[2].copy_(sink.tensors[0] + 0.1 * torch.randn(sink.tensors[0].shape, generator=gen, device=dev))
    sink.extend(staged)
    assert sink.ntimesteps == n
    chain = sc.otransf("controller", N)
    peaks, norms = {}, {}
    for tier in ("kernel", "torch"):
        norms[tier] = Normalize(aggregate=True, batched=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        if tier == "kernel":
            assert dp.update_delta_transform(sink, chain, norms[tier], 0.25).tier == "kernel"
        else:
            dp._fit_reference(sink.transitions(), chain, norms[tier], 0.25)
        torch.cuda.synchronize()
        peaks[tier] = torch.cuda.max_memory_allocated(dev) - before
    print(f"peak allocation above the start: kernel tier {peaks['kernel']} bytes, torch tier {peaks['torch']} bytes, one field "
          f"{n * N * 4} bytes")
    assert peaks["kernel"] < n * N * 4 <= peaks["torch"]
    assert norms["kernel"].count == norms["torch"].count == n
