#!/usr/bin/env python3
"""Timings of the controller's ``update_delta_transform`` on an MI355X (pdecontrol/mbrl/delta_phase.py).  Record and
criterion.

The replay is a ``DeviceExperienceReplay`` whose slabs are filled directly: episodes of 250 transitions, each in two
extents of 125 rows, the extents placed in a random permutation of the slab, so the live rows are neither sorted nor
contiguous.  N observations, 4 actions, the controller's connector (observations scaled by running extrema aggregated to
scalars, sensor of stride 1), ``Normalize(aggregate=True, batched=True)``, delta = 0.15.  Sizes: 10^5 and 10^6 rows at
N = 64, 2.5 10^5 rows at N = 256 (``--sizes``).

  (a) parent   the route of the parent commit, made only of calls it has: ``undscaling.reset()``, ``replay.transitions()``
               (seven fields gathered), the connector on both observation fields, the subtraction, the division and
               ``Normalize.update``.
  (b) kernel   ``update_delta_transform`` on its kernel tier: row list and coefficients uploaded, ``rpd_moments``,
               one copy back, ``Normalize.merge``.

One process, both routes warmed twice and then alternated over ``--rounds`` (5) rounds, a host clock around work that
ends in a device synchronisation; median, minimum and range.  Both routes also report the peak of
``torch.cuda.max_memory_allocated`` above the level before the call.  After the rounds the parts of (b) are timed one by
one, each ending in a synchronisation of its own (``b_laps``): they say where the time goes, they do not add up to (b).

Criterion, per size, against (a)'s median AND its minimum: (b)'s median <= 0.5 x (a), and (b)'s peak extra memory is below
the bytes of one field of the rows (n x N x 4).

  --parent-only   time (a) alone: runs on the parent commit's tree too, in a process of its own

Usage (repo root, on an MI355X):  python tools/delta_phase_bench.py    (writes profiles/delta_phase_bench.json)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "model-based-pde-control_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

A, EPISODE, EXTENT, DELTA = 4, 250, 125, 0.15


def filled_replay(n, N, dev, seed):
    """``n`` live rows (a multiple of 250) in a slab of exactly ``n`` rows, the extents permuted."""
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay, _Episode
    assert n % EPISODE == 0
    sink = DeviceExperienceReplay(device=dev, rows=n)
    sink._set_widths(N, A)
    sink._reserve(n)
    order = np.random.RandomState(seed).permutation(n // EXTENT)
    per = EPISODE // EXTENT
    for key in range(n // EPISODE):
        extents = [(int(b) * EXTENT, EXTENT) for b in order[key * per:(key + 1) * per]]
        sink._eps[key] = _Episode(extents, EPISODE, done=True, stopped=True)
    sink._live, sink._staged = n, 0
    sink._version += 1
    gen = torch.Generator(device=dev).manual_seed(seed)
    obs, nxt = sink.tensors[0], sink.tensors[2]
    obs.copy_(torch.randn(obs.shape, generator=gen, device=dev))
    nxt.copy_(torch.randn(obs.shape, generator=gen, device=dev))
    nxt.mul_(0.3).add_(obs).add_(0.05)
    for t in sink.tensors[1:2] + sink.tensors[3:]:
        t.zero_()
    return sink


def connector(N):
    from pdegym.common.transforms import BatchTransform, ScaleTransform, SensorTransform, SampleTransform
    oscaling = ScaleTransform(batched=True, aggregate=True, frozen=False)
    oscaling.update(np.random.RandomState(5).uniform(-4.0, 4.0, (16, 1, N)).astype(np.float32))
    return SampleTransform(otransf=[oscaling, BatchTransform(SensorTransform(stride=1))]).otransf


def route_parent(sink, chain, norm):
    norm.reset()
    data = sink.transitions()
    deltas = chain(data.nxtobs) - chain(data.obs)
    norm.update(deltas / DELTA)


def timed(call, dev):
    """(milliseconds, peak bytes allocated above the level before the call)"""
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    level = torch.cuda.memory_allocated(dev)
    t0 = time.perf_counter()
    call()
    torch.cuda.synchronize(dev)
    ms = 1e3 * (time.perf_counter() - t0)
    return ms, int(torch.cuda.max_memory_allocated(dev) - level)


def laps(sink, chain, N, n, dev, rounds):
    """Median milliseconds of the kernel tier's parts, each timed on its own with a synchronisation after it."""
    import hipbind
    from pdecontrol.mbrl import delta_phase as dp, replay_hip
    from pdecontrol.mbrl.device_replay import _rows_of
    from pdecontrol.mbrl.recognition import field_map
    from pdegym.common.transforms import Normalize
    out = {}

    def lap(name, call):
        call()
        out[name] = round(float(np.median([timed(call, dev)[0] for _ in range(rounds)])), 4)

    extents = [e for ep in sink._eps.values() for e in ep.extents]
    fmap = field_map(chain, N)
    coef, rows = fmap.coef.to(dev), dp.device_rows(extents, dev)
    workspace = torch.empty(replay_hip.delta_workspace_doubles(N, n), dtype=torch.float64, device=dev)
    sums = torch.empty((2, N + 1), dtype=torch.float64, device=dev)
    stats = torch.empty((2, N + 1), dtype=torch.float32, device=dev)
    norm = Normalize(aggregate=True, batched=True)

    def merge():
        norm.reset()
        norm.merge(stats[0, N:].reshape(1, 1, -1), stats[1, N:].reshape(1, 1, -1), n)

    lap("extent_list_ms", lambda: [e for ep in sink._eps.values() for e in ep.extents])
    lap("device_rows_ms", lambda: dp.device_rows(extents, dev))
    lap("host_rows_and_upload_ms", lambda: torch.from_numpy(_rows_of(extents)).to(dev))      # what device_rows replaced
    lap("field_map_ms", lambda: field_map(chain, N))
    lap("coef_upload_ms", lambda: fmap.coef.to(dev))
    lap("rpd_moments_ms", lambda: replay_hip.delta_moments(hipbind.stream(), sink.tensors[0], sink.tensors[2], fmap.start,
                                                           fmap.stride, coef, rows, n, DELTA, 0, workspace, sums, stats))
    lap("copy_back_ms", lambda: stats.cpu().numpy())
    lap("merge_ms", merge)
    return out


def summary(ms):
    return {"ms": [round(x, 3) for x in ms], "median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3),
            "range_ms": round(max(ms) - min(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sizes", default="100000x64,1000000x64,250000x256")
    ap.add_argument("--parent-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda", 0)
    from pdegym.common.transforms import Normalize
    routes = {"a_parent": route_parent}
    if not args.parent_only:
        from pdecontrol.mbrl import delta_phase as dp

        def route_kernel(sink, chain, norm):
            record = dp.update_delta_transform(sink, chain, norm, DELTA)
            assert record.tier == "kernel", (record.tier, record.tier_reason)
        routes["b_kernel"] = route_kernel

    sizes = []
    for i, size in enumerate(args.sizes.split(",")):
        n, N = (int(v) for v in size.split("x"))
        sink, chain = filled_replay(n, N, dev, 10 + i), connector(N)
        norms = {name: Normalize(aggregate=True, batched=True) for name in routes}
        for _ in range(2):                                   # warm-up: code objects, the allocator's blocks
            for name, call in routes.items():
                call(sink, chain, norms[name])
        torch.cuda.synchronize(dev)
        ms, peak = {name: [] for name in routes}, {name: 0 for name in routes}
        for _ in range(args.rounds):
            for name, call in routes.items():
                t, p = timed(lambda: call(sink, chain, norms[name]), dev)
                ms[name].append(t)
                peak[name] = max(peak[name], p)
        field = n * N * 4
        rec = {"rows": n, "N": N, "one_field_bytes": field}
        for name in routes:
            rec[name] = dict(summary(ms[name]), peak_extra_bytes=peak[name], mean=float(norms[name].mean.reshape(-1)[0]),
                             var=float(norms[name].var.reshape(-1)[0]))
        if not args.parent_only:
            a, b = rec["a_parent"], rec["b_kernel"]
            rec["b_over_a_median"] = round(b["median_ms"] / a["median_ms"], 4)
            rec["b_over_a_min"] = round(b["median_ms"] / a["min_ms"], 4)
            rec["b_at_most_half_of_a_median"] = bool(b["median_ms"] <= 0.5 * a["median_ms"])
            rec["b_at_most_half_of_a_min"] = bool(b["median_ms"] <= 0.5 * a["min_ms"])
            rec["b_peak_below_one_field"] = bool(b["peak_extra_bytes"] < field)
            rec["b_laps"] = laps(sink, chain, N, n, dev, args.rounds)
        sizes.append(rec)
        del sink
        torch.cuda.empty_cache()

    rec = {"what": "update_delta_transform over a DeviceExperienceReplay (episodes of 250 rows in two permuted extents, 4 actions, "
                   "the controller's connector, Normalize(aggregate, batched), delta 0.15): ms per call of (a) the parent commit's "
                   "route -- transitions() + connector + Normalize.update -- and (b) the kernel tier; one process, both warmed "
                   "twice, alternated over the rounds, host clock around work ending in a device synchronisation; peak of "
                   "max_memory_allocated above the level before the call",
           "device": torch.cuda.get_device_name(dev), "rounds": args.rounds, "parent_only": bool(args.parent_only), "sizes": sizes}
    if not args.parent_only:
        rec["criterion"] = "b median <= 0.5 x a (median and minimum) and b peak extra bytes < one field, at every size"
        rec["criterion_met"] = bool(all(s["b_at_most_half_of_a_median"] and s["b_at_most_half_of_a_min"] and s["b_peak_below_one_field"]
                                        for s in sizes))
    line = json.dumps(rec)
    print(line)
    out = args.out
    if out is None and not args.parent_only:
        out = os.path.join(ROOT, "profiles", "delta_phase_bench.json")
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
