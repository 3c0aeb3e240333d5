"""The controller's policy-update phase (reference ``pdecontrol/mbrl/mbrl.py:529-566``) behind one call.

The reference builds, per phase,

    data    = ConcatDataset((imagined, real))                     # SubSeqDataset(length=1, stride=1, bootstrapping=False)
    sampler = RandomSampler(data, replacement=True, num_samples=B * U)
    loader  = DataLoader(data, batch_size=B, sampler=sampler, collate_fn=PDEDataLoader.sample_collate)
    for batch in loader: agent.update(batch)

which costs B Python ``__getitem__`` calls, a collate and five host-to-device copies per update.  Here:

``PolicyBatchPlan``   the loader's index stream, drawn at once from torch's global CPU generator with the loader's own draws
                      in the loader's order, and resolved to (source, packed row) for all U x B samples (host, numpy).
``recognize``         reads a dataset's connector (``SampleTransform``) and, where it is sensors and at most one scaling per
                      field, reduces it to a column sensor and per-column affine coefficients.
``update_policy``     runs the U updates on one of three tiers (chosen per call, announced once per reason):
                      kernel tier      one ``rp_gather`` launch per update (csrc/replay.hip) writes the batch from the
                                       replays packed in HBM straight into the static input buffers of the agent's
                                       captured update, then the two noise draws and one graph replay;
                      torch on device  ``DeviceSubSeqStore.batch`` per source, merged in plan order, ``agent.update``;
                      CPU              one vectorised gather per field from the replays packed on the host, ``agent.update``.

In every tier the batches are the reference loader's, sample for sample and bit for bit, the global torch generator is
left where the loader would leave it, and the agent ends where the reference loop would leave it.
"""
import time
from dataclasses import dataclass

import numpy as np
import torch

from pdecontrol.mbrl.recognition import FieldMap, Unrecognized, field_map, notice
from pdecontrol.mbrl.types import Sample
from pdecontrol.surrogates import ops
from pdecontrol.surrogates.common.dataset import DeviceSubSeqStore, device_store
from pdegym.common import transforms as tr


# ----------------------------------------------------------------------------------------------------------------------
# 1. the index plan
# ----------------------------------------------------------------------------------------------------------------------
def _is_view(dataset):
    """A ``DeviceReplayView``: a dataset whose samples already lie in device slabs."""
    return hasattr(dataset, "physical_rows")


def _store(dataset, device):
    """The tensors the batches of ``dataset`` are gathered from: a view's slabs as they stand, else ``device_store``'s
    answer (one pack of a host replay; a device-resident replay's rows gathered into packed order on the device)."""
    return dataset.slab_store(device) if _is_view(dataset) else device_store(dataset.fields, device, DeviceSubSeqStore)


class PolicyBatchPlan:
    """The U x B samples the reference loader draws from ``ConcatDataset(datasets)``, in its order.

    ``source`` [U, B]   which dataset each sample comes from
    ``local``  [U, B]   its item index inside that dataset
    ``rows``   [U, B]   its row in that dataset's packed replay (``DeviceSubSeqStore`` order: episodes in key order)
    ``concat_rows``     its row in the concatenation of the packed replays (``first[source] + rows``)
    ``totals``          rows of each packed replay

    A ``DeviceReplayView`` (pdecontrol/mbrl/device_replay.py) among the datasets is a source that is not packed: its
    ``rows`` are physical rows of the replay's slab and its entry of ``totals`` is the slab's rows.

    Construction consumes from torch's global CPU generator exactly what the loader consumes: the ``DataLoader`` iterator's
    base seed, then ``RandomSampler``'s seed; the indices come from a private generator seeded with the latter, in
    ``RandomSampler``'s 32-wide ``torch.randint`` chunks plus the remainder.  numpy's generator is not touched."""

    def __init__(self, datasets, batch_size, num_updates, indices=None):
        """``indices`` (tests, tools): U x B item indices of the ``ConcatDataset`` to resolve in place of drawing them."""
        self.datasets = list(datasets)
        self.batch_size, self.num_updates = int(batch_size), int(num_updates)
        if not self.datasets or self.batch_size < 1 or self.num_updates < 0:
            raise ValueError("PolicyBatchPlan needs at least one dataset, a batch size >= 1 and a number of updates >= 0")
        for d in self.datasets:
            if d.length != 1:
                raise ValueError(f"the policy phase samples single transitions: dataset of window length {d.length}")
        cum = np.cumsum([int(len(d)) for d in self.datasets], dtype=np.int64)   # ConcatDataset.cumulative_sizes
        if cum[-1] < 1:
            raise ValueError("the policy phase has no sample to draw from")
        if indices is None:
            idx = self._draw(int(cum[-1]), self.batch_size * self.num_updates).numpy()
        else:
            idx = np.asarray(indices, dtype=np.int64).reshape(self.batch_size * self.num_updates)
            assert idx.size == 0 or (0 <= idx.min() and idx.max() < cum[-1])
        shape = (self.num_updates, self.batch_size)
        source = np.searchsorted(cum, idx, side="right")                        # ConcatDataset's bisect_right
        local = idx - np.where(source > 0, cum[np.maximum(source - 1, 0)], 0)
        rows = np.empty_like(idx)
        self.totals = []
        for s, d in enumerate(self.datasets):
            if _is_view(d):                   # a device-resident replay: the source is the slab, rows are physical
                self.totals.append(int(d.slab_rows))
                sel = source == s
                if sel.any():
                    rows[sel] = d.physical_rows(local[sel])
                continue
            keys = list(d.fields[0].keys())
            lengths = np.fromiter((len(d.fields[0][k]) for k in keys), dtype=np.int64, count=len(keys))
            starts = dict(zip(keys, np.concatenate(([0], np.cumsum(lengths)[:-1])) if keys else ()))
            self.totals.append(int(lengths.sum()))
            sel = source == s
            if sel.any():
                episodes, steps = d.locate_many(local[sel])
                rows[sel] = np.fromiter((starts[k] for k in episodes), dtype=np.int64, count=len(episodes)) + steps
        self.first = np.concatenate(([0], np.cumsum(self.totals)[:-1])).astype(np.int64)
        self.source, self.local, self.rows = source.reshape(shape), local.reshape(shape), rows.reshape(shape)
        self.concat_rows = (self.first[source] + rows).reshape(shape)

    @staticmethod
    def _draw(n, num_samples):
        torch.empty((), dtype=torch.int64).random_()            # _BaseDataLoaderIter.__init__: the base seed
        seed = int(torch.empty((), dtype=torch.int64).random_().item())    # RandomSampler.__iter__ at the first batch
        generator = torch.Generator()
        generator.manual_seed(seed)
        out = torch.empty(num_samples, dtype=torch.int64)
        whole = num_samples // 32 * 32
        for i in range(0, whole, 32):
            torch.randint(high=n, size=(32,), dtype=torch.int64, generator=generator, out=out[i:i + 32])
        if num_samples > whole:
            torch.randint(high=n, size=(num_samples - whole,), dtype=torch.int64, generator=generator, out=out[whole:])
        return out


# ----------------------------------------------------------------------------------------------------------------------
# 3. transform recognition
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Connector:
    obs: FieldMap
    actions: FieldMap


def recognize(stransf, obs_width, act_width):
    """``Connector`` of a dataset's ``stransf`` (None: the identity) for packed rows of these widths, or raises
    ``Unrecognized``: any number of ``SensorTransform``s and at most one ``ScaleTransform`` (either direction) per field,
    ``BatchTransform`` wrappers and ``Identity`` looked through."""
    if stransf is None:
        return Connector(FieldMap(0, 1, obs_width, None), FieldMap(0, 1, act_width, None))
    if not isinstance(stransf, tr.SampleTransform):
        raise Unrecognized(f"a {type(stransf).__name__} in place of a SampleTransform")
    return Connector(field_map(stransf.otransf, obs_width), field_map(stransf.atransf, act_width))


def _widths(dataset):
    """(channels, columns) of the stored observations and actions of a dataset's replay."""
    if _is_view(dataset):
        return dataset.widths()
    out = []
    for store in dataset.fields[:2]:
        shape = np.shape(next(iter(store.values()))[0])
        out.append((int(np.prod(shape[:-1], dtype=np.int64)), int(shape[-1])))
    return out


def _connector(dataset):
    (ochan, owidth), (achan, awidth) = _widths(dataset)
    if ochan != 1 or achan != 1:
        raise Unrecognized(f"replays with {ochan} observation and {achan} action channels")
    con = recognize(dataset.stransf, owidth, awidth)
    if (con.actions.start, con.actions.stride) != (0, 1):
        raise Unrecognized("a sensor on the actions")
    return con


# ----------------------------------------------------------------------------------------------------------------------
# 4. the phase
# ----------------------------------------------------------------------------------------------------------------------
def _notice(reason):
    notice("the fused batch gather does not implement %s: the policy-update phase assembles its batches with plain "
           "PyTorch-ROCm kernels", reason)


def _merge(parts, positions, B):
    """Per-source batches (lists of seven tensors) scattered to their positions in the loader's batch."""
    if len(parts) == 1:
        return list(parts[0])
    out = []
    for column in zip(*parts):
        merged = torch.empty((B,) + tuple(column[0].shape[1:]), dtype=column[0].dtype, device=column[0].device)
        for part, pos in zip(column, positions):
            merged[pos] = part
        out.append(merged)
    return out


def _transform_items(stransf, sample):
    """``stransf`` item by item, as the dataset's ``__getitem__`` applies it (for transforms that are not known to act
    independently of a leading batch axis)."""
    items = [tuple(stransf(Sample(*(f[i] for f in sample)))) for i in range(sample.obs.shape[0])]
    return Sample(*(torch.stack([torch.as_tensor(v) for v in col]) for col in zip(*items)))


def host_batches(plan, stores=None):
    """The loader's batches (lists of seven CPU tensors, ``default_collate``'s layout) from the replays packed on the
    host: per source and field one ``index_select``, the connector applied to the gathered block."""
    stores = stores or [_store(d, "cpu") for d in plan.datasets]
    whole = []
    for d in plan.datasets:
        try:
            _connector(d)
            whole.append(True)
        except Unrecognized:
            whole.append(False)
    for u in range(plan.num_updates):
        parts, positions = [], []
        for s, (d, store) in enumerate(zip(plan.datasets, stores)):
            pos = np.nonzero(plan.source[u] == s)[0]
            if pos.size == 0:
                continue
            rows = torch.from_numpy(plan.rows[u, pos])
            fields = [t.index_select(0, rows).reshape((pos.size, 1) + tuple(t.shape[1:])) for t in store.tensors]
            fields[6] = fields[6].to(torch.int32)
            sample = Sample(*fields)
            if d.stransf is not None:
                sample = d.stransf(sample) if whole[s] else _transform_items(d.stransf, sample)
            parts.append(list(sample))
            positions.append(torch.from_numpy(pos))
        yield _merge(parts, positions, plan.batch_size)


def device_batches(plan, stores):
    """The same batches assembled in HBM: ``DeviceSubSeqStore.batch`` per source, merged in plan order."""
    device = stores[0].device
    for u in range(plan.num_updates):
        parts, positions = [], []
        for s, (d, store) in enumerate(zip(plan.datasets, stores)):
            pos = np.nonzero(plan.source[u] == s)[0]
            if pos.size == 0:
                continue
            parts.append(list(store.batch(d, plan.local[u, pos], stransf=d.stransf)))
            positions.append(torch.from_numpy(pos).to(device))
        yield _merge(parts, positions, plan.batch_size)


class _KernelTier:
    """What the kernel tier keeps alive for one phase: the packed replays, the coefficient tensors, the ``rp_source``
    array pointing at both, and the plan's rows on the device."""

    def __init__(self, plan, connectors, device):
        from pdecontrol.mbrl import replay_hip
        self.stores = [_store(d, device) for d in plan.datasets]       # one pack per source per phase; a view: no pack
        self.coefs, entries = [], []
        for store, con in zip(self.stores, connectors):
            obs, actions, nxtobs, rewards, terminated = store.tensors[:5]
            assert store.total == obs.shape[0] and all(t.is_contiguous() for t in store.tensors[:5])
            ocoef, acoef = (None if m.coef is None else m.coef.to(device) for m in (con.obs, con.actions))
            self.coefs += [ocoef, acoef]
            entries.append(replay_hip.Source(
                obs.data_ptr(), actions.data_ptr(), nxtobs.data_ptr(), rewards.data_ptr(), terminated.data_ptr(), store.total,
                obs[0].numel(), actions[0].numel(), con.obs.start, con.obs.stride,
                None if ocoef is None else ocoef.data_ptr(), None if acoef is None else acoef.data_ptr()))
        assert [s.total for s in self.stores] == plan.totals
        self.srcs = replay_hip.sources(entries)
        self.rows = torch.from_numpy(plan.concat_rows).to(device)                      # [U, B] int64, uploaded once
        self.obs_dim, self.act_dim = connectors[0].obs.width, connectors[0].actions.width

    def refusal(self, B):
        from pdecontrol.mbrl import replay_hip
        return replay_hip.supported(self.srcs, B)


def _kernel_tier(agent, plan):
    """The ``_KernelTier`` and the agent's fused companion when this phase runs on the kernels, else (None, None)."""
    from pdecontrol.sac import sac_hip
    if not ops.fused_enabled():
        return None, None
    try:
        connectors = [_connector(d) for d in plan.datasets]
    except Unrecognized as e:
        _notice(str(e))
        return None, None
    if len({(c.obs.width, c.actions.width) for c in connectors}) != 1:
        _notice("replays whose connectors yield different widths")
        return None, None
    B, dev = plan.batch_size, agent.device
    obs_dim, act_dim = connectors[0].obs.width, connectors[0].actions.width
    like = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    obs, batch = like(B, 1, obs_dim), (like(B, 1, act_dim), like(B, 1), like(B, 1))
    if not sac_hip.use_kernels(agent, obs, batch):             # announces its own reason
        return None, None
    tier = _KernelTier(plan, connectors, dev)
    reason = tier.refusal(B)
    if reason is not None:
        _notice(reason)
        return None, None
    return tier, agent._fused_for(obs, batch)


def update_policy(agent, datasets, batch_size, num_updates, timings=None):
    """``for batch in loader: agent.update(batch)`` of the reference's ``update_policy`` for the loader described in the
    module docstring; returns the number of updates done.  ``datasets`` are the controller's ``SubSeqDataset``s in
    ``ConcatDataset`` order.  ``timings`` (tools/policy_phase_bench.py) is an optional dict that receives the host seconds
    of the plan, of packing the replays and of the updates, and the tier that ran; on a CUDA agent each of the three then
    ends in a device synchronisation, which the phase otherwise never does."""
    clock = time.perf_counter
    cuda = agent.device.type == "cuda"

    def lap(name, t0):
        if timings is not None:
            if cuda:
                torch.cuda.synchronize(agent.device)
            timings[name] = timings.get(name, 0.0) + clock() - t0
        return clock()

    t = clock()
    plan = PolicyBatchPlan(datasets, batch_size, num_updates)
    t = lap("plan_s", t)
    if plan.num_updates == 0:
        return 0
    if not cuda:
        stores = [_store(d, "cpu") for d in plan.datasets]
        t = lap("pack_s", t)
        for batch in host_batches(plan, stores):
            agent.update(batch)
        lap("updates_s", t)
        if timings is not None:
            timings["tier"] = "cpu"
        return plan.num_updates
    tier, fused = _kernel_tier(agent, plan)
    if tier is None:
        stores = [_store(d, agent.device) for d in plan.datasets]
        t = lap("pack_s", t)
        for batch in device_batches(plan, stores):
            agent.update(batch)
        lap("updates_s", t)
        if timings is not None:
            timings["tier"] = "torch-on-device"
        return plan.num_updates

    from pdecontrol.mbrl import replay_hip
    from pdecontrol.sac import sac_hip
    B = plan.batch_size
    graph = fused.graph_for((B, (1, tier.act_dim)))
    t = lap("pack_s", t)                                                    # the packs, the rows' upload, the first capture
    history = agent._stats_history(plan.num_updates)
    seen = None if history is not None else fused.counters[4].clone()      # without a logger: the device's own count
    base, stream = tier.rows.data_ptr(), sac_hip._stream()
    for u in range(plan.num_updates):
        fill = lambda: replay_hip.gather(stream, tier.srcs, B, base + u * B * 8, graph.obs, graph.actions, graph.nxtobs,
                                         graph.rewards, graph.terminated)
        agent._replay_update(fused, graph, fill, None if history is None else history[u])
    if history is None:
        agent._check_terminated(int(fused.counters[4] - seen))
    agent._log_history(history)
    lap("updates_s", t)
    if timings is not None:
        timings["tier"] = "kernel"
    return plan.num_updates
