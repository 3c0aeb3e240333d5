"""The imagined-experience replay kept in HBM: ``ExperienceReplay``'s semantics over one slab per field.

``DeviceExperienceReplay``   the controller's ``world_replay``.  The samples live in seven tensors (``DeviceSubSeqStore.tensors``
                             dtypes and trailing shapes) at physical rows that do not move until their episode is evicted;
                             WHICH rows exist is host metadata in integers: per episode its key, its insertion position and
                             its extents, plus ``vindex`` and ``capacity``, all following ``ExperienceReplay.extend`` and
                             ``resize`` to the letter.  Freed extents go to a coalescing free list; a new episode takes free
                             extents in address order and may be split over several, so nothing is ever compacted.
``StagedRollout``            what ``imagine(..., sink=)`` returns: rows already written by ``rp_append`` (csrc/replay.hip)
                             that no dataset sees until ``sink.extend(staged)`` commits them (``sink.discard`` frees them).
``DeviceReplayView``         stands where ``SubSeqDataset(data=world_replay.data, length=1, stride=1, bootstrapping=False)``
                             stands in the policy-update phase (pdecontrol/mbrl/policy_phase.py), which reads the slab in
                             place through the item -> physical-row map instead of packing the replay.


The same class is the controller's real replay: ``collect(..., sink=)`` writes its segments into the slabs
with ``ks_record_device`` and every later phase reads them in place:

``replay.data``              a ``Sample`` of seven read-only mappings from episode key to a lazy column: lengths are metadata,
                             iterating a column fetches it from the slab once.  ``SubSeqDataset``, ``StartingStateDataset``
                             and ``train_test_split(replay.episodes)`` are built from it unchanged.
``replay.window_store()``    ``DeviceSubSeqStore``'s surface over the slabs: windows of any length are gathered through a
                             device map from the packed ("logical") row order to physical rows.
``replay.transitions()``     what ``ExperienceReplay.dataset()`` returns, as device tensors.

Pack equality: ``DeviceSubSeqStore(host_replay.data, device).tensors`` after the same calls equals the slabs read in logical
order, field for field and bit for bit (the host deques hold fp64 rewards and int64 steps; every reader casts through
``_DTYPES``, which is what the slabs hold).

``device="cpu"`` keeps the same metadata over torch CPU tensors.
"""
import bisect
from collections import defaultdict, deque

import numpy as np
import torch

from pdecontrol.mbrl.replay import _DTYPES, _FIELDS, ExperienceReplay
from pdecontrol.mbrl.types import Sample

_TORCH_DTYPES = (torch.float32, torch.float32, torch.float32, torch.float32, torch.bool, torch.bool, torch.int32)


def new_vindex():
    """``ExperienceReplay.vindex``: a sub-environment's first access hands out the next free episode id."""
    vindex = defaultdict(lambda: max(vindex.values(), default=-1) + 1)
    return vindex


def episode_keys(vindex, B, T):
    """The keys ``ExperienceReplay.add`` hands out to the B episodes of one rollout round of T steps, and ``vindex`` moved
    on as their truncated last steps move it: an env's entry is created by its first sample and moved by its truncated
    one, env by env, so a round of several steps touches every env before any moves on (keys in env order) and a round of
    ONE step creates and moves each entry in turn (a first round of one step interleaves 0, 2, 4, ... then 1, 3, 5, ...)."""
    if T > 1:
        for b in range(B):
            vindex[b]
    keys, top = [], max(vindex.values(), default=-1)      # ``top`` stays the largest id: every new one is top + 1
    for b in range(B):
        if b not in vindex:
            top += 1
            vindex[b] = top
        keys.append(vindex[b])
        top += 1
        vindex[b] = top
    return keys


def _carve(extents, T, B):
    """``B`` consecutive pieces of ``T`` rows of a list of extents, each a list of extents."""
    pieces, rest = [], iter(extents)
    start = length = 0
    for _ in range(B):
        need, piece = T, []
        while need:
            if not length:
                start, length = next(rest)
            got = min(length, need)
            piece.append((start, got))
            start, length, need = start + got, length - got, need - got
        pieces.append(piece)
    return pieces


def _rows_of(extents):
    """Physical rows of a list of (start, length) extents, in order."""
    if not extents:
        return np.empty(0, dtype=np.int64)
    ext = np.asarray(extents, dtype=np.int64).reshape(-1, 2)
    starts, lengths = ext[:, 0], ext[:, 1]
    ends = np.cumsum(lengths)
    return np.repeat(starts - (ends - lengths), lengths) + np.arange(ends[-1], dtype=np.int64)


def _extents_of(rows):
    """The (start, length) runs of consecutive rows."""
    rows = np.asarray(rows, dtype=np.int64)
    cuts = np.nonzero(np.diff(rows) != 1)[0] + 1
    first = np.concatenate(([0], cuts))
    last = np.concatenate((cuts, [rows.size]))
    return [(int(rows[a]), int(b - a)) for a, b in zip(first, last)]


class _FreeList:
    """Free extents sorted by address, neighbours coalesced."""

    def __init__(self):
        self.starts, self.lengths, self.total = [], [], 0

    def give(self, start, length):
        if length <= 0:
            return
        i = bisect.bisect_left(self.starts, start)
        assert (i == 0 or self.starts[i - 1] + self.lengths[i - 1] <= start) and \
            (i == len(self.starts) or start + length <= self.starts[i]), "an extent was freed twice"
        self.total += length
        if i < len(self.starts) and start + length == self.starts[i]:
            length += self.lengths[i]
            del self.starts[i], self.lengths[i]
        if i > 0 and self.starts[i - 1] + self.lengths[i - 1] == start:
            self.lengths[i - 1] += length
        else:
            self.starts.insert(i, start)
            self.lengths.insert(i, length)

    def take(self, n):
        """``n`` rows as extents in address order (the caller made sure they exist)."""
        assert 0 <= n <= self.total
        out = []
        while n > 0:
            start, length = self.starts[0], self.lengths[0]
            got = min(length, n)
            out.append((start, got))
            if got == length:
                del self.starts[0], self.lengths[0]
            else:
                self.starts[0], self.lengths[0] = start + got, length - got
            n -= got
            self.total -= got
        return out


class _Episode:
    __slots__ = ("extents", "length", "done", "stopped")

    def __init__(self, extents=(), length=0, done=False, stopped=False):
        self.extents, self.length = list(extents), int(length)
        self.done = bool(done)            # holds a terminated or truncated step: ``extend`` then moves ``vindex`` on
        self.stopped = bool(stopped)      # its last step is truncated: ``ExperienceReplay.stopped``


class _SlabStore:
    """The slabs where the policy phase expects a ``DeviceSubSeqStore``: ``tensors``, ``total`` and ``batch``."""

    def __init__(self, tensors, device):
        self.device = torch.device(device)
        self.tensors = tuple(t.to(self.device) for t in tensors)
        self.total = int(self.tensors[0].shape[0])

    def batch(self, dataset, indices, stransf=None):
        rows = torch.from_numpy(dataset.physical_rows(indices)).to(self.device)
        out = [t.index_select(0, rows).reshape((rows.numel(), 1) + tuple(t.shape[1:])) for t in self.tensors]
        sample = Sample(*out)
        return stransf(sample) if stransf is not None else sample


def _same_device(a, b):
    a, b = torch.device(a), torch.device(b)
    if a.type != b.type:
        return False
    if a.type != "cuda":
        return True
    index = lambda d: torch.cuda.current_device() if d.index is None else d.index
    return index(a) == index(b)


def _stale():
    return RuntimeError("the replay changed after this snapshot of it was taken: take a new one")


class _Column:
    """One field of one episode of a ``DeviceExperienceReplay``: ``len`` is metadata, iterating (or indexing, or
    ``np.asarray``) fetches the column from the slab once and yields the items ``to_host()`` holds."""
    __slots__ = ("_replay", "_field", "_episode", "_version", "_values")

    def __init__(self, replay, field, episode):
        self._replay, self._field, self._episode = replay, field, episode
        self._version, self._values = replay._version, None

    def __len__(self):
        return self._episode.length

    def _fetch(self):
        if self._values is None:
            if self._version != self._replay._version:
                raise _stale()
            self._values = self._replay._fetch_field(self._field, _rows_of(self._episode.extents))
        return self._values

    def __iter__(self):
        return iter(self._fetch())

    def __getitem__(self, i):
        return self._fetch()[i]

    def __array__(self, dtype=None, copy=None):
        values = self._fetch()
        return values if dtype is None else values.astype(dtype, copy=False)


class _Columns(defaultdict):
    """Episode key -> ``_Column`` of one field, in insertion order; read-only, a missing key raises.  (A ``defaultdict``
    because that is how ``SubSeqDataset`` tells a replay's field from a plain array.)"""

    def __init__(self, replay, field):
        super().__init__(None)
        self._replay, self._version = replay, replay._version
        for key, ep in replay._eps.items():
            dict.__setitem__(self, key, _Column(replay, field, ep))

    def _read_only(self, *args, **kwargs):
        raise TypeError("the fields of a DeviceExperienceReplay are read-only: it is filled by extend()")

    __setitem__ = __delitem__ = pop = popitem = clear = update = setdefault = _read_only

    def window_store(self, device):
        """The replay's ``window_store()`` when ``device`` is where its slabs are, else None (the caller packs)."""
        if self._version != self._replay._version:
            raise _stale()
        if self._replay.tensors is None or not _same_device(device, self._replay.device):
            return None
        return self._replay.window_store()


class _WindowStore:
    """``DeviceSubSeqStore``'s surface over the slabs of a ``DeviceExperienceReplay``: ``starts`` and ``total`` of the
    packed ("logical") row order -- episodes in key-insertion order -- and ``rowmap``, a device int64 map from logical
    to physical row.  A snapshot: using it after the replay changed raises."""

    def __init__(self, replay):
        self.replay, self.device, self._version = replay, replay.device, replay._version
        self.starts, off = {}, 0
        for key, ep in replay._eps.items():
            self.starts[key] = off
            off += ep.length
        self.total = off
        self.rowmap = torch.from_numpy(_rows_of([e for ep in replay._eps.values() for e in ep.extents])).to(self.device)
        self._tensors = self._steps_host = None

    def _fresh(self):
        if self._version != self.replay._version:
            raise _stale()

    def gather(self, logical_rows):
        """The seven fields of these logical rows (a device int64 tensor): two ``index_select``s."""
        self._fresh()
        rows = self.rowmap.index_select(0, logical_rows)
        return [t.index_select(0, rows) for t in self.replay.tensors]

    @property
    def tensors(self):
        """The slabs in logical order -- ``DeviceSubSeqStore.tensors`` of the host replay -- gathered on the device
        once, for readers that want the pack itself."""
        if self._tensors is None:
            self._tensors = tuple(self.gather(torch.arange(self.total, device=self.device)))
        self._fresh()
        return self._tensors

    @property
    def steps_host(self):
        """The steps column on the host, in logical order (synchronises, once)."""
        if self._steps_host is None:
            self._fresh()
            self._steps_host = self.replay.tensors[6].index_select(0, self.rowmap).cpu().numpy()
        return self._steps_host

    def batch(self, dataset, indices, stransf=None):
        keys, starts = dataset.locate_many(indices)
        first = np.asarray([self.starts[k] for k in keys], dtype=np.int64) + starts
        rows = torch.from_numpy((first[:, None] + np.arange(dataset.length)[None, :]).reshape(-1)).to(self.device)
        shape = (len(keys), dataset.length)
        sample = Sample(*(t.reshape(shape + tuple(t.shape[1:])) for t in self.gather(rows)))
        return stransf(sample) if stransf is not None else sample


class StagedRollout:
    """Episodes whose rows are reserved (and written, or about to be, in stream order) in ``sink``'s slabs but not yet part
    of it.  It answers what ``ExperienceReplay.extend`` asks of a rollout: ``episodes`` and ``len(vindex)``."""
    device_rollout = None

    def __init__(self, sink, num_envs=None, vindex=None):
        self.sink, self.num_envs, self.state = sink, num_envs, "open"
        self.vindex = new_vindex() if vindex is None else dict(vindex)
        self._eps = {}

    def reserve(self, T):
        """Rows for one round of ``T`` steps of every env: int64 ``dst`` [T, B] for ``rp_append``; env b's episode gets
        the key of ``episode_keys`` and T rows in step order."""
        assert self.state == "open" and self.num_envs
        B = self.num_envs
        extents = self.sink._reserve(T * B)
        for key, piece in zip(episode_keys(self.vindex, B, T), _carve(extents, T, B)):
            self._eps[key] = _Episode(piece, T, done=True, stopped=True)
        return np.ascontiguousarray(_rows_of(extents).reshape(B, T).T)

    @property
    def episodes(self):
        return list(self._eps)

    @property
    def nepisodes(self):
        return len(self._eps)

    @property
    def ntimesteps(self):
        return sum(ep.length for ep in self._eps.values())

    def to_host(self):
        """The ``ExperienceReplay`` the phase returns without a sink (synchronises)."""
        assert self.state == "open", f"this rollout was {self.state}"
        return self.sink._host_replay(self._eps, self.vindex, None)


class DeviceReplayView:
    """Stands where ``SubSeqDataset(data=replay.data, length=1, stride=1, bootstrapping=False, stransf=stransf)`` stands:
    item i is the i-th live row in episode insertion order.  The constructor makes (and discards) the draw
    ``SubSeqDataset.__init__`` makes from numpy's global generator.  A snapshot: rows committed or evicted later are not
    seen, and using the view after such a change raises."""
    length, stride, bootstrapping = 1, 1, False

    def __init__(self, replay, stransf=None):
        self.replay, self.stransf = replay, stransf
        self._version = replay._version
        self.subsamples = replay.episodes
        self._rows = _rows_of([e for ep in replay._eps.values() for e in ep.extents])
        total = np.int64(self._rows.size).astype(np.int32)
        np.random.randint(low=0, high=total, size=total)       # SubSeqDataset's ``boots_mapping``

    def __len__(self):
        return np.int64(self._rows.size).astype(np.int32)

    def _fresh(self):
        if self._version != self.replay._version:
            raise RuntimeError("the replay changed after this view was taken: take a new one with dataset()")

    @property
    def slab_rows(self):
        self._fresh()
        return self.replay.rows

    def widths(self):
        """((channels, columns) of the observations, of the actions)"""
        self._fresh()
        return [(1, self.replay.obs_width), (1, self.replay.act_width)]

    def physical_rows(self, indices):
        """Item indices -> rows of the slab."""
        self._fresh()
        return self._rows[np.asarray(indices, dtype=np.int64)]

    def slab_store(self, device):
        self._fresh()
        return _SlabStore(self.replay.tensors, device)

    def __getitem__(self, idx):
        assert idx < len(self)
        self._fresh()
        row = int(self._rows[int(idx)])
        sample = Sample(*(t[row:row + 1].cpu().numpy().astype(dt) for t, dt in zip(self.replay.tensors, _DTYPES)))
        if self.stransf:
            sample = self.stransf(sample)
        return sample.totorch()


class DeviceExperienceReplay:
    """``ExperienceReplay`` over device slabs (module docstring).  ``rows`` (optional) is the slabs' first size; by default
    they hold ``capacity`` rows plus the first reservation (the whole phase's where ``stage`` is told what to expect), or
    that reservation alone for an unbounded replay."""

    def __init__(self, capacity=None, device="cpu", rows=None):
        self.capacity = np.inf if capacity is None else capacity
        self.device = torch.empty(0, device=device).device      # with its index: "cuda" is the current device
        self.vindex = new_vindex()
        self._eps = {}                      # key -> _Episode, in insertion order
        self._free = _FreeList()
        self._first_rows = rows
        self.tensors, self.rows = None, 0
        self.obs_width = self.act_width = None
        self._live = self._staged = 0
        self._version = 0
        self._window_store = None

    # -- the slabs -------------------------------------------------------------------------------------------------
    def _set_widths(self, obs_width, act_width):
        if self.obs_width is None:
            self.obs_width, self.act_width = int(obs_width), int(act_width)
        elif (self.obs_width, self.act_width) != (int(obs_width), int(act_width)):
            raise ValueError(f"this replay holds rows of {self.obs_width} observation and {self.act_width} action columns, "
                             f"not {obs_width} and {act_width}")

    def _allocate(self, rows):
        shapes = ((1, self.obs_width), (1, self.act_width), (1, self.obs_width), (), (), (), ())
        fresh = tuple(torch.empty((rows,) + s, dtype=dt, device=self.device) for s, dt in zip(shapes, _TORCH_DTYPES))
        if self.tensors is not None:
            for new, old in zip(fresh, self.tensors):
                new[:self.rows].copy_(old)
        self._free.give(self.rows, rows - self.rows)
        self.tensors, self.rows = fresh, rows

    def _ensure(self, n):
        """At least ``n`` free rows: the slabs are allocated at the first call and grow, by reallocate-and-copy, only when
        live plus staged rows plus ``n`` exceed them."""
        assert self.obs_width is not None, "the widths are set before the first reservation"
        if self.tensors is None:
            first = self._first_rows
            if first is None:
                first = n if self.capacity == np.inf else int(self.capacity) + n
            self._allocate(max(int(first), n, 1))
        elif self._free.total < n:
            self._allocate(max(self.rows - self._free.total + n, 2 * self.rows))

    def _reserve(self, n):
        """``n`` free rows as extents in address order."""
        self._ensure(n)
        self._staged += n
        return self._free.take(n)

    def slab(self):
        """``rp_slab`` of the slabs as they stand."""
        from pdecontrol.mbrl import replay_hip
        return replay_hip.slab(self.tensors)

    # -- ExperienceReplay's surface --------------------------------------------------------------------------------
    def _next_episode_id(self):
        return max(self.vindex.values(), default=-1) + 1

    def add(self, samples, stransf=None):
        raise NotImplementedError(
            "DeviceExperienceReplay is filled by extend(): workers write a fresh host ExperienceReplay of their own and the "
            "controller never calls add() on world_replay, so per-step appends have no device path")

    def stage(self, num_envs, obs_width, act_width, expect=0):
        """An empty ``StagedRollout`` of ``num_envs`` sub-environments for rows of these widths.  ``expect``: the rows
        it is going to reserve at the most, so that the slabs grow once, up front, where they have to."""
        self._set_widths(obs_width, act_width)
        if expect > 0:
            self._ensure(int(expect))
        return StagedRollout(self, num_envs)

    def _stage_host(self, replay):
        """The new rows of a host ``ExperienceReplay`` packed, uploaded and placed with ``index_copy_``."""
        staged = StagedRollout(self, vindex=replay.vindex)
        keys = [k for k in replay.episodes if len(replay.obs[k])]
        for k in replay.episodes:
            staged._eps[k] = _Episode()
        if not keys:
            return staged
        first = replay.obs[keys[0]][0], replay.actions[keys[0]][0]
        if np.ndim(first[0]) != 2 or np.ndim(first[1]) != 2 or np.shape(first[0])[0] != 1 or np.shape(first[1])[0] != 1:
            raise ValueError(f"one observation and one action channel are supported, not items of shape "
                             f"{np.shape(first[0])} and {np.shape(first[1])}")
        self._set_widths(np.shape(first[0])[1], np.shape(first[1])[1])
        total = sum(len(replay.obs[k]) for k in keys)
        rows = _rows_of(self._reserve(total))
        packed = [np.concatenate([np.asarray(store[k], dtype=dt).reshape(len(store[k]), *np.shape(store[k][0])) for k in keys])
                  for store, dt in zip(replay._stores(), _DTYPES)]
        index = torch.from_numpy(rows).to(self.device)
        for slab, block in zip(self.tensors, packed):
            slab.index_copy_(0, index, torch.from_numpy(block).to(self.device))
        off = 0
        for k in keys:
            n = len(replay.obs[k])
            term, trunc = packed[4][off:off + n], packed[5][off:off + n]
            staged._eps[k] = _Episode(_extents_of(rows[off:off + n]), n, done=bool(term.any() or trunc.any()),
                                      stopped=bool(trunc[-1]))
            off += n
        return staged

    def extend(self, rollout):
        """``ExperienceReplay.extend`` + ``resize`` on the metadata.  ``rollout``: a ``StagedRollout`` of this replay (its
        rows are in the slabs already) or a host ``ExperienceReplay`` (its rows are uploaded first)."""
        staged = self._stage_host(rollout) if isinstance(rollout, ExperienceReplay) else rollout
        if not isinstance(staged, StagedRollout) or staged.sink is not self:
            raise ValueError("extend() takes a host ExperienceReplay or a rollout staged in this replay")
        if staged.state != "open":
            raise ValueError(f"this rollout was {staged.state} before")
        top = self._next_episode_id() - 1       # stays the largest id in ``vindex``: every new one is top + 1
        for i, key in enumerate(sorted(staged.episodes)):
            vid = i % len(staged.vindex)
            if vid not in self.vindex:
                top += 1
                self.vindex[vid] = top
            vpos = self.vindex[vid]
            theirs = staged._eps[key]
            mine = self._eps.setdefault(vpos, _Episode())
            mine.extents += theirs.extents
            mine.length += theirs.length
            mine.done = mine.done or theirs.done
            if theirs.length:
                mine.stopped = theirs.stopped
            if mine.done:
                top += 1
                self.vindex[vid] = top
            self._live += theirs.length
            self._staged -= theirs.length
        staged.state = "committed"
        self._version += 1
        self.resize(self.capacity)

    def discard(self, staged):
        """Frees the rows of a rollout that is not to be committed."""
        if staged.sink is not self or staged.state != "open":
            raise ValueError("discard() takes an open rollout staged in this replay")
        for ep in staged._eps.values():
            for extent in ep.extents:
                self._free.give(*extent)
            self._staged -= ep.length
        staged.state = "discarded"

    def resize(self, size):
        """Drop the episodes of smallest key until at most ``size`` time steps remain."""
        self.capacity = size
        if self._live <= self.capacity:
            return
        for key in sorted(self._eps):
            ep = self._eps.pop(key)
            for extent in ep.extents:
                self._free.give(*extent)
            self._live -= ep.length
            if self._live <= self.capacity:
                break
        self._version += 1

    @property
    def episodes(self):
        return list(self._eps)

    @property
    def nepisodes(self):
        return len(self._eps)

    @property
    def ntimesteps(self):
        return self._live

    @property
    def stopped(self):
        return [k for k, ep in self._eps.items() if ep.stopped]

    @property
    def nstopped(self):
        return len(self.stopped)

    def _fetch(self, rows):
        """The seven fields of these rows as numpy arrays (synchronises)."""
        if self.tensors is None:
            return [np.empty((0,), dtype=dt) for dt in _DTYPES]
        index = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(self.device)
        return [t.index_select(0, index).cpu().numpy() for t in self.tensors]

    def _fetch_field(self, field, rows):
        """One field of these rows as a numpy array (synchronises)."""
        index = torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(self.device)
        return self.tensors[field].index_select(0, index).cpu().numpy()

    @property
    def data(self):
        """``ExperienceReplay.data`` of the replay as it stands: a ``Sample`` of seven read-only mappings from episode
        key to a lazy column (module docstring).  A snapshot: fetching from it after the replay changed raises."""
        return Sample(*(_Columns(self, field) for field in range(len(_FIELDS))))

    def window_store(self):
        """The ``_WindowStore`` of the replay as it stands (one per state of the replay: its readers share it)."""
        if self.tensors is None:
            raise ValueError("an empty replay has no rows to gather")
        if self._window_store is None or self._window_store._version != self._version:
            self._window_store = _WindowStore(self)
        return self._window_store

    def transitions(self):
        """The ``Sample`` ``ExperienceReplay.dataset()`` returns -- all live rows in insertion order, every field fp32
        -- as tensors on the replay's device (for ``update_delta_transform``)."""
        if self.tensors is None:
            return Sample(*(torch.empty(0, dtype=torch.float32, device=self.device) for _ in _FIELDS))
        rows = torch.from_numpy(_rows_of([e for ep in self._eps.values() for e in ep.extents])).to(self.device)
        return Sample(*(t.index_select(0, rows).to(torch.float32) for t in self.tensors))

    def sample(self, index=None, stransf=None):
        index = np.random.choice(self.episodes) if index is None else index
        sample = Sample(*(np.asarray(v, dtype=dt) for v, dt in zip(self._fetch(_rows_of(self._eps[index].extents)), _DTYPES)))
        if stransf is not None:
            sample = stransf(sample)
        return sample.totorch()

    def statistics(self):
        """Mean and standard deviation of the returns of the stopped episodes: each return is Python's ``sum`` over the
        episode's fp32 rewards (on a GPU: ``rp_episode_returns``, the same chain of fp32 additions), then ``np.mean`` and
        ``np.std`` over the list of ``np.float32``, as ``ExperienceReplay.statistics`` computes them."""
        eps = [self._eps[k] for k in self.stopped]
        if not eps:
            returns = []
        elif self.device.type != "cuda":
            rewards = self.tensors[3].numpy()
            returns = [sum(rewards[_rows_of(ep.extents)]) for ep in eps]
        else:
            import hipbind
            from pdecontrol.mbrl import replay_hip
            replay_hip.load()
            rows = torch.from_numpy(_rows_of([e for ep in eps for e in ep.extents])).to(self.device)
            offsets = torch.from_numpy(np.concatenate(([0], np.cumsum([ep.length for ep in eps]))).astype(np.int64)).to(self.device)
            out = torch.empty(len(eps), dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                replay_hip.episode_returns(hipbind.stream(), self.tensors[3], rows, offsets, out)
            returns = list(out.cpu().numpy())
        return np.mean(returns), np.std(returns)

    def dataset(self, stransf=None):
        """The ``DeviceReplayView`` of the live rows as they stand."""
        return DeviceReplayView(self, stransf)

    def _host_replay(self, eps, vindex, capacity):
        replay = ExperienceReplay(capacity)
        lengths = [ep.length for ep in eps.values()]
        fields = self._fetch(_rows_of([e for ep in eps.values() for e in ep.extents]))
        off = 0
        for key, n in zip(eps, lengths):
            for store, values in zip(replay._stores(), fields):
                store[key] = deque(values[off:off + n])
            off += n
        replay.vindex.update(vindex)
        return replay

    def to_host(self):
        """The ``ExperienceReplay`` the host replay would be after the same calls (synchronises)."""
        return self._host_replay(self._eps, self.vindex, None if self.capacity == np.inf else self.capacity)
