"""The device-resident real replay on the host: header, binding and library agree on
``ks_record_device`` and it refuses bad arguments before any device call; the CPU twin of ``ks_record_device`` against a
numpy twin bit for bit; the loop tier of ``collect(..., sink=)`` against ``worker.rollout`` + the host ``extend``; and the
readers of a ``DeviceExperienceReplay(device="cpu")`` (``data``, ``window_store``, ``transitions``, the policy phase)
against the packed host replay."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _collect_scenario as sc  # noqa: E402
import _policy_phase_scenario as pp_sc  # noqa: E402
import _real_replay_scenario as rr  # noqa: E402
import _sac_models as sm  # noqa: E402
from test_capi_symbols import LIBDIR, declared_functions  # noqa: E402

import kspde  # noqa: E402
from pdecontrol.mbrl import collection_phase as cp  # noqa: E402
from pdecontrol.mbrl.device_replay import DeviceExperienceReplay, StagedRollout  # noqa: E402
from pdecontrol.mbrl.replay import ExperienceReplay  # noqa: E402
from pdecontrol.mbrl.types import Sample  # noqa: E402
from pdecontrol.surrogates.common import dataset as ds  # noqa: E402


# ----------------------------------------------------------------------------------------------------------------------
# header, binding, refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_ks_record_device():
    assert "ks_record_device" in declared_functions("kspde.h", "ks")
    rows = {name: (res, args) for name, res, args in kspde.SYMBOLS}
    res, args = rows["ks_record_device"]
    assert res is ctypes.c_int and len(args) == 11 and args[-1] == ctypes.POINTER(kspde.ks_record)
    assert [n for n, _ in kspde.ks_record._fields_] == ["obs", "actions", "nxtobs", "rewards", "terminated", "truncated",
                                                       "steps", "rows"]
    assert ctypes.sizeof(kspde.ks_record) == 8 * 8
    assert os.path.exists(os.path.join(LIBDIR, "libkspde.so")), "libkspde.so not built (run __graft_entry__.build())"
    assert hasattr(kspde.load(), "ks_record_device")


def test_ks_record_device_refuses_before_any_device_call():
    """On the CPU twin's handle, with pointers that are never dereferenced: each refusal is negative and its text starts
    with the entry's name."""
    lib = kspde.load()
    E, T, A = 3, 2, 4
    s = kspde.KSStepper(E, 64, device=-1)
    fake = ctypes.c_void_p(64)
    dst = np.arange(T * E, dtype=np.int64)
    d = dst.ctypes.data_as(ctypes.c_void_p)
    slabs = lambda rows=16, **kw: kspde.ks_record(**{**{n: 64 for n, _ in kspde.ks_record._fields_[:7]}, "rows": rows, **kw})
    good = dict(h=s._h, traj=fake, actions=fake, A=A, ssq=fake, steps=fake, T=T, sub=250, dst=d, dst_host=d, out=slabs())

    def call(**change):
        a = {**good, **change}
        out = a["out"]
        return lib.ks_record_device(a["h"], a["traj"], a["actions"], a["A"], a["ssq"], a["steps"], a["T"], a["sub"], a["dst"],
                                    a["dst_host"], None if out is None else ctypes.byref(out))

    twice = dst.copy()
    twice[4] = twice[1]
    beyond = dst.copy()
    beyond[5] = 16
    cases = {"NULL handle": dict(h=None), "NULL traj": dict(traj=None), "NULL actions": dict(actions=None),
             "NULL ssq": dict(ssq=None), "NULL steps": dict(steps=None), "NULL dst": dict(dst=None),
             "NULL dst_host": dict(dst_host=None), "NULL out": dict(out=None), "NULL slab": dict(out=slabs(rewards=None)),
             "NULL flags": dict(out=slabs(truncated=None)), "T = 0": dict(T=0), "A = 0": dict(A=0), "A = 17": dict(A=17),
             "no sub-step": dict(sub=0), "no rows": dict(out=slabs(rows=0)),
             "beyond": dict(dst_host=beyond.ctypes.data_as(ctypes.c_void_p)),
             "twice": dict(dst_host=twice.ctypes.data_as(ctypes.c_void_p))}
    texts = {}
    for what, change in cases.items():
        assert call(**change) < 0, what
        texts[what] = lib.ks_last_error().decode()
        assert texts[what].startswith("ks_record_device:"), (what, texts[what])
    assert "beyond" in texts["beyond"] and "16" in texts["beyond"] and "twice" in texts["twice"]
    assert len({texts[k] for k in ("T = 0", "A = 0", "no sub-step", "no rows", "beyond", "twice")}) == 6
    with pytest.raises(kspde.KSError, match="ks_record_device: 0 steps"):
        s.record_device(64, 64, A, 64, 64, 0, 250, 64, np.empty(0, dtype=np.int64), slabs())


# ----------------------------------------------------------------------------------------------------------------------
# the CPU twin against the numpy twin
# ----------------------------------------------------------------------------------------------------------------------
def test_the_halfway_sums_exist():
    """The search finds rewards exactly halfway between two fp32 numbers where the scale is a power of two, and numpy
    rounds them to even -- the rounding the entry is held to."""
    sums = rr.halfway_sums(64, 1)
    assert len(sums) == 5
    for s in sums:
        reward = (-1.0) * (1 / 64) * s / 1
        lo, hi = np.float32(reward), np.nextafter(np.float32(reward), np.float32(-np.inf if np.float32(reward) > reward else np.inf))
        assert (np.float64(lo) + np.float64(hi)) / 2 == reward and not (lo.view(np.int32) & 1)
    assert rr.halfway_sums(64, 250) or rr.halfway_sums(100, 250) or rr.halfway_sums(98, 1)


def _record(stepper, seg, A, n_substeps, dst, slabs):
    traj, actions, ssq, steps = seg
    record = kspde.ks_record(*(a.ctypes.data for a in slabs), slabs[0].shape[0])
    stepper.record_device(traj.ctypes.data, actions.ctypes.data, A, ssq.ctypes.data, steps.ctypes.data, dst.shape[0],
                          n_substeps, dst.ctypes.data, dst, record)


@pytest.mark.parametrize("N", [64, 98, 100])
def test_ks_record_device_on_the_cpu_twin_equals_the_numpy_twin(N):
    rs = np.random.RandomState(N)
    for E in (1, 5):
        stepper = kspde.KSStepper(E, N, L=22.0 * N / 64, device=-1)
        for A in (1, 4, 16):
            for T in (1, 5):
                for n_substeps in (1, 250):
                    seg = rr.segment(rs, T, E, N, A, n_substeps)
                    for form in rr.DST_FORMS:
                        dst, rows = rr.dst_form(form, rs, T, E)
                        got, want = rr.filled_slabs(rows, N, A), rr.filled_slabs(rows, N, A)
                        _record(stepper, seg, A, n_substeps, dst, got)
                        rr.record_twin(want, seg, n_substeps, dst)
                        rr.same_slabs(got, want, (N, E, A, T, n_substeps, form))
                        untouched = np.setdiff1d(np.arange(rows), dst[dst >= 0])
                        assert untouched.size and np.all(got[0][untouched] == rr.FILL_F) and np.all(got[3][untouched] == rr.FILL_F)
                        assert np.all(got[4][untouched] == rr.FILL_B) and np.all(got[6][untouched] == rr.FILL_I)


# ----------------------------------------------------------------------------------------------------------------------
# the staged rollout of the kernel tier, filled by the CPU twin
# ----------------------------------------------------------------------------------------------------------------------
def _fill(phase, stepper, pieces, n_substeps):
    """What the kernel tier does with a phase's pieces: a segment through ``reserve`` + ``ks_record_device``, a host step
    through ``host_step``."""
    for piece in pieces:
        if isinstance(piece, Sample):
            phase.host_step(piece)
            continue
        traj, actions, ssq, steps = piece
        dst = phase.reserve(actions.shape[0])
        assert dst.dtype == np.int64 and dst.flags.c_contiguous and dst.shape == steps.shape
        stepper.record_device(traj.ctypes.data, actions.ctypes.data, actions.shape[2], ssq.ctypes.data,
                              np.ascontiguousarray(steps, dtype=np.int32).ctypes.data, actions.shape[0], n_substeps,
                              dst.ctypes.data, dst, phase.slabs())


@pytest.mark.parametrize("first_cut", [False, True])
def test_the_staged_rollout_of_the_kernel_tier_is_what_build_replay_builds(first_cut):
    """Two phases of (segment of 3 steps, a host step with a partial truncation, segment of 2 steps) -- the second phase
    optionally opened by a host step at which every env truncates, which interleaves the keys -- staged in a CPU sink with
    the CPU twin of ``ks_record_device`` and committed, against ``build_replay`` of the same pieces (rewards formed on the
    host with the env's expression) extended into a host replay: keys, ``vindex``, what ``extend`` sees, the pack."""
    E, N, A, n_substeps, rs = 3, 64, 4, 250, np.random.RandomState(int(first_cut))
    stepper = kspde.KSStepper(E, N, device=-1)
    host, sink = ExperienceReplay(20), DeviceExperienceReplay(20, device="cpu")
    for p in range(2):
        seg = lambda T: rr.segment(rs, T, E, N, A, n_substeps)[:3] + (rs.randint(0, 50, (T, E)).astype(np.int64),)
        step = lambda cut: Sample(rs.randn(E, 1, N).astype(np.float32), rs.randn(E, 1, A).astype(np.float32),
                                  rs.randn(E, 1, N).astype(np.float32), rs.randn(E), np.zeros(E, dtype=bool), cut,
                                  rs.randint(0, 50, E).astype(np.int64))
        pieces = [seg(3), step(np.asarray([False, True, False])), seg(2)]
        if first_cut and p == 1:
            pieces.insert(0, step(np.ones(E, dtype=bool)))
        with np.errstate(all="ignore"):
            built = cp.build_replay([x if isinstance(x, Sample) else (x[0], x[1], (-1.0) * (1 / N) * x[2] / n_substeps, x[3])
                                     for x in pieces], E)
        phase = cp._SinkPhase(sink, E, N, A, expect=sum(1 if isinstance(x, Sample) else x[1].shape[0] for x in pieces) * E)
        _fill(phase, stepper, pieces, n_substeps)
        staged = phase.staged
        built.tier = built.tier_reason = built.host_steps = staged.tier = staged.tier_reason = staged.host_steps = None
        rr.same_staged(staged, built, p)
        host.extend(built)
        sink.extend(staged)
        rr.same_metadata(sink, host, p)
        rr.pack_contract(sink, host, p)
    assert host.ntimesteps <= 20 < 2 * 6 * E and sink._staged == 0


# ----------------------------------------------------------------------------------------------------------------------
# the loop tier through a sink
# ----------------------------------------------------------------------------------------------------------------------
class RandomAgent:
    def select_action(self, obs, deterministic=False):
        return np.random.uniform(-1, 1, (obs.shape[0], 1, 4)).astype(np.float32)


def _phases(route, agent_kind, capacity=None, phases=2, stagger=True, E=3, steps=3):
    """``phases`` collection phases of ``steps`` steps on the CPU-twin stack: the committed replay and, per phase, what
    the phase returned, the replay's record after the commit and the state record."""
    s = sc.build(E=E)
    sc.seed()
    agent = s.agent if agent_kind == "sac" else RandomAgent()
    callback = sc.Callback()
    s.worker.callbacks.append(callback)
    sc.prime(s.worker, 11, stagger=stagger)
    stop = lambda ts, ep: ts >= steps * E
    replay = ExperienceReplay(capacity) if route == "host" else DeviceExperienceReplay(capacity, device="cpu")
    out = []
    for _ in range(phases):
        got = s.worker.rollout(agent, stop) if route == "host" else cp.collect(s.worker, agent, stop, sink=replay)
        if route == "host":
            got.tier, got.tier_reason, got.host_steps = "loop", None, steps
        replay.extend(got)
        out.append((got, sc.state_record(s.worker), dict(episodes=replay.episodes, vindex=dict(replay.vindex),
                                                          ntimesteps=replay.ntimesteps, stopped=replay.stopped)))
    assert len(callback.seen) == phases and all(isinstance(r, ExperienceReplay) for r in callback.seen)
    return replay, out


@pytest.mark.parametrize("agent_kind", ["random", "sac"])
def test_the_loop_tier_through_a_sink_equals_rollout_plus_extend(agent_kind):
    host, want = _phases("host", agent_kind)
    sink, got = _phases("sink", agent_kind)
    for i, ((a, sa, ma), (b, sb, mb)) in enumerate(zip(want, got)):
        assert ma == mb, (i, ma, mb)
        assert isinstance(b, StagedRollout) and b.state == "committed" and b.tier == "loop" and b.host_steps == 3
        assert b.tier_reason and ("RandomAgent" in b.tier_reason or "on the CPU" in b.tier_reason)
        assert b.episodes == a.episodes and dict(b.vindex) == dict(a.vindex), i
        sc.assert_same_state(sa, sb)
    rr.same_metadata(sink, host)
    rr.pack_contract(sink, host)
    assert host.nstopped > 0 and any(len(ep.extents) > 1 for ep in sink._eps.values()), "no episode grew across phases"


def test_a_small_capacity_evicts_an_episode_that_is_still_open():
    """Three envs from counters 0, phases of 3 steps, capacity 5: the first commit evicts the open episodes 0 and 1, the
    second phase continues them under their old keys at the end of the order."""
    kwargs = dict(capacity=5, phases=3, stagger=False)
    host, want = _phases("host", "sac", **kwargs)
    sink, got = _phases("sink", "sac", **kwargs)
    assert [m for _, _, m in got] == [m for _, _, m in want]
    first = got[0][2]
    assert first["episodes"] == [2] and first["vindex"] == {0: 0, 1: 1, 2: 2} and first["stopped"] == []
    # (the second phase writes one more step under the keys 0, 1 and 2, re-created at the end of the order, and the
    # third commits while they are still among the smallest keys: both replays evict them again, in the same order)
    rr.same_metadata(sink, host)
    rr.pack_contract(sink, host)
    assert sink.ntimesteps <= 5 and sink._staged == 0 and sink._free.total == sink.rows - sink.ntimesteps


def test_a_sink_on_another_device_is_refused():
    s = sc.build(E=3)

    class Elsewhere(DeviceExperienceReplay):
        def __init__(self):
            super().__init__(device="cpu")
            self.device = torch.device("cuda", 1)

    sc.prime(s.worker, 3, stagger=False)
    with pytest.raises(ValueError, match="sink"):
        cp.collect(s.worker, s.agent, lambda ts, ep: ts >= 3, sink=Elsewhere())
    with pytest.raises(ValueError, match="DeviceExperienceReplay"):
        cp.collect(s.worker, s.agent, lambda ts, ep: ts >= 3, sink=ExperienceReplay())


# ----------------------------------------------------------------------------------------------------------------------
# the readers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair():
    """Host replay and CPU sink after five phases under a capacity that evicts: episodes of up to four steps, some split
    over extents, the slab fragmented."""
    host, _ = _phases("host", "sac", capacity=30, phases=5, steps=4)
    sink, _ = _phases("sink", "sac", capacity=30, phases=5, steps=4)
    rr.same_metadata(sink, host)
    assert any(len(ep.extents) > 1 for ep in sink._eps.values())
    logical = sink.window_store().rowmap.numpy()
    assert not np.array_equal(logical, np.sort(logical)), "the slab order is the packed order: nothing is remapped"
    return host, sink


@pytest.fixture
def no_pack(monkeypatch):
    packs = []
    real = ds.DeviceSubSeqStore.__init__
    monkeypatch.setattr(ds.DeviceSubSeqStore, "__init__", lambda self, *a, **k: (packs.append(1), real(self, *a, **k))[1])
    return packs


def _same_item(a, b, what):
    a, b = tuple(a), tuple(b)
    assert len(a) == len(b) == 7
    for name, x, y in zip(rr.FIELDS, a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (what, name)


def _numpy_state():
    return np.random.get_state()[1].copy(), np.random.get_state()[2]


@pytest.mark.parametrize("kind,kwargs", [("subseq", dict(length=2, stride=1, bootstrapping=True)),
                                         ("subseq", dict(length=3, stride=2, bootstrapping=False)),
                                         ("subseq", dict(length=1, stride=1, bootstrapping=False, bounds=(1, 0))),
                                         ("starting", dict(length=3, stride=1, bootstrapping=False))])
def test_datasets_over_replay_data_equal_the_ones_over_the_host_copy(pair, kind, kwargs):
    host, sink = pair
    cls = ds.SubSeqDataset if kind == "subseq" else ds.StartingStateDataset
    built = []
    for data in (sink.to_host().data, sink.data):
        np.random.seed(17)
        d = cls(data=data, subsamples=sink.episodes[1:], **kwargs)
        built.append((d, _numpy_state()))
    (want, want_rng), (got, got_rng) = built
    assert np.array_equal(got_rng[0], want_rng[0]) and got_rng[1] == want_rng[1]
    assert len(got) == len(want) > 0
    parts = zip(got.datasets, want.datasets) if kind == "starting" else [(got, want)]
    for g, w in parts:
        assert len(g) == len(w)
        if len(w):
            gk, gs = g.locate_many(np.arange(len(g)))
            wk, ws = w.locate_many(np.arange(len(w)))
            assert gk == wk and np.array_equal(gs, ws)
    for i in range(len(want)):
        _same_item(got[i], want[i], i)
    assert isinstance(sink.data.obs, ds.defaultdict) and list(sink.data.steps.keys()) == sink.episodes
    with pytest.raises(TypeError):
        sink.data.obs[0] = []
    with pytest.raises(KeyError):
        sink.data.obs[10 ** 6]


@pytest.mark.parametrize("bootstrapping", [True, False])
def test_device_batch_loader_over_the_slabs_equals_the_packed_route(pair, bootstrapping, no_pack):
    host, sink = pair
    store = ds.device_store(sink.data, "cpu")
    assert store is sink.window_store() and not no_pack
    packed = ds.device_store(host.data, "cpu")
    assert type(packed) is ds.DeviceSubSeqStore and no_pack == [1]
    loaders = []
    for data, st in ((host.data, packed), (sink.data, store)):
        np.random.seed(5)
        d = ds.SubSeqDataset(data=data, subsamples=sink.episodes[:-1], length=2, stride=1, bootstrapping=bootstrapping)
        loaders.append(ds.DeviceBatchLoader(d, st, batch_size=next(b for b in (4, 3, 5, 7) if len(d) % b)))
    want, got = (list(loader) for loader in loaders)
    assert len(got) == len(want) == len(loaders[0]) and len(want) > 1
    assert want[-1][0].shape[0] < want[0][0].shape[0], "no ragged last batch"
    for i, (g, w) in enumerate(zip(got, want)):
        pp_sc.same_batch(g, w, f"batch {i}")


def test_starting_states_over_the_slabs_equal_the_packed_route(pair, no_pack):
    from pdecontrol.mbrl.world.world import _DeviceStartingStates
    host, sink = pair
    out = []
    for data in (host.data, sink.data):
        np.random.seed(3)
        torch.manual_seed(8)
        starting = ds.StartingStateDataset(data=data, length=3, stride=1, bootstrapping=False)
        states = _DeviceStartingStates(starting, torch.device("cpu"), 6)
        batches = [states.next_batch() for _ in range(3)]
        out.append((states, batches, torch.get_rng_state().clone()))
    (w_states, want, w_rng), (g_states, got, g_rng) = out
    assert type(w_states.store) is ds.DeviceSubSeqStore and g_states.store is sink.window_store() and no_pack == [1]
    assert torch.equal(g_rng, w_rng)
    for i, ((gs, gsteps), (ws, wsteps)) in enumerate(zip(got, want)):
        pp_sc.same_batch(list(gs), list(ws), f"batch {i}")
        assert gsteps.dtype == wsteps.dtype and np.array_equal(gsteps, wsteps)


def test_transitions_are_the_host_dataset(pair):
    host, sink = pair
    got = sink.transitions()
    for want in (sink.to_host().dataset(), host.dataset()):
        for name, g, w in zip(rr.FIELDS, got, want):
            assert g.dtype == torch.float32 and w.dtype == np.float32 and tuple(g.shape) == w.shape, name
            assert g.numpy().tobytes() == w.tobytes(), name
    empty = DeviceExperienceReplay(device="cpu").transitions()
    assert all(t.shape == (0,) and t.dtype == torch.float32 for t in empty)


def test_snapshots_of_a_replay_that_changed_raise():
    host, _ = _phases("host", "sac", phases=1)
    sink = DeviceExperienceReplay(device="cpu")
    sink.extend(host)
    store, data = sink.window_store(), sink.data
    assert sink.window_store() is store                                # one per state of the replay
    store.gather(torch.arange(2))
    sink.extend(host)
    assert sink.window_store() is not store
    with pytest.raises(RuntimeError, match="changed"):
        store.gather(torch.arange(2))
    with pytest.raises(RuntimeError, match="changed"):
        store.batch(ds.SubSeqDataset(data=sink.data, length=1, bootstrapping=False), [0])
    with pytest.raises(RuntimeError, match="changed"):
        list(data.obs[sink.episodes[0]])
    with pytest.raises(RuntimeError, match="changed"):
        ds.device_store(data, "cpu")
    assert len(data.obs[sink.episodes[0]]) >= 0                        # lengths are metadata: no fetch, no check


def test_cpu_policy_phase_over_two_views_equals_the_one_over_two_host_datasets(pair, no_pack):
    """Imagined and real replay both device-resident (``device="cpu"``): the agent ends where it ends over the two host
    ``SubSeqDataset``s, bit for bit, with torch's and numpy's generators."""
    from pdecontrol.mbrl import policy_phase as pp
    real_host, real = pair
    rollout = pp_sc.scripted_replay(16, 4, 3, 21, {0: (4, 11, 30), 1: (9,), 2: (15, 16)})
    world_host, world = ExperienceReplay(), DeviceExperienceReplay(device="cpu")
    world_host.extend(rollout)
    world.extend(rollout)
    to_agent_world, to_agent = pp_sc.controller_connectors(4, stride=4, low=-1.0, high=1.0)
    host_sets = lambda: [ds.SubSeqDataset(data=r.data, length=1, stride=1, bootstrapping=False, stransf=t)
                         for r, t in ((world_host, to_agent_world), (real_host, to_agent))]
    views = lambda: [world.dataset(to_agent_world), real.dataset(to_agent)]
    out = []
    for make in (host_sets, views):
        agent = sm.build(32, auto=True, interval=2, obs_dim=16, act_dim=4, seed=5, low=-1.0, high=1.0)
        torch.manual_seed(11)
        np.random.seed(12)
        before = len(no_pack)
        assert pp.update_policy(agent, make(), 33, 4) == 4
        state = sm.full_state(agent)
        state["rng"] = torch.get_rng_state()
        state["numpy"] = torch.from_numpy(np.random.get_state()[1].astype(np.int64))
        out.append((state, len(no_pack) - before))
    assert out[0][1] == 2 and out[1][1] == 0, "the views pack nothing"
    assert set(out[0][0]) == set(out[1][0])
    for k in out[0][0]:
        assert torch.equal(out[0][0][k], out[1][0][k]), k
