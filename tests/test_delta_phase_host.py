"""The delta-statistics phase without a GPU: header, binding and refusals of ``rpd_moments``;
``Normalize.merge`` inside ``update`` against the formula it replaced; the numpy twin of the kernel's per-row arithmetic
against the reference expression on torch CPU tensors, bit for bit; the host tier; tier selection and its notices."""
import ctypes
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _delta_phase_scenario as sc  # noqa: E402
from _policy_phase_scenario import scripted_replay  # noqa: E402
from test_capi_symbols import LIBDIR, declared_functions  # noqa: E402

from pdecontrol.mbrl import delta_phase as dp, replay_hip  # noqa: E402
from pdecontrol.mbrl.device_replay import DeviceExperienceReplay  # noqa: E402
from pdecontrol.mbrl.recognition import field_map  # noqa: E402
from pdegym.common.transforms import FuncTransform, Normalize, SampleTransform  # noqa: E402


def same_bits(a, b):
    a, b = (np.ascontiguousarray(torch.as_tensor(v).detach().cpu().numpy()) for v in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ----------------------------------------------------------------------------------------------------------------------
# header, binding, refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_delta_entries():
    """The ``rpd_*`` half of replay_hip.h is bound name for name by ``DELTA_SYMBOLS`` and exported by the library; the
    ``rp_*`` half and its table stay what they were."""
    names = declared_functions("replay_hip.h", "rpd")
    assert names == ["rpd_moments", "rpd_workspace_doubles"] == sorted(n for n, _, _ in replay_hip.DELTA_SYMBOLS)
    assert not [n for n, _, _ in replay_hip.SYMBOLS if n.startswith("rpd_")]
    rows = {name: (res, args) for name, res, args in replay_hip.DELTA_SYMBOLS}
    res, args = rows["rpd_moments"]
    assert res is ctypes.c_int and len(args) == 15 and args[10] is ctypes.c_float
    assert rows["rpd_workspace_doubles"] == (ctypes.c_long, [ctypes.c_int, ctypes.c_long, ctypes.c_int])
    header = open(os.path.join(os.path.dirname(LIBDIR), "..", "include", "replay_hip.h")).read()
    assert f"#define RP_MAX_DELTA_GROUPS {replay_hip.MAX_DELTA_GROUPS}\n" in header
    assert os.path.exists(os.path.join(LIBDIR, "libreplay_hip.so")), "libreplay_hip.so not built (run __graft_entry__.build())"
    lib = replay_hip.load()
    assert hasattr(lib, "rpd_moments") and hasattr(lib, "rpd_workspace_doubles")
    assert lib.rpd_moments.argtypes == args and lib.rpd_workspace_doubles.restype is ctypes.c_long


def test_the_workspace_query_is_a_host_function():
    ws = replay_hip.delta_workspace_doubles
    G = replay_hip.MAX_DELTA_GROUPS                      # above 32 workgroups the middle launch has ceil(G / 32) rows more
    assert ws(64, 1) == 2 * 64 and ws(64, 16) == 2 * 64 and ws(64, 17) == 2 * 2 * 64            # default: ceil(n / 16), capped
    assert ws(98, 512) == 32 * 2 * 98 and ws(98, 513) == (33 + 2) * 2 * 98 and ws(98, 4099) == (257 + 9) * 2 * 98
    assert ws(64, 10 ** 6) == (G + G // 32) * 2 * 64 and ws(1024, 7, 3) == 3 * 2 * 1024 and ws(8, 7, 5000) == (G + G // 32) * 2 * 8
    assert ws(0, 5) == 0 and ws(1025, 5) == 0 and ws(64, 0) == 0 and ws(64, 5, -1) == 0


def test_rpd_moments_refuses_before_any_device_call():
    """Every code, with pointers that are never dereferenced and no device in the process: each refusal is negative, has
    a code of its own and a text that starts with the entry's name."""
    lib = replay_hip.load()
    fake = ctypes.c_void_p(64)
    good = dict(stream=None, obs=fake, nxtobs=fake, slab_rows=10, obs_width=64, start=0, stride=1, coef=None, rows=None, n=5,
                delta=0.25, groups=0, workspace=fake, sums=fake, stats=fake)
    cases = {"NULL obs": (dict(obs=None), -70), "NULL nxtobs": (dict(nxtobs=None), -70), "NULL workspace": (dict(workspace=None), -70),
             "NULL sums": (dict(sums=None), -70), "NULL stats": (dict(stats=None), -70), "n = 0": (dict(n=0), -71),
             "no slab rows": (dict(slab_rows=0), -72), "stride 0": (dict(stride=0), -73), "start beyond": (dict(start=64), -74),
             "start negative": (dict(start=-1), -74), "no columns": (dict(obs_width=0), -74),
             "too wide": (dict(obs_width=1025), -75), "delta 0": (dict(delta=0.0), -76), "delta inf": (dict(delta=float("inf")), -76),
             "delta nan": (dict(delta=float("nan")), -76), "groups -1": (dict(groups=-1), -77)}
    texts = {}
    for what, (change, code) in cases.items():
        a = {**good, **change}
        assert lib.rpd_moments(*a.values()) == code, what
        texts[what] = replay_hip.last_error()
        assert texts[what].startswith("rpd_moments:"), (what, texts[what])
    assert len({texts[k] for k in ("NULL obs", "n = 0", "no slab rows", "stride 0", "start beyond", "too wide", "delta 0",
                                   "groups -1")}) == 8
    # 1024 columns of a wider row through a sensor are fine: only the output columns are capped (and nothing else is
    # wrong with `good`, which would launch)
    assert "1025" in texts["too wide"] and "-1" in texts["groups -1"]


def test_the_binding_raises_with_the_code():
    t = torch.zeros(4, 1, 8)
    with pytest.raises(replay_hip.ReplayHipError, match="rpd_moments: a step of 0") as e:
        replay_hip.delta_moments(None, t, t, 0, 1, None, None, 4, 0.0, 0, torch.zeros(16, dtype=torch.float64),
                                 torch.zeros(2, 9, dtype=torch.float64), torch.zeros(2, 9))
    assert e.value.code == -76


# ----------------------------------------------------------------------------------------------------------------------
# Normalize.merge
# ----------------------------------------------------------------------------------------------------------------------
def parent_update(state, t, dim):
    """``Normalize.update`` as it stood before ``merge`` was split off, on (mean, var, count)."""
    mean, var, count = state
    n_new = t.shape[0]
    b_mean = torch.mean(t, dim=dim, keepdim=True, dtype=torch.float32)
    b_var = torch.var(t, dim=dim, keepdim=True)
    if mean is None:
        mean = torch.zeros_like(b_mean)
    if var is None:
        var = torch.zeros_like(b_mean)
    total = count + n_new
    delta = b_mean - mean
    m2 = var * count + b_var * n_new + delta * delta * count * n_new / total
    return mean + delta * n_new / total, m2 / total, total


@pytest.mark.parametrize("aggregate", [True, False])
def test_update_equals_the_formula_it_had_before_merge(aggregate):
    rs = np.random.RandomState(3)
    norm = Normalize(aggregate=aggregate, batched=True)
    state = (None, None, 0)
    for n, N in ((37, 16), (5, 16)):                     # two successive updates
        t = torch.from_numpy((rs.randn(n, 1, N) * 3 + 0.7).astype(np.float32))
        norm.update(t)
        state = parent_update(state, t, (0, 1, 2) if aggregate else (0, 1))
        assert same_bits(norm.mean, state[0]) and same_bits(norm.var, state[1]) and norm.count == state[2]
        assert tuple(norm.mean.shape) == ((1, 1, 1) if aggregate else (1, 1, N))
    # merge alone is update after its two reductions
    other, t = Normalize(aggregate=aggregate, batched=True), torch.from_numpy(rs.randn(9, 1, 16).astype(np.float32))
    other.merge(torch.mean(t, dim=other.dim, keepdim=True, dtype=torch.float32), torch.var(t, dim=other.dim, keepdim=True), 9)
    want = parent_update((None, None, 0), t, other.dim)
    assert same_bits(other.mean, want[0]) and same_bits(other.var, want[1]) and other.count == 9
    frozen = Normalize(aggregate=aggregate, batched=True, frozen=True)
    frozen.merge(want[0], want[1], 9)
    assert frozen.mean is None and frozen.count == 0


# ----------------------------------------------------------------------------------------------------------------------
# the numpy twin
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [0.25, 0.15])
@pytest.mark.parametrize("kind", sc.CONNECTORS)
def test_delta_rows_numpy_equals_the_reference_expression_bit_for_bit(kind, delta):
    """0.15 is where a multiplication by the reciprocal would show: it is not a power of two."""
    rs = np.random.RandomState(11)
    n, N = 301, 22
    obs = rs.randn(n, 1, N).astype(np.float32)
    nxt = (obs + delta * (0.3 + 2.0 * rs.randn(n, 1, N))).astype(np.float32)
    chain = sc.otransf(kind, N)
    want = sc.reference_deltas(chain, torch.from_numpy(obs.copy()), torch.from_numpy(nxt.copy()), delta)
    fmap = field_map(chain, N)
    got = dp.delta_rows_numpy(obs, nxt, fmap, delta)
    assert fmap.stride == (2 if kind == "stride2" else 1) and (fmap.coef is None) == (kind == "unscaled")
    assert got.dtype == np.float32 and want.dtype == torch.float32 and got.shape == tuple(want.shape) == (n, 1, fmap.width)
    assert got.tobytes() == want.numpy().tobytes()
    if delta == 0.15:                                    # the reciprocal route is a different function on these inputs
        reciprocal = (fmap.apply_numpy(nxt) - fmap.apply_numpy(obs)) * (np.float32(1) / np.float32(delta))
        assert np.any(reciprocal != got)


def test_moments_numpy_layout():
    rs = np.random.RandomState(5)
    d = (rs.randn(13, 1, 6) * 2 + 1).astype(np.float32)
    sums, stats = dp.moments_numpy(d)
    d64 = d.astype(np.float64).reshape(13, 6)
    assert sums.shape == stats.shape == (2, 7) and sums.dtype == stats.dtype == np.float64
    assert np.array_equal(sums[0, :6], d64.sum(0)) and sums[1, 6] == (d64 * d64).sum()
    assert np.array_equal(stats[0, :6], d64.mean(0)) and np.array_equal(stats[1, :6], d64.var(0, ddof=1))
    assert stats[0, 6] == d64.mean() and stats[1, 6] == d64.var(ddof=1)
    one = dp.moments_numpy(d[:1, :, :1])[1]
    assert np.isnan(one[1]).all() and one[0, 0] == d64[0, 0]


# ----------------------------------------------------------------------------------------------------------------------
# tiers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("aggregate", [True, False])
def test_the_host_tier_is_the_reference_lines(aggregate):
    replay = scripted_replay(12, 2, 4, 14, {0: (5, 12), 1: (8,)})
    chain, delta = sc.otransf("controller", 12), 0.15
    got, want = Normalize(aggregate=aggregate, batched=True), Normalize(aggregate=aggregate, batched=True)
    got.update(torch.ones(3, 1, 12))                     # the phase resets first
    record = dp.update_delta_transform(replay, chain, got, delta)
    want.reset()
    dataset = replay.dataset()
    deltas = chain(dataset.nxtobs) - chain(dataset.obs)
    want.update(deltas / delta)
    assert (record.tier, record.tier_reason, record.rows) == ("host", None, 28) and got.count == want.count == 28
    assert same_bits(got.mean, want.mean) and same_bits(got.var, want.var)


def test_tier_selection_and_the_once_per_reason_notice(caplog):
    from pdecontrol.surrogates import ops
    sink = DeviceExperienceReplay(device="cpu")
    sink.extend(scripted_replay(12, 2, 4, 14, {0: (5, 12), 1: (8,)}))
    chain, delta = sc.otransf("controller", 12), 0.25
    odd = SampleTransform(otransf=[FuncTransform(lambda t: t * 2.0)]).otransf
    cases = [("a frozen Normalize", chain, Normalize(aggregate=True, batched=True, frozen=True)),
             ("a Normalize that is not batched", chain, Normalize(aggregate=True, batched=False)),
             ("a FuncTransform", odd, Normalize(aggregate=True, batched=True)),
             ("a replay that is not on a GPU", chain, Normalize(aggregate=True, batched=True))]
    for reason, _, _ in cases:
        ops._NOTIFIED.discard(reason)
    with caplog.at_level(logging.INFO, logger="pdecontrol.surrogates"):
        for reason, otransf, norm in cases:
            for _ in range(2):
                record = dp.update_delta_transform(sink, otransf, norm, delta)
                assert (record.tier, record.tier_reason, record.rows) == ("torch", reason, 28)
            want = Normalize(aggregate=norm.aggregate, batched=norm.batched, frozen=norm.frozen)
            data = sink.transitions()
            want.update((otransf(data.nxtobs) - otransf(data.obs)) / delta)
            assert norm.count == want.count == (0 if norm.frozen else 28)
            assert norm.frozen or (same_bits(norm.mean, want.mean) and same_bits(norm.var, want.var))
    said = [r.getMessage() for r in caplog.records if "delta statistics" in r.getMessage()]
    assert len(said) == 4 and all(sum(reason in s for s in said) == 1 for reason, _, _ in cases)
    levels = {r.getMessage().split(": ", 1)[1]: r.levelno for r in caplog.records if "delta statistics" in r.getMessage()}
    assert levels == {reason: logging.INFO for reason, _, _ in cases}       # expected on a CPU replay


def test_device_rows_is_rows_of():
    """The row list expanded from the extent table with torch ops (here on the CPU) is ``_rows_of``'s."""
    from pdecontrol.mbrl.device_replay import _rows_of
    sink = sc.fragmented_replay("cpu")
    extents = [e for ep in sink._eps.values() for e in ep.extents]
    for ext in (extents, extents[:1], [(7, 1)], [(5, 3), (0, 2), (40, 1), (9, 4)]):
        got = dp.device_rows(ext, "cpu")
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), _rows_of(ext))
    assert len(extents) > len(sink.episodes) and np.array_equal(dp.device_rows(extents, "cpu").numpy(), sc.live_rows(sink))


def test_the_host_and_torch_tiers_agree_on_a_cpu_replay():
    host = scripted_replay(12, 2, 4, 14, {0: (5, 12), 1: (8,)})
    sink = DeviceExperienceReplay(device="cpu")
    sink.extend(host)
    chain = sc.otransf("stride2", 12)
    a, b = Normalize(aggregate=False, batched=True), Normalize(aggregate=False, batched=True)
    assert dp.update_delta_transform(host, chain, a, 0.15).tier == "host"
    assert dp.update_delta_transform(sink, chain, b, 0.15).tier == "torch"
    assert a.count == b.count == 28 and tuple(a.mean.shape) == (1, 1, 6)
    assert same_bits(a.mean, b.mean) and same_bits(a.var, b.var)
