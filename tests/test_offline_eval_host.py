"""The offline surrogate evaluation without a GPU: a frozen, fitted ``Normalize`` as the affine map of
``recognition.field_map`` bit for bit; the folds; header, binding and refusals of ``rpn_moments``; its numpy twin
against ``Normalize.update``; the host tier of ``fit_scalings`` against the reference's lines; ``generate_dataset`` and
``main`` end to end on the stepper's CPU twin."""
import ctypes
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _offline_eval_scenario as sc  # noqa: E402
from test_capi_symbols import LIBDIR, declared_functions  # noqa: E402

from pdecontrol.mbrl import replay_hip  # noqa: E402
from pdecontrol.mbrl.recognition import Unrecognized, field_map, flatten, inverse_map, world_connector  # noqa: E402
from pdecontrol.surrogates.evaluation import evaluate as ev  # noqa: E402
from pdegym.common import transforms as T  # noqa: E402


# ----------------------------------------------------------------------------------------------------------------------
# a frozen, fitted Normalize is an affine map
# ----------------------------------------------------------------------------------------------------------------------
STATISTICS = {"scalar": (0.37, 2.5), "scalar-wide": (0.0, 1e20), "scalar-negative": (-4.0, 1e-3),
              "columns": (np.linspace(-2.0, 3.0, 12), np.linspace(0.05, 9.0, 12)), "columns-wide": (np.zeros(12), np.full(12, 1e20))}
WRAPS = {"bare": lambda n: n, "batch": lambda n: T.BatchTransform(n), "operation": lambda n: T.Operation([T.BatchTransform(n)]),
         "sensor": lambda n: T.Operation([n, T.BatchTransform(T.SensorTransform(stride=1))])}


@pytest.mark.parametrize("wrap", sorted(WRAPS))
@pytest.mark.parametrize("stats", sorted(STATISTICS))
def test_a_frozen_normalize_is_the_affine_map_bit_for_bit(stats, wrap):
    """``FieldMap.apply_numpy`` of the chain against the torch CPU transform, forward and inverse, on 2000 rows of random
    values plus +-0, +-inf, NaN, the mean and its neighbours, subnormals and the largest values.  With a variance of 1e20
    the forward quotient of a subnormal underflows to -0.0, which the map keeps only because it adds MINUS zero."""
    mean, var = STATISTICS[stats]
    width = 12
    norm = sc.fitted(mean, var, aggregate=np.ndim(mean) == 0)
    chain = WRAPS[wrap](norm)
    values = sc.probe_values(np.random.RandomState(len(stats) + 7 * len(wrap)), mean, width)
    for inverse, transform in ((False, chain), (True, chain.Inverse)):
        fmap = field_map(transform, width, normalize=True)
        assert (fmap.start, fmap.stride, fmap.width) == (0, 1, width) and tuple(fmap.coef.shape) == (4, width)
        assert fmap.coef.dtype == torch.float32 and fmap.coef.is_contiguous()
        with np.errstate(all="ignore"):
            want = transform(torch.from_numpy(values)).numpy()
            got = fmap.apply_numpy(values)
        assert got.dtype == np.float32 and got.shape == want.shape
        assert got.tobytes() == want.tobytes(), (inverse, np.argwhere(got.view(np.int32) != want.view(np.int32))[:4])
    forward = field_map(chain, width, normalize=True).coef
    assert np.signbit(forward[3].numpy()).all() and not np.signbit(field_map(chain.Inverse, width, normalize=True).coef[0].numpy()).any()
    if stats.endswith("wide"):             # the corner is in the probe: -1e-45 / 1e10 is -0.0 and stays -0.0
        out = field_map(chain, width, normalize=True).apply_numpy(np.full((1, 1, width), -1e-45, np.float32))
        assert (out == 0).all() and np.signbit(out).all()


def test_a_sensor_after_the_frozen_normalize_thins_its_columns():
    norm = sc.fitted(np.linspace(-1.0, 1.0, 8), np.linspace(0.5, 4.0, 8), aggregate=False)
    chain = T.Operation([norm, T.BatchTransform(T.SensorTransform(stride=2))])
    fmap = field_map(chain, 8, normalize=True)
    assert (fmap.start, fmap.stride, fmap.width) == (1, 2, 4)
    values = np.random.RandomState(0).standard_normal((5, 1, 8)).astype(np.float32)
    assert fmap.apply_numpy(values).tobytes() == chain(torch.from_numpy(values)).numpy().tobytes()


def test_an_unfrozen_or_unfitted_normalize_is_refused_as_before():
    unfrozen = sc.fitted(0.1, 2.0, frozen=False)
    unfitted = T.Normalize(aggregate=True, batched=True, frozen=True)
    half = sc.fitted(0.1, 2.0)
    half.var = None
    for norm in (unfrozen, unfitted, half):
        for wrap in WRAPS.values():
            for asked in (False, True):
                with pytest.raises(Unrecognized) as e:
                    field_map(wrap(norm), 8, normalize=asked)
                assert str(e.value) == "a Normalize"
                with pytest.raises(Unrecognized) as e:
                    field_map(wrap(norm).Inverse, 8, normalize=asked)
                assert str(e.value) == "the inverse of a Normalize"
        with pytest.raises(Unrecognized):
            flatten(norm, normalize=True)
    # what else refuses stays: statistics of another shape or dtype, two scalings in a row
    with pytest.raises(Unrecognized, match="not one value or one per column"):
        field_map(sc.fitted(np.zeros(3), np.ones(3), aggregate=False), 8, normalize=True)
    double = sc.fitted(0.0, 1.0)
    double.mean = double.mean.double()
    with pytest.raises(Unrecognized, match="float64"):
        field_map(double, 8, normalize=True)
    with pytest.raises(Unrecognized, match="two scalings in a row"):
        field_map(T.Operation([sc.fitted(0.0, 1.0), T.ScaleTransform(bounds=(-1.0, 1.0), frozen=True)]), 8, normalize=True)


def test_only_the_callers_that_ask_take_a_frozen_normalize():
    """``flatten`` / ``field_map`` take a frozen, fitted ``Normalize`` only with ``normalize=True``, which
    ``world_connector`` and the validation loss pass.  Every other reader of a chain -- the collection stack, the stack of
    the imagined rollouts, the policy phase's connectors, the delta phase -- calls them without it and refuses the
    transform by the words it always had."""
    from pdecontrol.mbrl import delta_phase
    from pdecontrol.mbrl.recognition import action_maps
    norm = sc.fitted(0.3, 1.7)
    for wrap in WRAPS.values():
        with pytest.raises(Unrecognized) as e:
            field_map(wrap(norm), 8)
        assert str(e.value) == "a Normalize"
        with pytest.raises(Unrecognized) as e:
            flatten(wrap(norm).Inverse)
        assert str(e.value) == "the inverse of a Normalize"
    env = sc.toy_env()
    with pytest.raises(Unrecognized, match="a Normalize"):
        action_maps([norm], env.forcing, [])
    assert action_maps([norm], env.forcing, [sc.fitted(0.0, 2.0)], normalize=True)[2].coef is not None

    class Replay:                                    # what _kernel_tier reads before it asks for the device
        tensors, ntimesteps, obs_width = (), 5, 8
    with pytest.raises(Unrecognized) as e:
        delta_phase._kernel_tier(Replay(), T.SampleTransform(norm, None).otransf, T.Normalize(aggregate=True, batched=True))
    assert str(e.value) == "a Normalize"


def test_inverse_map_and_the_statistics_rule_are_untouched():
    """``inverse_map`` keeps its kind 2 for a Normalize, frozen or not; a frozen one never counts as updating."""
    from types import SimpleNamespace
    from pdecontrol.mbrl.recognition import updates_statistics
    for frozen in (False, True):
        norm = sc.fitted(0.3, 1.7, frozen=frozen)
        kind, coef = inverse_map(T.SampleTransform(norm, None).otransf.Inverse, 8)
        assert kind == 2 and torch.equal(coef[0], torch.sqrt(norm.var + norm.epsilon).reshape(1).expand(8))
        assert torch.equal(coef[1], norm.mean.reshape(1).expand(8))
    assert not updates_statistics(SimpleNamespace(frozen=False, transform=sc.fitted(0.3, 1.7)))


@pytest.mark.parametrize("untransformed", (False, True))
def test_world_connector_takes_the_offline_connector(untransformed):
    env = sc.toy_env()
    rs = np.random.RandomState(4)
    data = (rs.standard_normal((5, 4, 1, 64)).astype(np.float32), rs.uniform(-1, 1, (5, 4, 1, 4)).astype(np.float32),
            rs.standard_normal((5, 4, 1, 64)).astype(np.float32))
    fit = ev.fit_scalings(data, [0, 2, 3], env.forcing, 0.25, untransformed=untransformed)
    obs_map, (act_in, matrix, act_out) = world_connector(fit.stransf, 64, 4)
    obs = torch.from_numpy(data[0][1])
    assert obs_map.apply_numpy(obs.numpy()).tobytes() == fit.oscaling(obs).numpy().tobytes()
    acts = torch.from_numpy(data[1][1])
    assert act_in.coef is None and act_in.width == 4
    if untransformed:
        assert matrix is None and act_out.width == 4
        assert act_out.apply_numpy(acts.numpy()).tobytes() == fit.stransf.atransf(acts).numpy().tobytes()
    else:
        assert torch.equal(matrix, env.forcing.forcing) and act_out.width == 64
        forced = T.BatchTransform(env.forcing)(acts)
        assert act_out.apply_numpy(forced.numpy()).tobytes() == fit.stransf.atransf(acts).numpy().tobytes()
    # the same connector before it is frozen is what today's tests pin: refused
    for scaling in fit[:4]:
        scaling.frozen = False
    with pytest.raises(Unrecognized) as e:
        world_connector(fit.stransf, 64, 4)
    assert str(e.value) == "a Normalize"


# ----------------------------------------------------------------------------------------------------------------------
# folds
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (3, 5))
@pytest.mark.parametrize("n", (7, 10, 33, 90))
def test_kfold_indices_is_sklearns_draw(n, k):
    for seed in (0, 4):
        folds = ev.kfold_indices(n, k, seed)
        # the stated rule, written out again
        order = np.arange(n)
        np.random.RandomState(seed).shuffle(order)
        sizes = [n // k + (1 if i < n % k else 0) for i in range(k)]
        assert len(folds) == k
        start = 0
        for (train, test), size in zip(folds, sizes):
            want = np.sort(order[start:start + size])
            assert np.array_equal(test, want) and np.array_equal(train, np.setdiff1d(np.arange(n), want))
            start += size
        rule = ev._kfold_rule(n, k, seed)
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(rule, folds))
        try:
            from sklearn.model_selection import KFold
        except ImportError:
            continue
        for (train, test), (sk_train, sk_test) in zip(folds, KFold(k, shuffle=True, random_state=seed).split(np.arange(n))):
            assert np.array_equal(train, sk_train) and np.array_equal(test, sk_test)


def test_fold_split_and_total_at_hand_computed_sizes():
    idx = np.arange(100, 172)                                           # 72 train episodes of a 5-fold split of 90
    train, val = ev.fold_split(idx, 0.2)
    assert len(train) == 58 and len(val) == 14 and train[0] == 100 and val[0] == 158       # ceil(0.8 * 72) = 58
    assert [len(ev.fold_split(np.arange(n), v)[0]) for n, v in ((3, 0.34), (5, 0.2), (4, 0.5), (7, 0.0), (1, 0.2))] == [2, 4, 2, 7, 1]
    assert [ev.total_count(t, 100) for t in (0.9, 0.3, 1.0, 0.005)] == [90, 30, 100, 1] and ev.total_count(0.5, 7) == 4
    with pytest.raises(ValueError):
        ev._kfold_rule(3, 4, 0)


# ----------------------------------------------------------------------------------------------------------------------
# rpn_moments: header, binding, refusals
# ----------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_fit_entries():
    names = declared_functions(os.path.join("replay", "fit.h"), "rpn")
    assert names == ["rpn_moments", "rpn_workspace_doubles"] == sorted(n for n, _, _ in replay_hip.FIT_SYMBOLS)
    assert not [n for n, _, _ in replay_hip.SYMBOLS + replay_hip.DELTA_SYMBOLS if n.startswith("rpn_")]
    assert not declared_functions("replay_hip.h", "rpn")
    rows = {name: (res, args) for name, res, args in replay_hip.FIT_SYMBOLS}
    res, args = rows["rpn_moments"]
    assert res is ctypes.c_int and len(args) == 13 and args[3] is ctypes.c_long and args[8] is ctypes.c_long
    assert rows["rpn_workspace_doubles"] == (ctypes.c_long, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_long, ctypes.c_int])
    header = open(os.path.join(os.path.dirname(LIBDIR), "..", "include", "replay", "fit.h")).read()
    assert '#include "../replay_hip.h"' in header and f"{replay_hip.FIT_LAUNCH_FAILURE} launch failure" in header
    assert os.path.exists(os.path.join(LIBDIR, "libreplay_hip.so")), "libreplay_hip.so not built (run __graft_entry__.build())"
    lib = replay_hip.load()
    assert lib.rpn_moments.argtypes == args and lib.rpn_workspace_doubles.restype is ctypes.c_long


def test_the_fit_workspace_and_layout_are_host_functions():
    ws, G = replay_hip.fit_workspace_doubles, replay_hip.MAX_DELTA_GROUPS
    assert ws(64, 4, True, 1) == 2 * 132 and ws(64, 4, False, 16) == 2 * 68 and ws(64, 4, True, 17) == 2 * 2 * 132
    assert ws(98, 16, True, 513) == (33 + 2) * 2 * 212 and ws(256, 1, False, 4099) == (257 + 9) * 2 * 257
    assert ws(64, 4, True, 10 ** 6) == (G + G // 32) * 2 * 132 and ws(1024, 16, True, 7, 3) == 3 * 2 * 2064
    assert ws(0, 4, True, 5) == ws(1025, 4, True, 5) == ws(64, 0, True, 5) == ws(64, 17, True, 5) == ws(64, 4, True, 0) == 0
    assert ws(64, 4, True, 5, -1) == 0
    assert replay_hip.fit_layout(64, 4, True) == ((0, 65, 70), 135) and replay_hip.fit_layout(98, 16, False) == ((0, 99, 116), 116)


def test_rpn_moments_refuses_before_any_device_call():
    """Every code, with pointers that are never dereferenced and no device in the process."""
    lib = replay_hip.load()
    fake = ctypes.c_void_p(64)
    good = dict(stream=None, obs=fake, actions=fake, slab_rows=10, N=64, A=4, F=fake, rows=None, n=5, groups=0, workspace=fake,
                sums=fake, stats=fake)
    cases = {"NULL obs": (dict(obs=None), -90), "NULL actions": (dict(actions=None), -90), "NULL workspace": (dict(workspace=None), -90),
             "NULL sums": (dict(sums=None), -90), "NULL stats": (dict(stats=None), -90), "n = 0": (dict(n=0), -91),
             "no slab rows": (dict(slab_rows=0), -92), "N = 0": (dict(N=0), -93), "N too wide": (dict(N=1025), -93),
             "A = 0": (dict(A=0), -94), "A too wide": (dict(A=17), -94), "groups -1": (dict(groups=-1), -95)}
    texts = {}
    for what, (change, code) in cases.items():
        a = {**good, **change}
        assert lib.rpn_moments(*a.values()) == code, what
        texts[what] = replay_hip.last_error()
        assert texts[what].startswith("rpn_moments:"), (what, texts[what])
    assert len({texts[k] for k in ("NULL obs", "n = 0", "no slab rows", "N too wide", "A too wide", "groups -1")}) == 6
    assert "1025" in texts["N too wide"] and "17" in texts["A too wide"] and "-1" in texts["groups -1"]
    t = torch.zeros(4, 1, 8)
    with pytest.raises(replay_hip.ReplayHipError, match="rpn_moments: action width 17") as e:
        replay_hip.fit_moments(None, t, torch.zeros(4, 1, 17), None, None, 4, 0, torch.zeros(64, dtype=torch.float64),
                               torch.zeros(2, 27, dtype=torch.float64), torch.zeros(2, 27))
    assert e.value.code == -94


# ----------------------------------------------------------------------------------------------------------------------
# the numpy twin
# ----------------------------------------------------------------------------------------------------------------------
def test_the_fp32_fma_of_the_twin_rounds_once():
    """Against exact rational arithmetic on values chosen to sit on rounding boundaries, and on random ones."""
    from fractions import Fraction
    rs = np.random.RandomState(1)
    a = np.concatenate([rs.standard_normal(300), [1 + 2.0 ** -12, 3.0, 1e-20, 1.0]]).astype(np.float32)
    b = np.concatenate([rs.standard_normal(300), [1 + 2.0 ** -12, 1 / 3, 1e-20, 2.0 ** -24]]).astype(np.float32)
    c = np.concatenate([rs.standard_normal(300) * 1e-3, [2.0 ** -24, -1.0, 1.0, 1.0]]).astype(np.float32)
    got = ev._fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        err = abs(Fraction(float(g)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), (x, y, z, g)
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):      # a tie goes to even
            assert int(np.float32(g).view(np.int32)) % 2 == 0 or exact == Fraction(float(g)), (x, y, z, g)


@pytest.mark.parametrize("aggregate", (True, False))
def test_the_twin_against_normalize_update(aggregate):
    """``field_moments_numpy`` against ``Normalize.update`` on torch CPU tensors for the three fields, means and variances
    at rtol 1e-6 with no absolute term on the means (torch's fp32 reductions are the looser side), the layout the kernel
    documents, a row list and a bad row.  A relative bound on an fp32 sum can hold only where the terms do not cancel, so
    the observations lie around 2 and the actions are positive (the env's forcing matrix has no negative entry and no empty column), and the test
    first asserts on the twin's rows that no column of any field, and no field as a whole, cancels below a half."""
    env = sc.toy_env()
    F = env.forcing.forcing.numpy()
    assert (F >= 0).all() and (F.max(axis=0) > np.finfo(np.float32).tiny).all()      # nothing negative, no empty column
    rs = np.random.RandomState(8)
    n, N, A = 300, 64, 4
    obs = (2.0 + 0.5 * rs.standard_normal((n + 20, 1, N))).astype(np.float32)
    actions = rs.uniform(0.2, 1.0, (n + 20, 1, A)).astype(np.float32)
    rows = rs.permutation(n + 20)[:n]
    forced = T.BatchTransform(env.forcing)(torch.from_numpy(actions[rows]))
    for field in (obs[rows], actions[rows], ev.forced_numpy(actions[rows], F), forced.numpy()):
        assert sc.cancellation(field) >= 0.5, sc.cancellation(field)
    sums, stats = ev.field_moments_numpy(obs, actions, F, rows)
    offsets, ld = replay_hip.fit_layout(N, A, True)
    assert sums.shape == stats.shape == (2, ld) and sums.dtype == stats.dtype == np.float64
    # torch's matmul and the fma chain round single products differently: elementwise a few ulp
    np.testing.assert_allclose(ev.forced_numpy(actions[rows], F), forced.numpy(), rtol=1e-6)
    for values, first, width in ((torch.from_numpy(obs[rows]), offsets[0], N), (torch.from_numpy(actions[rows]), offsets[1], A),
                                 (forced, offsets[2], N)):
        norm = T.Normalize(aggregate=aggregate, batched=True)
        norm.update(values)
        cols = slice(first + width, first + width + 1) if aggregate else slice(first, first + width)
        np.testing.assert_allclose(norm.mean.numpy().reshape(-1), stats[0, cols], rtol=1e-6, atol=0)
        # the forcing is a Gaussian: far from an actuator its columns have variances below fp32's normal range (1e-46),
        # where torch's fp32 result has fewer than 24 bits or is flushed and no relative bound can hold; atol = the
        # smallest normal fp32 value takes exactly those out and nothing else (every other variance is above 1e-30)
        np.testing.assert_allclose(norm.var.numpy().reshape(-1), stats[1, cols], rtol=1e-6, atol=float(np.finfo(np.float32).tiny))
        v = values.numpy().astype(np.float64).reshape(n, width)
        np.testing.assert_allclose(sums[0, first:first + width], v.sum(0), rtol=1e-12 if values is not forced else 1e-6)
        np.testing.assert_allclose(sums[1, first + width], (v * v).sum(), rtol=1e-12 if values is not forced else 1e-6)
    short = ev.field_moments_numpy(obs, actions, None, rows)
    assert short[0].shape == (2, N + A + 2) and np.array_equal(short[1], stats[:, :N + A + 2])
    one = ev.field_moments_numpy(obs, actions, F, rows[:1])[1]
    totals = np.asarray([first + width for first, width in zip(offsets, (N, A, N))])      # m = width there: a variance exists
    assert np.isnan(np.delete(one[1], totals)).all() and np.isfinite(one[1][totals]).all() and np.isfinite(one[0]).all()
    bad = rows.copy()
    bad[5] = n + 20
    assert all(np.isnan(part).all() for part in ev.field_moments_numpy(obs, actions, F, bad))


# ----------------------------------------------------------------------------------------------------------------------
# fit_scalings, host tier
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("numpy", "torch"))
def test_fit_scalings_host_tier_is_the_references_lines(kind):
    env = sc.toy_env()
    rs = np.random.RandomState(2)
    E, S, N, A = 7, 5, 64, 4
    fields = [(0.2 + rs.standard_normal((E, S, 1, N))).astype(np.float32), rs.uniform(-1, 1, (E, S, 1, A)).astype(np.float32)]
    fields.append((fields[0] + 0.05 * rs.standard_normal((E, S, 1, N))).astype(np.float32))
    data = fields if kind == "numpy" else [torch.from_numpy(f) for f in fields]
    train_idx, delta = np.asarray([4, 0, 5, 2]), 0.25
    fit = ev.fit_scalings(data + [None] * 4, train_idx, env.forcing, delta)
    assert fit.tier == "host" and fit.tier_reason is None

    # the reference's lines (evaluate.py:86-112), restated
    oscaling = T.Normalize(aggregate=True, batched=True)
    ascaling = T.Normalize(aggregate=True, batched=True)
    forcing = T.BatchTransform(env.forcing)
    pdescaling = T.Normalize(aggregate=True, batched=True)
    undscaling = T.Normalize(aggregate=True, batched=True)
    obs, actions, nxtobs = (f[train_idx] for f in data)
    obs, actions, nxtobs = (f.reshape(f.shape[0] * f.shape[1], f.shape[2], f.shape[3]) for f in (obs, actions, nxtobs))
    oscaling.update(obs)
    ascaling.update(actions)
    pdescaling.update(forcing(actions))
    deltas = oscaling(nxtobs) - oscaling(obs)
    undscaling.update(deltas / delta)

    for got, want in zip(fit[:4], (oscaling, ascaling, pdescaling, undscaling)):
        assert got.frozen and got.aggregate and got.batched and got.count == want.count == 4 * S
        assert sc.same_bits(got.mean, want.mean) and sc.same_bits(got.var, want.var) and tuple(got.mean.shape) == (1, 1, 1)
        before = got.mean
        got.update(torch.zeros(3, 1, 4))                            # frozen: nothing moves
        assert got.mean is before and got.count == 4 * S
    assert type(fit.stransf) is T.SampleTransform and fit.stransf.otransf.transforms == [fit.oscaling]
    (chain,) = fit.stransf.atransf.transforms
    assert type(chain) is T.Operation and chain.transforms[0].transform is env.forcing and chain.transforms[1] is fit.pdescaling
    other = ev.fit_scalings(data + [None] * 4, train_idx, env.forcing, delta, untransformed=True)
    assert other.stransf.atransf.transforms == [other.ascaling] and sc.same_bits(other.ascaling.mean, ascaling.mean)


# ----------------------------------------------------------------------------------------------------------------------
# the dataset and the command line on the CPU twin
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy_data(tmp_path_factory):
    from torch.utils.data import TensorDataset
    data = sc.toy_dataset()
    path = tmp_path_factory.mktemp("offline") / "data.pl"
    torch.save(TensorDataset(*data.tensors), path)
    return data, path


def test_generate_dataset_on_the_cpu_twin(toy_data):
    data, _ = toy_data
    obs, actions, nxt, rewards, terminated, truncated, steps = data.tensors
    E, S = sc.EPISODES, 4
    assert data.tier == "loop" and len(data) == E
    assert [tuple(t.shape) for t in data.tensors] == [(E, S, 1, 64), (E, S, 1, 4), (E, S, 1, 64), (E, S), (E, S), (E, S), (E, S)]
    assert [t.dtype for t in data.tensors] == [torch.float32] * 4 + [torch.bool] * 2 + [torch.long]
    assert torch.equal(steps, torch.arange(S).repeat(E, 1)) and not terminated.any()
    assert truncated[:, -1].all() and not truncated[:, :-1].any()
    assert torch.equal(nxt[:, :-1], obs[:, 1:]) and torch.isfinite(nxt).all() and (rewards < 0).all()
    assert (actions.abs() <= 1).all() and len({tuple(a.reshape(-1).tolist()) for a in actions}) == E
    again = sc.toy_dataset(tier="loop")
    assert all(torch.equal(a, b) for a, b in zip(data.tensors, again.tensors))
    other = sc.toy_dataset(seed=6)
    assert not torch.equal(other.tensors[0], obs)
    with pytest.raises(ValueError):
        sc.toy_dataset(tier="kernel")


def _fold_record(directory):
    out = {}
    for name in sorted(os.listdir(directory)):
        path = os.path.join(directory, name)
        if name.endswith(".json"):
            record = json.load(open(path))
            record.pop("Training Time")
            out[name] = json.dumps(record, sort_keys=True)
        elif name.endswith(".npz"):
            out[name] = {k: (v.dtype, v.shape, v.tobytes()) for k, v in np.load(path).items()}
        elif name.endswith(".pt"):
            saved = torch.load(path, weights_only=False)
            out[name] = {k: v.numpy().tobytes() for k, v in saved["state_dict"].items()}
            out[name].update({k: (saved[k].mean.numpy().tobytes(), saved[k].var.numpy().tobytes(), saved[k].frozen)
                              for k in ("oscaling", "ascaling", "pdescaling", "undscaling")})
    return out


def test_main_end_to_end_and_reproducible(toy_data, tmp_path):
    """Six four-step episodes, two folds, one epoch each: the reports exist and hold what a fold computes; a second run
    from the same seed writes the same bits (the seconds aside)."""
    _, path = toy_data
    records = []
    for run in ("a", "b"):
        out = tmp_path / run
        assert ev.main(sc.toy_argv(path, out) + ["--store"], make_env=sc.toy_env) == 0
        assert sorted(os.listdir(out)) == ["fold0.json", "fold0.npz", "fold0_model.pt", "fold1.json", "fold1.npz", "fold1_model.pt",
                                           "history.jsonl"]
        records.append(_fold_record(out))
    assert records[0] == records[1]
    folds = ev.kfold_indices(6, 2, 3)
    for k in range(2):
        record = json.load(open(tmp_path / "a" / f"fold{k}.json"))
        train, val = ev.fold_split(folds[k][0], 0.34)
        assert (record["train"], record["val"], record["test"]) == (list(train), list(val), list(folds[k][1]))
        assert record["tiers"] == {"fit": "host", "training": "loop", "training_reason": "a module that is not on a GPU", "test": "torch"}
        assert record["epochs"] == 1 == len(record["history"]) and record["history"][0]["global_step"] == 1
        assert math.isfinite(record["Val. Loss"]) and record["Val. Loss"] == record["history"][0]["Val. Loss"]
        assert record["config"]["training"]["target_length"] == sc.TARGET and record["config"]["trainer"]["gradient_clip_val"] == 0.5
        assert math.isfinite(record["test_scalars"]["MSE"]) and record["test_samples"] == 3          # hop tau: one window per episode
        arrays = np.load(tmp_path / "a" / f"fold{k}.npz")
        assert arrays["hsteploss"].shape == (1, sc.TAU + sc.TARGET) and arrays["states"].shape == (3, sc.TAU + sc.TARGET, 1, 64)
        assert any(name.startswith("table/") for name in arrays.files)
    assert len(open(tmp_path / "a" / "history.jsonl").read().splitlines()) == 2
    assert records[0]["fold0.json"] != records[0]["fold1.json"]
