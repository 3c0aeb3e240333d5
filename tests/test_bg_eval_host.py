"""The Burgers test-phase entries without a GPU: include/burgers/eval.h, the binding's ``EVAL_SYMBOLS`` and the built library
name the same functions; the ``*_host`` entries (the arithmetic of csrc/bg_eval.h run serially on host memory) against the
fp64 numpy restatement of tests/_bg_eval_oracle.py; every refusal, made on the host before any HIP call.

The bars: rowstats and derivatives at rtol 1e-12, atol 0.  On the white-noise rows of these cases two fp64 orderings of one
stencil differ by <= 1e-14 in every one of the 14 sums, and reordering an fp64 sum of <= 1024 terms adds about 1e-13."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bg_eval_oracle as mo  # noqa: E402
from _bg_eval_calls import Mem, batch_major, time_major  # noqa: E402
from test_capi_symbols import LIBDIR, ROOT, declared_functions  # noqa: E402

from oracle import burgers_oracle as bo  # noqa: E402
from pdegym.burgers import _hip  # noqa: E402

HEADER = os.path.join("burgers", "eval.h")
LIB = os.path.join(LIBDIR, "libburgers_hip.so")
ENTRIES = ["bg_derivatives", "bg_derivatives_host", "bg_eval_fold", "bg_eval_fold_host", "bg_eval_last_error", "bg_eval_rows",
           "bg_eval_rows_host"]


@pytest.fixture(scope="module")
def host():
    assert os.path.exists(LIB), "libburgers_hip.so not built (run __graft_entry__.build())"
    return Mem("host")


def test_the_eval_header_its_table_and_the_library_agree():
    declared = declared_functions(HEADER, "bg")
    assert declared == ENTRIES == sorted(name for name, _, _ in _hip.EVAL_SYMBOLS)
    # the pinned header and its table keep their own list
    assert not set(declared) & set(declared_functions("burgers_hip.h", "bg"))
    assert not set(declared) & {name for name, _, _ in _hip.SYMBOLS}
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "../burgers_hip.h"' in text
    for top in os.listdir(os.path.join(ROOT, "include")):          # included by nothing at top level
        if top.endswith(".h"):
            assert "burgers/eval.h" not in open(os.path.join(ROOT, "include", top)).read(), top
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    assert re.findall(r"typedef struct (\w+)", text) == ["bg_eval_batch"]
    fields = re.search(r"typedef struct bg_eval_batch \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[;,]", fields) == [name for name, _ in _hip.EvalBatch._fields_]
    assert int(re.search(r"#define BG_EVAL_ROW_STATS\s+(\d+)", text).group(1)) == _hip.EVAL_ROW_STATS == mo.ROW_STATS == 14
    assert int(re.search(r"#define BG_EVAL_TABLES\s+(\d+)", text).group(1)) == _hip.EVAL_TABLES == mo.TABLES == 20
    assert list(_hip.EVAL_TABLE_NAMES) == mo.TABLE_NAMES and len(mo.TABLE_NAMES) == 20
    assert os.path.exists(LIB), "libburgers_hip.so not built (run __graft_entry__.build())"
    lib = _hip.load()
    for name, restype, argtypes in _hip.SYMBOLS + _hip.EVAL_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


@pytest.mark.parametrize("shape", mo.SHAPES, ids=lambda s: "N%d-B%d-T%d" % s)
def test_rows_host_against_the_numpy_restatement(host, shape):
    """Through a non-trivial kind-1 map and a shifted, time-major prediction."""
    c = mo.case(shape)
    stats, t_out, p_out = host.case_rows(c)
    np.testing.assert_array_equal(t_out, c["s"])
    np.testing.assert_array_equal(p_out, c["o"])
    np.testing.assert_allclose(stats, c["stats"], rtol=1e-12, atol=0)
    # without the outputs: the same sums
    again, _, _ = host.case_rows(c, outs=False)
    np.testing.assert_array_equal(again, stats)


def test_fold_host_against_the_restated_fold(host):
    for shape in ((64, 1, 4), (64, 3, 7), (100, 3, 7)):
        n, b, t = shape
        c = mo.case(shape)
        got = host.fold(c["stats"], b, t, n)
        assert got.shape == (1 + 20 * t,)
        np.testing.assert_allclose(got, c["tables"], rtol=1e-12, atol=0)
        accum = host.up(np.zeros(1 + mo.TABLES * t))
        first = host.fold(c["stats"], b, t, n, accum)
        second = host.fold(c["stats"], b, t, n, accum)
        np.testing.assert_array_equal(first, got)
        np.testing.assert_array_equal(second, got)
        np.testing.assert_array_equal(accum, 2 * b * got)
    # a zero truth row: 0 / 0 and x / 0 exactly where numpy (and the host lines of test_step) give them
    n, b, t = 64, 2, 3
    truth, pred = (v.copy() for v in mo.noise_rows(n, b, t, seed=11))
    truth[1, 2] = 0.0                      # x / 0
    truth[0, 0] = pred[0, 0] = 0.0         # 0 / 0
    stats, _, _ = host.rows(truth, pred, batch_major(b, t, n), batch_major(b, t, n), b, t, n, mo.L / n)
    np.testing.assert_allclose(stats, mo.row_stats(truth, pred, mo.L / n), rtol=1e-12, atol=0)
    want, got = mo.fold(stats, n), host.fold(stats, b, t, n)
    assert np.isinf(want).any() and np.isnan(want).any() and not np.isfinite(want[1 + 2 * t + 2])
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
    ok = np.isfinite(want)
    np.testing.assert_allclose(got[ok], want[ok], rtol=1e-12, atol=0)


def test_outputs_have_the_bits_of_the_torch_inverse(host):
    """Kinds 1 and 2: ``truth_out`` / ``pred_out`` equal ``stransf.otransf.Inverse`` computed by torch on the host."""
    from pdecontrol.mbrl.recognition import inverse_map
    from pdegym.common import transforms as T
    n, b, t = 64, 3, 7
    raw, other = mo.noise_rows(n, b, t, seed=3)
    raw_t = torch.from_numpy(raw.reshape(b * t, 1, n).copy())
    scale = T.ScaleTransform(scale=(-1.0, 1.0))
    scale.update(raw_t)
    chain = T.Operation([T.BatchTransform(scale)])
    norm = T.Normalize(aggregate=False, batched=False)
    norm.update(raw_t)
    for expect, forward, inverse in ((1, chain, chain.Inverse), (2, norm, norm.Inverse)):
        kind, coef = inverse_map(inverse, n)
        assert kind == expect and tuple(coef.shape) == ({1: 4, 2: 2}[kind], n)
        rows = forward(raw_t).reshape(b, t, n).numpy()
        rows2 = forward(torch.from_numpy(other.reshape(b * t, 1, n).copy())).reshape(b, t, n).numpy()
        want = inverse(torch.from_numpy(rows.reshape(b * t, 1, n).copy())).numpy().reshape(b, t, n)
        want2 = inverse(torch.from_numpy(rows2.reshape(b * t, 1, n).copy())).numpy().reshape(b, t, n)
        _, t_out, p_out = host.rows(rows, rows2, batch_major(b, t, n), batch_major(b, t, n), b, t, n, mo.L / n, kind=kind,
                                    coef=coef.numpy(), outs=True)
        np.testing.assert_array_equal(t_out, want)
        np.testing.assert_array_equal(p_out, want2)
        restated = mo.affine_inverse if kind == 1 else mo.normalize_inverse
        np.testing.assert_array_equal(t_out, restated(rows, coef.numpy()))


def test_shift_over_time_major_equals_the_concatenated_layout(host):
    c = mo.case((64, 3, 7))
    n, b, t = c["n"], c["b"], c["t"]
    s1, t1, p1 = host.case_rows(c)
    s2, t2, p2 = host.rows(c["truth"], mo.shifted(c["truth"], c["pred"]), batch_major(b, t, n), batch_major(b, t, n), b, t, n,
                           c["dx"], shift=0, kind=1, coef=c["coef"], outs=True)
    np.testing.assert_array_equal(s1, s2)
    np.testing.assert_array_equal(t1, t2)
    np.testing.assert_array_equal(p1, p2)
    np.testing.assert_array_equal(host.fold(s1, b, t, n), host.fold(s2, b, t, n))
    for j in (0, 1, 6, 7, 10, 11):
        assert np.all(s1[:, 0, j] == 0.0), j
    assert np.all(s1[:, 1:, 0] > 0.0)
    assert np.array_equal(s1[:, 0, 4], s1[:, 0, 5])


@pytest.mark.parametrize("shape", mo.SHAPES, ids=lambda s: "N%d-B%d-T%d" % s)
def test_derivatives_host_against_the_oracle(host, shape):
    c = mo.case(shape)
    u = c["truth"].reshape(-1, c["n"])
    ux, uxx = host.derivatives(u, c["dx"])
    np.testing.assert_allclose(ux, bo.grad(u.astype(np.float64), c["dx"], dtype=np.float64), rtol=1e-12, atol=0)
    np.testing.assert_allclose(uxx, bo.laplace(u.astype(np.float64), c["dx"], dtype=np.float64), rtol=1e-12, atol=0)


FAKE = 4096        # stands in for every device pointer: a refusal that read it would fault


def test_every_refusal_is_made_on_the_host():
    """By message prefix, with no GPU present: the device entries are given pointers that must never be read and a NULL
    stream that must never be launched on."""
    if not os.path.exists(LIB):
        pytest.skip("libburgers_hip.so not built (run __graft_entry__.build())")
    lib = _hip.load()
    N, B, T, dx = 64, 2, 3, mo.L / 64
    p = ctypes.c_void_p

    def batch(**change):
        fields = dict(truth=FAKE, truth_bstride=T * N, truth_tstride=N, pred=2 * FAKE, pred_bstride=T * N, pred_tstride=N,
                      pred_shift=0, inv_kind=0, inv_coef=None, truth_out=None, pred_out=None)
        fields.update(change)
        return ctypes.byref(_hip.EvalBatch(**fields))

    stats, tables, u, ux, uxx = p(3 * FAKE), p(4 * FAKE), p(5 * FAKE), p(6 * FAKE), p(7 * FAKE)
    entries = {
        "bg_eval_rows": lambda *a: lib.bg_eval_rows(None, *a), "bg_eval_rows_host": lib.bg_eval_rows_host,
        "bg_eval_fold": lambda *a: lib.bg_eval_fold(None, *a), "bg_eval_fold_host": lib.bg_eval_fold_host,
        "bg_derivatives": lambda *a: lib.bg_derivatives(None, *a), "bg_derivatives_host": lib.bg_derivatives_host,
    }

    def refused(name, *args):
        rc = entries[name](*args)
        message = lib.bg_eval_last_error().decode()
        assert rc == -1, (name, rc, message)
        assert message.startswith(name + ":"), (name, message)
        return message

    for name in ("bg_eval_rows", "bg_eval_rows_host"):
        texts = [refused(name, None, B, T, N, dx, stats), refused(name, batch(truth=None), B, T, N, dx, stats),
                 refused(name, batch(pred=None), B, T, N, dx, stats), refused(name, batch(), B, T, N, dx, None),
                 refused(name, batch(), 0, T, N, dx, stats), refused(name, batch(), B, 0, N, dx, stats),
                 refused(name, batch(truth_bstride=4, truth_tstride=4, pred_bstride=4, pred_tstride=4), B, T, 4, dx, stats)]
        for bad in (0.0, -dx, float("inf"), float("nan")):
            texts.append(refused(name, batch(), B, T, N, bad, stats))
        for kind in (-1, 3):
            texts.append(refused(name, batch(inv_kind=kind, inv_coef=8 * FAKE), B, T, N, dx, stats))
        for kind in (1, 2):
            texts.append(refused(name, batch(inv_kind=kind), B, T, N, dx, stats))
        for shift in (-1, 2):
            texts.append(refused(name, batch(pred_shift=shift), B, T, N, dx, stats))
        for field in ("truth_bstride", "truth_tstride", "pred_bstride", "pred_tstride"):
            for stride in (N - 1, 0, -N):
                texts.append(refused(name, batch(**{field: stride}), B, T, N, dx, stats))
        for out in ("truth_out", "pred_out"):
            for source in (FAKE, 2 * FAKE):
                texts.append(refused(name, batch(**{out: source}), B, T, N, dx, stats))
        assert len(set(texts)) >= 9
    for name in ("bg_eval_fold", "bg_eval_fold_host"):
        refused(name, None, B, T, N, tables, None)
        refused(name, stats, B, T, N, None, None)
        refused(name, stats, 0, T, N, tables, None)
        refused(name, stats, B, 0, N, tables, None)
        refused(name, stats, B, T, 4, tables, None)
    for name in ("bg_derivatives", "bg_derivatives_host"):
        refused(name, None, B, N, dx, ux, uxx)
        refused(name, u, B, N, dx, None, uxx)
        refused(name, u, B, N, dx, ux, None)
        refused(name, u, 0, N, dx, ux, uxx)
        refused(name, u, B, 4, dx, ux, uxx)
        for bad in (0.0, -dx, float("inf"), float("nan")):
            refused(name, u, B, N, bad, ux, uxx)
    # the binding raises with the same text
    with pytest.raises(_hip.BurgersHipError, match="bg_eval_fold_host: NULL"):
        _hip.check_eval(lib.bg_eval_fold_host(None, B, T, N, tables, None))


def test_host_lines_take_two_derivatives():
    """``test_step``'s host lines on a CPU module whose env hands out two derivatives (a bare Burgers env with ``rhs`` from
    the numpy oracle): exactly the 20 table names plus MSE, states, outputs and actions, the tables those of the fp64
    restatement at the bar of the torch tier (rtol 2e-4, atol 2e-5: fp32 sums over N = 64); ``test_surrogate`` folds them."""
    import types

    import _burgers_world_scenario as bw
    import _rollout_scenario as rsc
    from pdecontrol.architectures.fno import BurgersFNO
    from pdecontrol.surrogates import test_phase
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.common import transforms as tr
    n, b, t, tau = 64, 3, 7, 3
    env = bw.bare_env(1, N=n, cfg_steps=50, Tmax=10.0)
    f64 = lambda u: np.asarray(u, dtype=np.float32).astype(np.float64)
    env.rhs = lambda u, phi=None: (bo.residual(u, env.dx, env.nu, phi),
                                   (bo.grad(f64(u), env.dx, dtype=np.float64), bo.laplace(f64(u), env.dx, dtype=np.float64)))
    tf = rsc.transforms(types.SimpleNamespace(T=tr), types.SimpleNamespace(action_space=env.single_action_space,
                                                                           forcing=env.forcing))
    tstep = env.cfg_steps * env.dt
    torch.manual_seed(0)
    f = BurgersFNO()
    sur = f.surrogate(delta=tstep, dscaling=None, tau=tau, **f.model())
    module = PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=tstep, delta=tstep, env=env,
                               stransf=tf.replay_to_world, tau=tau, tbtt=10)
    rs = np.random.RandomState(3)
    raw = torch.from_numpy(rs.uniform(-1.0, 1.0, (b * t, 1, n)).astype(np.float32))
    acts = torch.from_numpy(rs.uniform(-1.0, 1.0, (b * t, 1, 4)).astype(np.float32))
    states = tf.replay_to_world.otransf(raw).reshape(b, t, 1, n)
    actions = tf.replay_to_world.atransf(acts).reshape(b, t, 1, n)
    with torch.no_grad():
        data = module.test_step((states, actions), 0)
    assert module.last_test_tier == "torch"
    assert sorted(data) == sorted(mo.TABLE_NAMES + ["MSE", "states", "outputs", "actions"]) and len(data) == 24
    s, o = data["states"][:, :, 0], data["outputs"][:, :, 0]
    want = mo.named(mo.fold(mo.row_stats(s, o, env.dx), n), t)
    for name in ["MSE"] + mo.TABLE_NAMES:
        np.testing.assert_allclose(np.asarray(data[name]), want[name], rtol=2e-4, atol=2e-5, err_msg=name)
    report = test_phase.test_surrogate(module, dataloaders=[(states[:2], actions[:2]), (states[2:], actions[2:])], nstore=2,
                                       tier="torch")
    assert (report.tier, report.batches, report.samples) == ("torch", 2, 3)
    assert sorted(report.tables) == sorted(mo.TABLE_NAMES) and report.states.shape == (2, t, 1, n)


def test_generate_dataset_names_the_burgers_env_and_refuses_the_cpu():
    import pdegym.burgers
    from pdecontrol.surrogates.evaluation.generate import generate_dataset
    with pytest.raises(ValueError, match="BurgersEnv-v0.*cpu"):
        generate_dataset(pdegym.burgers.ENV_ID, 3, config={"N": 64, "Tmax": 0.4}, device="cpu", seed=0)
    with pytest.raises(ValueError, match="built for KuramotoSivashinskyEnv-v0"):
        generate_dataset("NoSuchEnv-v0", 3)
