"""The Burgers test phase on the MI355X: ``bg_eval_rows`` / ``bg_eval_fold`` / ``bg_derivatives`` against the fp64 numpy
restatement of tests/_bg_eval_oracle.py and against their ``*_host`` twins, ``PDETrainingModule.test_step``'s kernel tier
on a Burgers env against the restatement and against its torch tier, ``test_surrogate``, ``generate_dataset`` on the
Burgers env and one ``evaluate_fold``.

Bars: rowstats at rtol 1e-12 (tests/test_bg_eval_host.py says why); the fold and the derivatives bit for bit against the
host twin (same operations in the same order, fp64, contraction off); the module's fp32 tables at rtol 1e-6 of the
restatement applied to the returned rows (the cast to fp32 is 2^-24); the torch tier at the bar tests/test_eval_rows_gpu.py
uses (rtol 2e-4, atol 2e-5)."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _bg_eval_oracle as mo  # noqa: E402
from _bg_eval_calls import Mem  # noqa: E402
from conftest import GRAD_LOG  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL, ATOL = 2e-4, 2e-5
OBSERVED = os.path.join(os.path.dirname(GRAD_LOG), "burgers_test_phase_parity_observed.jsonl")
N, B, T, TAU = 64, 3, 7, 3
KEYS = sorted(mo.TABLE_NAMES + ["MSE", "states", "outputs", "actions"])


@pytest.fixture(scope="module")
def mems():
    return Mem("cuda"), Mem("host")


@pytest.mark.parametrize("shape", mo.SHAPES, ids=lambda s: "N%d-B%d-T%d" % s)
def test_rows_against_the_restatement_and_the_host_twin(mems, shape):
    """One N per lane-group width (16 lanes up to N = 64, 32 up to 512, 64 above), an N that is no multiple of its width
    (100), last workgroups that are not full (21 and 17 rows) and the smallest N."""
    gpu, host = mems
    c = mo.case(shape)
    stats, t_out, p_out = gpu.case_rows(c)
    np.testing.assert_array_equal(t_out, c["s"])
    np.testing.assert_array_equal(p_out, c["o"])
    np.testing.assert_allclose(stats, c["stats"], rtol=1e-12, atol=0)
    twin, _, _ = host.case_rows(c)
    np.testing.assert_allclose(stats, twin, rtol=1e-12, atol=0)
    again, _, _ = gpu.case_rows(c, outs=False)
    assert again.tobytes() == stats.tobytes(), "two launches differ"


def test_fold_has_the_host_twins_bits(mems):
    gpu, host = mems
    for shape in ((64, 1, 4), (64, 3, 7), (48, 17, 1)):
        n, b, t = shape
        stats = mo.case(shape)["stats"]
        got, want = gpu.fold(stats, b, t, n), host.fold(stats, b, t, n)
        assert got.tobytes() == want.tobytes(), shape
        np.testing.assert_allclose(got, mo.case(shape)["tables"], rtol=1e-12, atol=0)
        g_acc, h_acc = gpu.up(np.zeros(1 + mo.TABLES * t)), host.up(np.zeros(1 + mo.TABLES * t))
        for _ in range(2):
            assert gpu.fold(stats, b, t, n, g_acc).tobytes() == want.tobytes()
            host.fold(stats, b, t, n, h_acc)
        assert gpu.down(g_acc).tobytes() == h_acc.tobytes()
        np.testing.assert_array_equal(h_acc, 2 * b * want)
    # zero norms: inf and nan in the same places, the same bits elsewhere
    n, b, t = 64, 2, 3
    truth, pred = (v.copy() for v in mo.noise_rows(n, b, t, seed=11))
    truth[1, 2] = 0.0
    truth[0, 0] = pred[0, 0] = 0.0
    stats = mo.row_stats(truth, pred, mo.L / n)
    got, want = gpu.fold(stats, b, t, n), host.fold(stats, b, t, n)
    assert np.isnan(want).any() and np.isinf(want).any()
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("shape", mo.SHAPES, ids=lambda s: "N%d-B%d-T%d" % s)
def test_derivatives_have_the_host_twins_bits(mems, shape):
    gpu, host = mems
    c = mo.case(shape)
    u = c["truth"].reshape(-1, c["n"])
    got, want = gpu.derivatives(u, c["dx"]), host.derivatives(u, c["dx"])
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()


# ---- the module and the epoch ----------------------------------------------------------------------------------------------
def _batches(env, stransf, sizes, steps, seed):
    """Scaled white-noise states [b, steps, 1, N] and forced, scaled uniform actions [b, steps, 1, N] on the device."""
    rs = np.random.RandomState(seed)
    out = []
    for b in sizes:
        raw = torch.from_numpy(rs.uniform(-1.0, 1.0, (b * steps, 1, N)).astype(np.float32))
        acts = torch.from_numpy(rs.uniform(-1.0, 1.0, (b * steps, 1, 4)).astype(np.float32))
        states = stransf.otransf(raw).reshape(b, steps, 1, N)
        actions = stransf.atransf(acts).reshape(b, steps, 1, N)
        out.append((states.to(env.device), actions.to(env.device)))
    return out


@pytest.fixture(scope="module")
def burgers_module():
    """N = 64: a seeded ``BurgersFNO`` surrogate under the controller's connector (a frozen ``ScaleTransform`` observation
    scaling; actions forced to full width and scaled) with ``env = BurgersBatchedVecEnv(1, N=64)``."""
    import _rollout_scenario as rsc
    from pdecontrol.architectures.fno import BurgersFNO
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.burgers import BurgersBatchedVecEnv
    from pdegym.common import transforms as tr
    env = BurgersBatchedVecEnv(1, N=N)
    tstep = env.cfg_steps * env.dt
    tf = rsc.transforms(types.SimpleNamespace(T=tr), types.SimpleNamespace(action_space=env.single_action_space,
                                                                           forcing=env.forcing))
    torch.manual_seed(0)
    f = BurgersFNO()
    sur = f.surrogate(delta=tstep, dscaling=None, tau=TAU, **f.model())
    module = PDETrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=tstep, delta=tstep, env=env,
                               stransf=tf.replay_to_world, tau=TAU, tbtt=10).to(env.device)
    module.eval()
    return module, env, tf


def _restated(states, outputs, dx):
    """The tables of the restatement from the rows a test step returned ([b, t, 1, N] fp32, already inverse-scaled)."""
    s, o = states[:, :, 0], outputs[:, :, 0]
    return mo.named(mo.fold(mo.row_stats(s, o, dx), s.shape[-1]), s.shape[1])


def _family(name):
    return "rewards" if name.endswith("_rews") else "derivatives" if "-derivative-" in name else "states"


def test_test_step_on_a_burgers_env(burgers_module):
    from pdecontrol.surrogates import ops
    module, env, tf = burgers_module
    (states, actions), = _batches(env, tf.replay_to_world, (B,), T, seed=3)
    with torch.no_grad():
        data = module.test_step((states, actions), 0)
    assert module.last_test_tier == "kernel"
    assert sorted(data) == KEYS and len(KEYS) == 24
    for name, value in data.items():
        assert isinstance(value, np.ndarray) and value.dtype == np.float32, (name, type(value))
    # the returned rows: the torch inverse of the states on the host, the initial condition in front of the prediction
    want_states = tf.replay_to_world.otransf.Inverse(states.cpu().reshape(B * T, 1, N)).numpy().reshape(B, T, 1, N)
    np.testing.assert_array_equal(data["states"], want_states)
    np.testing.assert_array_equal(data["outputs"][:, 0], data["states"][:, 0])
    assert np.isfinite(data["outputs"]).all() and not np.array_equal(data["outputs"][:, 1:], data["states"][:, 1:])
    want = _restated(data["states"], data["outputs"], env.dx)
    worst = {"kernel_vs_restatement": {}, "torch_vs_kernel": {}}
    for name in ["MSE"] + mo.TABLE_NAMES:
        dev = np.max(np.abs(data[name] - want[name]) / np.maximum(np.abs(want[name]), 1e-300))
        fam = "MSE" if name == "MSE" else _family(name)
        worst["kernel_vs_restatement"][fam] = max(worst["kernel_vs_restatement"].get(fam, 0.0), float(dev))
    print("burgers test phase parity (kernel tier vs fp64 restatement, relative)", worst["kernel_vs_restatement"])
    with ops.fused(False), torch.no_grad():
        host = module.test_step((states, actions), 0)
    assert module.last_test_tier == "torch"
    assert sorted(host) == KEYS
    host = {name: np.asarray(value) for name, value in host.items()}     # the host lines leave some tables as tensors
    for name in ["MSE"] + mo.TABLE_NAMES:
        top = float(np.max(np.abs(host[name])))
        dev = float(np.max(np.abs(np.asarray(host[name], dtype=np.float64) - data[name])) / top) if top > 0 else 0.0
        fam = "MSE" if name == "MSE" else _family(name)
        worst["torch_vs_kernel"][fam] = max(worst["torch_vs_kernel"].get(fam, 0.0), dev)
    rec = {"label": "gfx950", "shape": {"N": N, "B": B, "T": T},
           "largest_relative_deviation_kernel_tier_vs_fp64_restatement": worst["kernel_vs_restatement"],
           "largest_deviation_over_largest_entry_torch_tier_vs_kernel_tier": worst["torch_vs_kernel"],
           "bars": {"kernel_vs_restatement_rtol": 1e-6, "torch_vs_kernel": {"rtol": RTOL, "atol": ATOL}}}
    print("burgers test phase parity", json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        with open(OBSERVED, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    for name in ["MSE"] + mo.TABLE_NAMES:
        np.testing.assert_allclose(data[name], want[name], rtol=1e-6, atol=0, err_msg=name)
    for name in KEYS:
        np.testing.assert_allclose(host[name], data[name], rtol=RTOL, atol=ATOL, err_msg=name)
    # a BurgersEnv (the single-env view) is taken too
    from pdegym.burgers import BurgersEnv
    single = BurgersEnv(N=N)
    module.env = single
    try:
        with torch.no_grad():
            again = module.test_step((states, actions), 0)
        assert module.last_test_tier == "kernel"
        for name in KEYS:
            assert again[name].tobytes() == data[name].tobytes(), name
    finally:
        module.env = env


def test_rhs_hook(burgers_module):
    """``env.rhs``: the residual of ``bg_residual`` and the fp64 derivatives, for numpy and tensor rows of any leading shape."""
    from oracle import burgers_oracle as bo
    _, env, _ = burgers_module
    u = mo.noise_rows(N, 2, 3, seed=5)[0].reshape(2, 3, 1, N)
    res, (ux, uxx) = env.rhs(u)
    assert res.shape == ux.shape == uxx.shape == u.shape and res.dtype == np.float32 and ux.dtype == uxx.dtype == np.float64
    np.testing.assert_allclose(ux, bo.grad(u.astype(np.float64), env.dx, dtype=np.float64), rtol=1e-12, atol=0)
    np.testing.assert_allclose(uxx, bo.laplace(u.astype(np.float64), env.dx, dtype=np.float64), rtol=1e-12, atol=0)
    np.testing.assert_array_equal(res.reshape(-1, N), env.residual(u.reshape(-1, N)).cpu().numpy())
    phi = np.full((1, N), 0.5, dtype=np.float32)
    res_t, (ux_t, _) = env.rhs(torch.from_numpy(u).to(env.device), torch.from_numpy(phi))
    np.testing.assert_array_equal(ux_t, ux)
    np.testing.assert_array_equal(res_t.reshape(-1, N), env.residual(u.reshape(-1, N), np.broadcast_to(phi, (6, N)).copy()).cpu().numpy())


def test_test_surrogate_on_a_burgers_env(burgers_module):
    from pdecontrol.surrogates import test_phase
    module, env, tf = burgers_module
    loader = _batches(env, tf.replay_to_world, (2, 1), T, seed=4)
    reports = {}
    for tier in (None, "torch"):
        report = reports[tier] = test_phase.test_surrogate(module, dataloaders=loader, nstore=2, tier=tier)
        assert (report.tier, report.batches, report.samples) == ("kernel" if tier is None else "torch", 2, 3)
        assert report.states.shape == report.outputs.shape == (2, T, 1, N) and report.actions.shape == (2, T, 1, N)
        assert sorted(report.tables) == sorted(mo.TABLE_NAMES) and sorted(report.scalars) == ["MSE"]
    # the numpy fold's batch-size-weighted mean, from rows the kernel tier returned batch by batch
    want = {}
    with torch.no_grad():
        for states, actions in loader:
            data = module.test_step((states, actions), 0)
            for name, value in _restated(data["states"], data["outputs"], env.dx).items():
                want[name] = want.get(name, 0.0) + states.shape[0] * np.asarray(value) / 3.0
    np.testing.assert_allclose(reports[None].scalars["MSE"], want["MSE"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(reports["torch"].scalars["MSE"], want["MSE"], rtol=RTOL, atol=ATOL)
    for name in mo.TABLE_NAMES:
        np.testing.assert_allclose(reports[None].tables[name], want[name], rtol=1e-12, atol=0, err_msg=name)
        np.testing.assert_allclose(reports["torch"].tables[name], want[name], rtol=RTOL, atol=ATOL, err_msg=name)
    np.testing.assert_allclose(reports[None].states, reports["torch"].states, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(reports[None].outputs, reports["torch"].outputs, rtol=RTOL, atol=ATOL)
    s, a = loader[0]
    with pytest.raises(ValueError, match="share T"):
        test_phase.test_surrogate(module, dataloaders=[(s, a), (s[:, :5], a[:, :5])])


@pytest.fixture(scope="module")
def burgers_dataset():
    import pdegym.burgers
    from pdecontrol.surrogates.evaluation.generate import generate_dataset
    make = lambda tier: generate_dataset(pdegym.burgers.ENV_ID, 3, config={"N": N, "Tmax": 0.4}, device="cuda", seed=0, tier=tier)
    return make(None), make("loop")


def test_generate_dataset_on_the_burgers_env(burgers_dataset):
    data, loop = burgers_dataset
    assert (data.tier, loop.tier) == ("kernel", "loop")
    E, S = 3, 8
    assert len(data.tensors) == 7
    assert [tuple(t.shape) for t in data.tensors] == [(E, S, 1, N), (E, S, 1, 4), (E, S, 1, N), (E, S), (E, S), (E, S), (E, S)]
    assert [t.dtype for t in data.tensors] == [torch.float32] * 4 + [torch.bool] * 2 + [torch.long]
    for i, (a, b) in enumerate(zip(data.tensors, loop.tensors)):
        assert a.is_cuda and a.dtype == b.dtype and a.shape == b.shape
        if i != 3:
            assert torch.equal(a, b), i
    # the rewards: the kernel tier rounds one fp64 product to fp32, the loop the env's host value; (N + 4) 2^-24 relative
    r, rl = data.tensors[3].double().cpu().numpy(), loop.tensors[3].double().cpu().numpy()
    assert np.all(np.abs(r - rl) <= (N + 4) * 2.0 ** -24 * np.abs(rl))
    obs, _, nxt, rewards, terminated, truncated, steps = (t.cpu() for t in data.tensors)
    assert torch.equal(steps, torch.arange(S).repeat(E, 1)) and not terminated.any()
    assert truncated[:, -1].all() and not truncated[:, :-1].any()
    assert torch.equal(nxt[:, :-1], obs[:, 1:]) and torch.isfinite(nxt).all() and (rewards < 0).all()


def test_evaluate_fold_on_the_burgers_dataset(burgers_dataset):
    from pdecontrol.architectures.fno import BurgersFNO
    from pdecontrol.surrogates.evaluation import evaluate as ev
    from pdegym.burgers import BurgersBatchedVecEnv
    data, _ = burgers_dataset
    env = BurgersBatchedVecEnv(1, N=N, Tmax=0.4)
    factory = BurgersFNO()
    sections = {"model": {}, "surrogate": {}, "curriculum": {}, "training": dict(tau=2, tbtt=10, batch_size=4, patience=5),
                "trainer": {"max_steps": 2}}
    config = ev.merged_config(factory, "BurgersFNO", sections, "MSELoss", 4)
    torch.manual_seed(1)
    np.random.seed(1)
    report = ev.evaluate_fold(data.tensors, [0], [1], [2], env, factory, config, target_length=4, device="cuda", tier="loop")
    assert report.tiers["test"] == "kernel" and report.test.tier == "kernel"
    assert sorted(report.test.tables) == sorted(mo.TABLE_NAMES)
    assert np.isfinite(report.test.scalars["MSE"])
    for name, table in report.test.tables.items():
        assert table.shape == (6,) and np.isfinite(table).all(), name
