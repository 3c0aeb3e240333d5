"""The offline surrogate evaluation on the GPU: ``rpn_moments`` against its numpy twin over row counts,
widths, forcing, row lists, group counts and alignments; the kernel tier of ``fit_scalings``; the window gather, the
validation loss and the surrogate-update phase through the offline connector of frozen ``Normalize`` transforms;
``generate_dataset`` against its loop tier; one fold of ``main``.

Bounds.  They are the ones tests/test_delta_phase_gpu.py holds the same reduction to, for the same reasons: ``sums`` to
1e-12 of the twin's own fp64 value (an fp64 sum of n terms carries an error of a few 1e-16 of the sum of the terms'
magnitudes, so the bound holds where a column does not cancel below about 1e-4 of them; every case asserts on the twin,
before anything runs, that none cancels below 1e-3), ``stats`` within 1 ulp of the fp32 rounding of the twin's two-pass
value (the fp64 one-pass value differs from it by about 1e-10 relative at |mean| / std <= 100), and 2 ulp for statistics
that went through ``Normalize.merge`` (one more rounding, of b * n / n)."""
import itertools
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _offline_eval_scenario as sc  # noqa: E402
import _surrogate_phase_scenario as psc  # noqa: E402
from _delta_phase_scenario import MOMENTS, ulps  # noqa: E402
from _rollout_scenario import host_matmul_is_fma_chain  # noqa: E402

pytestmark = pytest.mark.gpu

NS, WIDTHS, ACTS = (1, 3, 257, 4099), (64, 98, 256), (1, 4, 16)
GROUPS = (1, 2, 3, 0)
GUARD, FILL = 16, -7.5
SEED, CROSS_SEED = 2000, 2500       # bases under which no column of any case cancels below 1e-3 (``Case`` asserts it)


def _modules():
    import hipbind
    from pdecontrol.mbrl import replay_hip
    from pdecontrol.surrogates.evaluation import evaluate as ev
    replay_hip.load()
    return hipbind, replay_hip, ev


def _moments(n, i):
    """(mean, std) of a case's observations: the pairs with |mean| / std = 100 where three terms or fewer would cancel
    easily, else the first four of the delta tests' in rotation."""
    pairs = MOMENTS[1:3] if n <= 3 else MOMENTS[:4]
    return pairs[i % len(pairs)]


class Case:
    """Slabs on the device with NaN in every row that is not listed, the row list, and the twin's sums and statistics."""

    def __init__(self, n, N, A, forced, rows, offset, moments, seed):
        _, replay_hip, ev = _modules()
        self.dev = torch.device("cuda", 0)
        self.n, self.N, self.A, self.forced = n, N, A, forced
        obs, actions, F, live = sc.fit_case(n, N, A, rows, moments, seed)
        fields = [obs[live], actions[live]] + ([ev.forced_numpy(actions[live], F)] if forced else [])
        worst = min(sc.cancellation(f) for f in fields)
        assert worst >= 1e-3, ("a column of this case cancels too far for the bound on the sums", worst)
        self.sums, self.stats = ev.field_moments_numpy(obs, actions, F if forced else None, live)
        self.offsets, self.ld = replay_hip.fit_layout(N, A, forced)
        assert self.sums.shape == (2, self.ld)
        self.obs, self.actions = self._place(obs, offset), self._place(actions, offset)
        self.F = self._place(F, offset) if forced else None
        self.live = live
        self.rows = None if rows == "packed" else torch.from_numpy(live).to(self.dev)

    def _place(self, a, offset):
        flat = torch.empty(a.size + 4, dtype=torch.float32, device=self.dev)
        view = flat[offset:offset + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 16 == 4 * offset
        return view

    def run(self, groups, rows=None):
        """One call with fill patterns behind the workspace and both outputs; asserts they are still there."""
        hipbind, replay_hip, _ = _modules()
        rows = self.rows if rows is None else rows
        need = replay_hip.fit_workspace_doubles(self.N, self.A, self.forced, self.n, groups)
        assert need >= 2 * (self.N + self.A)
        ws = torch.full((need + GUARD,), FILL, dtype=torch.float64, device=self.dev)
        sums = torch.full((2 * self.ld + GUARD,), FILL, dtype=torch.float64, device=self.dev)
        stats = torch.full((2 * self.ld + GUARD,), FILL, dtype=torch.float32, device=self.dev)
        replay_hip.fit_moments(hipbind.stream(), self.obs, self.actions, self.F, rows, self.n, groups, ws, sums, stats)
        ws, sums, stats = ws.cpu().numpy(), sums.cpu().numpy(), stats.cpu().numpy()
        assert np.all(ws[need:] == FILL) and np.all(sums[2 * self.ld:] == FILL) and np.all(stats[2 * self.ld:] == FILL), "a guard changed"
        return sums[:2 * self.ld].reshape(2, self.ld), stats[:2 * self.ld].reshape(2, self.ld)

    def check(self, sums, stats, what):
        err = np.abs(sums - self.sums)
        assert np.all(err <= 1e-12 * np.abs(self.sums)), (what, "sums", float(np.max(err / np.abs(self.sums))))
        d = ulps(stats, self.stats.astype(np.float32))
        assert d.max() <= 1, (what, "stats", int(d.max()), stats.reshape(-1)[d.argmax()], self.stats.reshape(-1)[d.argmax()])
        return int(d.max())

    def columns(self):
        """Indices of the per-column entries (everything but the fields' totals)."""
        widths = (self.N, self.A, self.N)[:3 if self.forced else 2]
        return np.concatenate([np.arange(first, first + width) for first, width in zip(self.offsets, widths)])


def _rotation():
    """Every (n, N, A) once; forcing, row list, group count and alignment rotate with the index, each at its own period."""
    for i, (n, N, A) in enumerate(itertools.product(NS, WIDTHS, ACTS)):
        yield pytest.param(n, N, A, i % 3 != 2, ("packed", "permuted")[(i // 3 + i) % 2], GROUPS[(i // 2 + i) % 4], (i // 4) % 2,
                           _moments(n, i), SEED + i, id=f"n{n}-N{N}-A{A}")


@pytest.mark.parametrize("n,N,A,forced,rows,groups,offset,moments,seed", list(_rotation()))
def test_moments_against_the_twin(n, N, A, forced, rows, groups, offset, moments, seed):
    case = Case(n, N, A, forced, rows, offset, moments, seed)
    sums, stats = case.run(groups)
    worst = case.check(sums, stats, (forced, rows, groups, offset))
    again = case.run(groups)
    assert again[0].tobytes() == sums.tobytes() and again[1].tobytes() == stats.tobytes(), "two runs differ"
    assert np.isnan(stats[1, case.columns()]).all() == (n == 1)                 # one value per column has no variance
    assert np.isfinite(stats[0]).all() and np.isfinite(sums).all()              # the NaN rows around the listed ones were not read
    print(f"n={n} N={N} A={A} forced={forced} rows={rows} groups={groups} offset={offset}: stats within {worst} ulp")


def test_moments_in_full_cross():
    """With and without the forcing x row list x alignment x group count at (257, 256, 4), a width that takes float4 loads
    where the bases are aligned and a lane per column where they are not; the group counts of one combination agree with
    each other within the 1-ulp rule and each is repeatable."""
    worst = 0
    for i, (forced, rows, offset) in enumerate(itertools.product((True, False), ("packed", "permuted"), (0, 1))):
        case = Case(257, 256, 4, forced, rows, offset, _moments(257, i), CROSS_SEED + i)
        first = None
        for groups in GROUPS:
            sums, stats = case.run(groups)
            worst = max(worst, case.check(sums, stats, (forced, rows, offset, groups)))
            again = case.run(groups)
            assert again[0].tobytes() == sums.tobytes() and again[1].tobytes() == stats.tobytes(), "two runs differ"
            first = stats if first is None else first
            assert ulps(stats, first).max() <= 1, (forced, rows, offset, groups)
    print(f"n=257 N=256 A=4: 8 combinations x 4 group counts, stats within {worst} ulp of the twin")


def test_one_row_and_rows_outside_the_slab():
    """n = 1: the means are the row itself and only the fields' totals (N or A values) have a variance.  One row entry
    outside the slab, on either side, makes every sum and statistic NaN; numbers in the unlisted rows change nothing."""
    case = Case(1, 98, 4, True, "permuted", 0, (5.0, 0.05), 11)
    sums, stats = case.run(0)
    case.check(sums, stats, "one row")
    row = int(case.live[0])
    assert np.array_equal(stats[0, :98], case.obs[row].cpu().numpy()) and np.isnan(stats[1, case.columns()]).all()
    totals = np.setdiff1d(np.arange(case.ld), case.columns())
    assert totals.size == 3 and np.isfinite(stats[1, totals]).all()

    case = Case(257, 98, 16, True, "permuted", 0, (0.3, 2.0), 21)
    sums, stats = case.run(3)
    dead = torch.from_numpy(np.setdiff1d(np.arange(257 + 37), case.live)).to(case.dev)
    assert torch.isnan(case.obs[dead]).all() and torch.isnan(case.actions[dead]).all()
    case.obs[dead] = 1e6
    case.actions[dead] = -1e6
    other = case.run(3)
    assert other[0].tobytes() == sums.tobytes() and other[1].tobytes() == stats.tobytes()
    for bad in (257 + 37, -1, 2 ** 40):
        rows = case.rows.clone()
        rows[100] = bad
        sums, stats = case.run(3, rows=rows)
        assert np.isnan(sums).all() and np.isnan(stats).all(), bad


# ----------------------------------------------------------------------------------------------------------------------
# fit_scalings, kernel tier
# ----------------------------------------------------------------------------------------------------------------------
def _dataset(E=8, S=14, N=64, A=4, seed=3):
    """Seven ``[E, S, ...]`` numpy fields: smooth travelling fields around 0.7 that drift upwards by 0.02 a step, so
    that neither the observations nor their changes cancel over the columns; uniform actions."""
    episodes = psc.scripted_episodes(N, A, lengths=(S,) * E, seed=seed)
    drift = (0.7 + 0.02 * np.arange(S + 1, dtype=np.float32))[:, None, None]
    obs = np.stack([(field + drift)[:-1] for field, _ in episodes]).astype(np.float32)
    nxt = np.stack([(field + drift)[1:] for field, _ in episodes]).astype(np.float32)
    actions = np.stack([acts for _, acts in episodes])
    rewards = np.full((E, S), -1.0, np.float32)
    flags = np.zeros((E, S), bool)
    truncated = flags.copy()
    truncated[:, -1] = True
    return obs, actions, nxt, rewards, flags, truncated, np.tile(np.arange(S, dtype=np.int64), (E, 1))


def test_fit_scalings_kernel_tier_against_the_twin():
    from pdecontrol.mbrl.delta_phase import delta_rows_numpy, moments_numpy
    from pdecontrol.mbrl.recognition import field_map
    _, replay_hip, ev = _modules()
    env = sc.toy_env(device=0)
    data = _dataset()
    E, S, N, A = 8, 14, 64, 4
    train_idx, delta = np.asarray([5, 1, 6, 2, 7]), 0.25
    dev = torch.device("cuda", 0)
    device_data = [torch.from_numpy(f).to(dev) for f in data]
    fit = ev.fit_scalings(device_data, train_idx, env.forcing, delta)
    assert fit.tier == "kernel" and fit.tier_reason is None
    n = len(train_idx) * S
    rows = (train_idx[:, None] * S + np.arange(S)[None, :]).reshape(-1)
    flat = [f.reshape(E * S, f.shape[-1]) for f in data[:3]]
    F = env.forcing.forcing.numpy()
    _, stats = ev.field_moments_numpy(flat[0], flat[1], F, rows)
    offsets, _ = replay_hip.fit_layout(N, A, True)
    worst = {}
    for name, scaling, first, width in (("oscaling", fit.oscaling, offsets[0], N), ("ascaling", fit.ascaling, offsets[1], A),
                                        ("pdescaling", fit.pdescaling, offsets[2], N)):
        total = first + width
        worst[name] = (int(ulps(scaling.mean.cpu().numpy(), np.float32(stats[0, total])).max()),
                       int(ulps(scaling.var.cpu().numpy(), np.float32(stats[1, total])).max()))
    # the fourth fit takes the fitted observation scaling's own coefficients: the twin reads them from the same object
    fmap = field_map(fit.oscaling, N, normalize=True)
    _, dstats = moments_numpy(delta_rows_numpy(flat[0][rows], flat[2][rows], fmap, delta))
    worst["undscaling"] = (int(ulps(fit.undscaling.mean.cpu().numpy(), np.float32(dstats[0, N])).max()),
                           int(ulps(fit.undscaling.var.cpu().numpy(), np.float32(dstats[1, N])).max()))
    for scaling in fit[:4]:
        assert scaling.frozen and scaling.count == n
        for stat in (scaling.mean, scaling.var):
            assert stat.dtype == torch.float32 and stat.device == dev and tuple(stat.shape) == (1, 1, 1)
    host = ev.fit_scalings(data, train_idx, env.forcing, delta)
    assert host.tier == "host"
    distance = {name: (int(ulps(getattr(fit, name).mean.cpu().numpy(), getattr(host, name).mean.numpy()).max()),
                       int(ulps(getattr(fit, name).var.cpu().numpy(), getattr(host, name).var.numpy()).max()))
                for name in ("oscaling", "ascaling", "pdescaling", "undscaling")}
    print(f"kernel tier against the twin, ulp of (mean, var): {worst}; against the host tier (logged, not asserted): {distance}")
    assert all(max(pair) <= 2 for pair in worst.values()), worst
    # a forcing the kernels do not know goes to the host tier, on the device tensors, and says why
    from pdegym.common.transforms import FuncTransform
    other = ev.fit_scalings(device_data, train_idx, FuncTransform(lambda a: a.repeat(1, 1, 16)), delta)
    assert other.tier == "host" and "FuncTransform" in other.tier_reason and other.oscaling.mean.device == dev


# ----------------------------------------------------------------------------------------------------------------------
# the offline connector on the kernels of the surrogate-update phase
# ----------------------------------------------------------------------------------------------------------------------
CONFIG = {"factory": "KSAutoRegConvolutionalLSTM", "model": {}, "surrogate": {}, "loss": "MSELoss", "curriculum": {},
          "training": {"tau": 5, "tbtt": 10, "batch_size": 4, "patience": 5}, "trainer": {}}
SPLITS = ([0, 2, 3, 5, 6], [1, 7], [4])


def _fold(frozen=True, seed=5, untransformed=False):
    """(ev, env, fitted scalings, device fields, numpy fields) of an eight-episode dataset on the GPU."""
    _, _, ev = _modules()
    env = sc.toy_env(device=0)
    data = _dataset()
    fields = ev.device_fields(data, "cuda")
    fit = ev.fit_scalings(fields.obs.tensors, SPLITS[0], env.forcing, 0.25, untransformed=untransformed)
    assert fit.tier == "kernel"
    for scaling in fit[:4]:
        scaling.frozen = frozen
    return ev, env, fit, fields, data


def _module(ev, env, fit, seed=5):
    from pdecontrol import architectures
    torch.manual_seed(seed)
    return ev.build_module(env, architectures.KSAutoRegConvolutionalLSTM(), CONFIG, fit, "cuda")


@pytest.mark.parametrize("untransformed", (False, True))
def test_gather_through_the_offline_connector_is_the_host_loaders_batch(untransformed):
    """``sur_gather_windows`` with the coefficients of the frozen ``Normalize`` transforms against the batch the host
    ``PDEDataLoader`` builds with the transforms themselves: N = 64, B = 5, L = 6, bit for bit.  Actions behind the
    forcing are compared where torch's CPU matmul forms the product as the fma chain (else to 1e-6)."""
    from pdecontrol.mbrl.recognition import world_connector
    from pdecontrol.surrogates import hipops
    from pdecontrol.surrogates.common.dataset import PDEDataLoader, SubSeqDataset
    ev, env, fit, fields, data = _fold(untransformed=untransformed)
    N, A, B, L = 64, 4, 5, 6
    host_fit = ev.FittedScalings(*[_to_host(s) for s in fit[:4]], None, "host")
    atransf = host_fit.ascaling if untransformed else [fit.stransf.atransf.transforms[0].transforms[0], host_fit.pdescaling]
    from pdegym.common.transforms import SampleTransform
    host_stransf = SampleTransform(host_fit.oscaling, atransf)
    np.random.seed(1)
    dataset = SubSeqDataset(data=tuple(data), subsamples=[0, 3, 6], length=L, stride=4, bootstrapping=False, stransf=host_stransf)
    loader = PDEDataLoader(dataset, batch_size=B, shuffle=False, num_workers=0, collate_fn=PDEDataLoader.sample_collate)
    want = next(iter(loader))
    assert want[0].shape == (B, L, 1, N)

    store = fields.obs.window_store("cuda")
    obs_map, act_maps = world_connector(fit.stransf, N, A)
    gather = hipops.WindowGather(store.tensors[0], store.tensors[1], None, store.total, obs_map, act_maps)
    assert gather.refused() is None, gather.refused()
    keys, offsets = dataset.locate_many(np.arange(B))
    first = torch.from_numpy(np.asarray([store.starts[k] for k in keys], np.int64) + offsets).cuda()
    states = torch.full((B, L, 1, N), FILL, device="cuda")
    actions = torch.full((B, L, 1, act_maps[2].width), FILL, device="cuda")
    gather(first, 0, B, L, states, actions)
    assert states.cpu().numpy().tobytes() == want[0].numpy().tobytes()
    F = env.forcing.forcing.numpy()
    raw = np.stack([data[1][k][o:o + L] for k, o in zip(keys, offsets)])
    if untransformed or host_matmul_is_fma_chain(F, raw.reshape(B * L, 1, A)):
        assert actions.cpu().numpy().tobytes() == want[1].numpy().tobytes()
    else:
        np.testing.assert_allclose(actions.cpu().numpy(), want[1].numpy(), rtol=1e-6, atol=1e-6)


def _to_host(norm):
    from pdegym.common.transforms import Normalize
    out = Normalize(aggregate=norm.aggregate, batched=norm.batched, frozen=norm.frozen, epsilon=norm.epsilon)
    out.mean, out.var, out.count = norm.mean.cpu(), norm.var.cpu(), norm.count
    return out


def test_validation_loss_with_the_normalize_inverse(monkeypatch):
    """``sur_val_loss`` takes the inverse of the frozen ``Normalize``: ``decoded`` has the bits of ``Normalize._inv``, the
    three losses are within 1e-5 of ``validation_step``'s torch ops."""
    ev, env, fit, fields, data = _fold()
    module = _module(ev, env, fit)
    B, S, N = 3, 6, 64
    raw = torch.from_numpy(data[0][:B, :S]).cuda()
    states = fit.oscaling(raw)
    actions = fit.stransf.atransf(torch.from_numpy(data[1][:B, :S]).cuda())
    # time-major storage, as the phase's validation buffers are
    states = states.transpose(0, 1).contiguous().transpose(0, 1)
    actions = actions.transpose(0, 1).contiguous().transpose(0, 1)
    module.eval()
    with torch.no_grad():
        out = module._full_rollout(states, actions)
        fused = module._fused_validation_loss(out, states)
        assert fused is not None, "validation must take sur_val_loss with a frozen Normalize"
        loss, hstep, scalars, deltas, decoded = fused
        dec_in = torch.cat((states[:, :1], out.outputs[:, :-1]), dim=1)
        want = _to_host(fit.oscaling).Inverse(dec_in.cpu())
        assert decoded.cpu().numpy().tobytes() == want.numpy().tobytes()
        fused_step = module.validation_step((states, actions), 0)
        fused_logged = {k: float(v) for k, v in module.logged.items() if k.startswith("Val.")}
        monkeypatch.setattr(module, "_fused_validation_loss", lambda *a, **k: None)
        torch_step = module.validation_step((states, actions), 0)
        torch_logged = {k: float(v) for k, v in module.logged.items() if k.startswith("Val.")}
    print("fused", fused_logged, "torch", torch_logged)
    for name in ("Val. Loss", "Val. Scaled Loss", "Val. Delta Loss"):
        assert abs(fused_logged[name] - torch_logged[name]) <= 1e-5 * abs(torch_logged[name]), name
    assert abs(float(fused_step["loss"]) - float(torch_step["loss"])) <= 1e-5 * float(torch_step["loss"])
    np.testing.assert_allclose(fused_step["hsteploss"].cpu().numpy(), torch_step["hsteploss"].cpu().numpy(), rtol=1e-4)
    # unfrozen, the same module keeps the torch ops
    monkeypatch.undo()
    fit.oscaling.frozen = False
    with torch.no_grad():
        assert module._fused_validation_loss(out, states) is None


def test_update_surrogate_runs_the_offline_fold_on_the_kernel_tier(monkeypatch):
    """Eight episodes, batch 4, tau 5: ``fit.tier`` is "kernel", and after three steps the parameters and the Adam state
    have the bits of a hand-written loop (tests/_surrogate_phase_scenario.py) that feeds ``fused_step`` from numpy-twin
    batches.  With the scalings unfrozen the same datamodule is refused as before."""
    from pdecontrol.mbrl import surrogate_phase as sp
    from pdecontrol.mbrl.recognition import world_connector
    from pdecontrol.surrogates import ops
    monkeypatch.setenv("PDECONTROL_PIPELINED", "1")
    ev, env, fit, fields, data = _fold()
    train, val, test = SPLITS
    kernel_dm = ev.build_datamodule(fields, train, val, test, fit.stransf, CONFIG, 3, device_data="cuda")
    ref_dm = ev.build_datamodule(tuple(data), train, val, test, fit.stransf, CONFIG, 3)
    kernel, ref = _module(ev, env, fit), _module(ev, env, fit)
    monkeypatch.setattr(ref, "_fused_validation_loss", lambda *a, **k: None)
    maps = world_connector(fit.stransf, 64, 4)
    E, S = data[0].shape[:2]
    packed = (data[0].reshape(E * S, 64), data[1].reshape(E * S, 4), {e: e * S for e in range(E)})
    kernel_fit, ref_fit = sp.FitState(), sp.FitState()
    args = dict(max_steps=3, min_steps=0, patience=5)
    np.random.seed(17)
    torch.manual_seed(17)
    got = sp.update_surrogate(kernel, kernel_dm, kernel_fit, **args)
    assert (kernel_fit.tier, kernel_fit.tier_reason, kernel_fit.global_step) == ("kernel", None, 3)
    np.random.seed(17)
    torch.manual_seed(17)
    want = psc.reference_fit(ref, ref_dm, ref_fit, packed, maps, **args)
    torch.cuda.synchronize()
    assert (kernel_fit.current_epoch, kernel_fit.global_step) == (ref_fit.current_epoch, ref_fit.global_step)
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    (kp, ka), (rp, ra) = psc.optimizer_state(kernel), psc.optimizer_state(ref)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(kp, rp)), "parameters differ"
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ka, ra)), "Adam state differs"

    for scaling in fit[:4]:
        scaling.frozen = False
    ops._NOTIFIED.discard("a Normalize")
    loop_fit = sp.FitState()
    np.random.seed(17)
    sp.update_surrogate(_module(ev, env, fit), kernel_dm, loop_fit, max_steps=1, min_steps=0, patience=5)
    assert (loop_fit.tier, loop_fit.tier_reason) == ("loop", "a Normalize")


# ----------------------------------------------------------------------------------------------------------------------
# the dataset and one fold of the command line
# ----------------------------------------------------------------------------------------------------------------------
def test_generate_dataset_on_the_gpu_against_its_loop_tier():
    data = sc.toy_dataset(episodes=3, device="cuda")
    loop = sc.toy_dataset(episodes=3, device="cuda", tier="loop")
    assert (data.tier, loop.tier) == ("kernel", "loop")
    for a, b in zip(data.tensors, loop.tensors):
        assert a.is_cuda and a.dtype == b.dtype and torch.equal(a, b)
    obs, actions, nxt, rewards, terminated, truncated, steps = (t.cpu() for t in data.tensors)
    E, S = 3, 4
    assert [tuple(t.shape) for t in data.tensors] == [(E, S, 1, 64), (E, S, 1, 4), (E, S, 1, 64), (E, S), (E, S), (E, S), (E, S)]
    assert [t.dtype for t in data.tensors] == [torch.float32] * 4 + [torch.bool] * 2 + [torch.long]
    assert torch.equal(steps, torch.arange(S).repeat(E, 1)) and not terminated.any()
    assert truncated[:, -1].all() and not truncated[:, :-1].any()
    assert torch.equal(nxt[:, :-1], obs[:, 1:]) and torch.isfinite(nxt).all() and (rewards < 0).all()


def test_one_fold_of_main_on_the_gpu(tmp_path):
    from torch.utils.data import TensorDataset
    _, _, ev = _modules()
    data = sc.toy_dataset(device="cuda")
    path = tmp_path / "data.pl"
    torch.save(TensorDataset(*(t.cpu() for t in data.tensors)), path)
    out = tmp_path / "run"
    assert ev.main(sc.toy_argv(path, out, device="cuda"), make_env=lambda: sc.toy_env(device=0)) == 0
    for k in range(2):
        record = json.load(open(out / f"fold{k}.json"))
        assert record["tiers"] == {"fit": "kernel", "training": "kernel", "training_reason": None, "test": "kernel"}, record["tiers"]
        assert np.isfinite(record["Val. Loss"]) and np.isfinite(record["test_scalars"]["MSE"]) and record["test_samples"] == 3
        arrays = np.load(out / f"fold{k}.npz")
        assert arrays["states"].shape == (3, sc.TAU + sc.TARGET, 1, 64) and np.isfinite(arrays["hsteploss"]).all()
