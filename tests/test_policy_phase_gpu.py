"""The policy-update phase on an MI355X (pdecontrol/mbrl/policy_phase.py, csrc/replay.hip): ``rp_gather`` against the
host loader's collated batch, the kernel tier against the reference's loop feeding the same GPU agent, call counts,
determinism, the terminated check and the torch-on-device tier.  Every comparison with the host loader is bit for bit: the
gather copies, and its affine map is the host transform's four separately rounded fp32 operations.  Replays are the
scripted ragged pair of tests/_policy_phase_scenario.py."""
import logging

import numpy as np
import pytest
import torch

import _policy_phase_scenario as sc
import _sac_models as sm

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
LOSS_REL = 1e-3            # the bound of test_sac_gpu.py::test_updates_against_the_torch_spelling_on_the_gpu


class _Counting:
    """A stand-in for a loaded library that counts the calls of the named entries (the pattern of tests/test_sac_gpu.py)."""

    def __init__(self, lib, names):
        self.lib, self.calls = lib, {n: 0 for n in names}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in self.calls:
            return fn

        def counted(*a):
            self.calls[name] += 1
            return fn(*a)
        return counted


@pytest.fixture
def counting(monkeypatch):
    from pdecontrol.mbrl import policy_phase, replay_hip
    from pdecontrol.sac import sac_hip
    rp = _Counting(replay_hip.load(), ("rp_gather",))
    sac = _Counting(sac_hip.load(), ("sac_update", "sac_grads"))
    monkeypatch.setattr(replay_hip, "load", lambda: rp)
    monkeypatch.setattr(sac_hip, "load", lambda: sac)
    packs = []

    class CountingStore(policy_phase.DeviceSubSeqStore):
        def __init__(self, data, device, keys=None):
            packs.append(str(device))
            super().__init__(data, device, keys)

    monkeypatch.setattr(policy_phase, "DeviceSubSeqStore", CountingStore)
    return {"rp": rp.calls, "sac": sac.calls, "packs": packs}


# ---------------------------------------------------------------------------------------------------------------------
# the gather against the host loader
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act_dim", [1, 4, 16])
@pytest.mark.parametrize("stride", [1, 4])
@pytest.mark.parametrize("obs_dim", [64, 128, 256])
def test_gather_equals_the_host_loaders_batch(obs_dim, stride, act_dim):
    from pdecontrol.mbrl import policy_phase as pp, replay_hip
    from pdecontrol.sac import sac_hip
    datasets = sc.replay_pair(obs_dim, act_dim, stride, seed=obs_dim + stride + act_dim, per_column=act_dim == 4, scale=3)
    n0, n1 = (int(len(d)) for d in datasets)
    edges = [0, n0 - 1, n0, n0 + n1 - 1]                 # first and last row of each source
    rs = np.random.RandomState(obs_dim + act_dim)
    connectors = [pp._connector(d) for d in datasets]
    for B in (1, 37, 256, 257):
        picks = rs.randint(0, n0 + n1, size=B)
        picks[:min(B, 4)] = (edges if B > 1 else edges[3:])[:min(B, 4)]
        if B == 1:
            batches = [np.asarray([e]) for e in edges]   # every edge on its own at B = 1
        else:
            batches = [rs.permutation(picks)]
        for idx in batches:
            want = sc.collate_items(datasets, idx)
            plan = pp.PolicyBatchPlan(datasets, B, 1, indices=idx)
            tier = pp._KernelTier(plan, connectors, DEV)
            assert tier.refusal(B) is None and (tier.obs_dim, tier.act_dim) == (obs_dim, act_dim)
            nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)
            out = (nan(B + 1, obs_dim), nan(B + 1, act_dim), nan(B + 1, obs_dim), nan(B + 1), nan(B + 1))
            replay_hip.gather(sac_hip._stream(), tier.srcs, B, tier.rows.data_ptr(), *out)
            torch.cuda.synchronize(DEV)
            for name, got, ref in zip(sc.FIELDS, out, want):
                ref = ref.squeeze(1).reshape(B, -1).to(torch.float32)
                assert torch.equal(got[:B].reshape(B, -1).cpu(), ref), (name, B, obs_dim, stride, act_dim)
                assert bool(torch.isnan(got[B:]).all()), f"{name}: written past the batch"


def test_gather_poisons_rows_outside_the_replays():
    from pdecontrol.mbrl import policy_phase as pp, replay_hip
    from pdecontrol.sac import sac_hip
    datasets = sc.replay_pair(64, 4, seed=1)
    plan = pp.PolicyBatchPlan(datasets, 4, 1, indices=[0, 1, 2, 3])
    tier = pp._KernelTier(plan, [pp._connector(d) for d in datasets], DEV)
    rows = torch.tensor([0, -1, sum(plan.totals), sum(plan.totals) - 1], dtype=torch.int64, device=DEV)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=DEV)
    out = (z(4, 64), z(4, 4), z(4, 64), z(4), z(4))
    replay_hip.gather(sac_hip._stream(), tier.srcs, 4, rows.data_ptr(), *out)
    torch.cuda.synchronize(DEV)
    for t in out:
        bad = torch.isnan(t.reshape(4, -1)).all(dim=1).cpu().tolist()
        assert bad == [False, True, True, False] and not bool(torch.isnan(t[0]).any()) and not bool(torch.isnan(t[3]).any())


# ---------------------------------------------------------------------------------------------------------------------
# the phase against the loop
# ---------------------------------------------------------------------------------------------------------------------
def _state(agent, logs):
    torch.cuda.synchronize(DEV)
    state = sm.full_state(agent)
    state["counters"] = agent._fused.counters.cpu().clone()
    state["logged"] = torch.tensor([[float(v) for _, v in sorted(e.items())] for e, _ in logs if "SAC/Qloss" in e], dtype=torch.float64)
    state["rewards"] = torch.tensor([float(e["Pol. Rew. Mean"]) for e, _ in logs if "Pol. Rew. Mean" in e], dtype=torch.float64)
    return state


def _same(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def _phase(datasets, B, U, auto, interval, seed, how, logs=None):
    """A fresh agent on the GPU after U updates; ``how``: "phase" (update_policy) or "loop" (the reference's loop)."""
    from pdecontrol.mbrl import policy_phase as pp
    logs = [] if logs is None else logs
    agent = sm.build(256, auto=auto, interval=interval, obs_dim=64, act_dim=4, seed=seed, device=DEV, logs=logs, low=-2.0, high=1.0)
    torch.manual_seed(seed + 100)                        # torch's CPU and CUDA generators
    if how == "phase":
        assert pp.update_policy(agent, datasets, B, U) == U
    else:
        for batch in sc.reference_loader(datasets, B, U):
            agent.update(batch)
    return agent, _state(agent, logs), torch.get_rng_state(), torch.cuda.get_rng_state(DEV)


@pytest.mark.parametrize("interval", [1, 2])
@pytest.mark.parametrize("auto", [False, True], ids=["fixed-alpha", "auto-alpha"])
def test_kernel_tier_equals_the_reference_loop(auto, interval, counting):
    B, U = 64, 6
    datasets = sc.replay_pair(64, 4, stride=4, seed=2)
    _, loop, cpu_l, cuda_l = _phase(datasets, B, U, auto, interval, 3, "loop")
    before = dict(counting["rp"]), dict(counting["sac"]), len(counting["packs"])
    _, phase, cpu_p, cuda_p = _phase(datasets, B, U, auto, interval, 3, "phase")
    _same(loop, phase, "update_policy against the loop over the host loader")
    assert phase["logged"].shape == (U, 4) and int(phase["updates"]) == U and int(phase["counters"][3]) == U
    assert torch.equal(cpu_l, cpu_p) and torch.equal(cuda_l, cuda_p), "both generators end where the loop leaves them"
    # call counts: U gathers, sac_update only while the graph is captured, one pack per source
    assert counting["rp"]["rp_gather"] - before[0]["rp_gather"] == U
    assert counting["sac"]["sac_update"] - before[1]["sac_update"] == 1
    assert counting["packs"][before[2]:] == [str(DEV)] * 2


def test_two_phases_are_bit_identical():
    datasets = sc.replay_pair(64, 4, seed=5)
    runs = [_phase(datasets, 37, 5, True, 1, 8, "phase") for _ in range(2)]
    _same(runs[0][1], runs[1][1], "two runs of update_policy")
    assert torch.equal(runs[0][0]._fused.stats.cpu(), runs[1][0]._fused.stats.cpu())


def test_phase_without_a_logger_fetches_nothing_but_ends_the_same():
    from pdecontrol.mbrl import policy_phase as pp
    datasets = sc.replay_pair(64, 4, seed=6)
    _, logged, _, _ = _phase(datasets, 32, 4, False, 1, 2, "phase")
    agent = sm.build(256, obs_dim=64, act_dim=4, seed=2, device=DEV, low=-2.0, high=1.0)
    torch.manual_seed(102)
    assert pp.update_policy(agent, datasets, 32, 4) == 4
    quiet = _state(agent, [])
    for k in quiet:
        if k not in ("logged", "rewards"):
            assert torch.equal(quiet[k], logged[k]), k


@pytest.mark.parametrize("with_logger", [True, False], ids=["logger", "no-logger"])
def test_a_terminated_sample_raises_at_the_end_of_the_phase(with_logger):
    from pdecontrol.mbrl import policy_phase as pp
    datasets = sc.replay_pair(64, 4, seed=7, terminated_at=20)
    B, U = 64, 4
    torch.manual_seed(0)
    plan = pp.PolicyBatchPlan(datasets, B, U)
    flags = np.concatenate([np.asarray(v, dtype=bool) for v in datasets[0].fields[4].values()])
    assert flags.sum() == 1 and (plan.concat_rows == int(np.nonzero(flags)[0][0])).any(), "the plan must draw the terminated sample"
    agent = sm.build(256, obs_dim=64, act_dim=4, seed=1, device=DEV, logs=[] if with_logger else None, low=-2.0, high=1.0)
    torch.manual_seed(0)
    with pytest.raises(AssertionError, match="terminated samples are not expected"):
        pp.update_policy(agent, datasets, B, U)
    assert agent.updates == U, "the check is the one fetch at the end of the phase"


# ---------------------------------------------------------------------------------------------------------------------
# the torch-on-device tier
# ---------------------------------------------------------------------------------------------------------------------
def test_an_unrecognised_transform_runs_the_torch_on_device_tier_with_one_notice(counting, caplog):
    from pdecontrol.surrogates import ops
    from pdegym.common.transforms import BatchTransform, FuncTransform, SampleTransform
    datasets = sc.replay_pair(64, 4, seed=9)
    halve = SampleTransform(otransf=[BatchTransform(FuncTransform(lambda v: v * 0.5))], atransf=datasets[1].stransf.atransf)
    datasets[1].stransf = halve
    B, U = 64, 5
    ops._NOTIFIED.clear()
    caplog.clear()
    loop_logs, phase_logs = [], []
    loop_agent, loop, _, _ = _phase(datasets, B, U, True, 2, 4, "loop", loop_logs)
    with caplog.at_level(logging.WARNING, logger="pdecontrol.surrogates"):
        agent, phase, _, _ = _phase(datasets, B, U, True, 2, 4, "phase", phase_logs)
        _phase(datasets, B, U, True, 2, 4, "phase")
    notices = [r for r in caplog.records if "plain PyTorch-ROCm" in r.message]
    assert len(notices) == 1 and "FuncTransform" in notices[0].message, [r.message for r in caplog.records]
    assert counting["rp"]["rp_gather"] == 0 and counting["packs"] == [str(DEV)] * 4
    rel = lambda a, b: abs(float(a.detach()) - float(b.detach())) / abs(float(b.detach()))
    assert phase["logged"].shape == loop["logged"].shape == (U, 4)
    worst = max(rel(x, y) for x, y in zip(phase["logged"][:, :3].reshape(-1), loop["logged"][:, :3].reshape(-1)))
    print("torch-on-device tier against the host loop: worst relative loss difference", worst)
    assert worst <= LOSS_REL, worst
    assert rel(agent.log_alpha, loop_agent.log_alpha) <= LOSS_REL
    for k in loop:
        if k.startswith(("critic.", "policy.", "critic_target.")):
            scale = float(loop[k].abs().max())
            assert float((phase[k] - loop[k]).abs().max()) <= LOSS_REL * scale, k
