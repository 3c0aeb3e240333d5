"""The policy-update phase without a GPU (pdecontrol/mbrl/policy_phase.py): the index plan against the reference's real
``DataLoader`` / ``RandomSampler`` / ``ConcatDataset`` construction, the CPU tier against the reference's loop, the C ABI
of libreplay_hip.so, and the recognition of the controller's connectors.  Replays are the scripted ragged scenario of
tests/_policy_phase_scenario.py: an imagined and a real ``ExperienceReplay`` of different size, samples falling in both."""
import os
import re

import numpy as np
import pytest
import torch

import _policy_phase_scenario as sc
import _sac_models as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------------
# the plan equals the loader
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("U", [1, 3])
@pytest.mark.parametrize("B", [1, 32, 33, 256])
@pytest.mark.parametrize("seed", [0, 7, 123])
def test_plan_batches_equal_the_reference_loader(seed, B, U):
    from pdecontrol.mbrl import policy_phase as pp
    datasets = sc.replay_pair(seed=seed)
    torch.manual_seed(seed)
    want = list(sc.reference_loader(datasets, B, U))
    want_state = torch.get_rng_state()

    torch.manual_seed(seed)
    numpy_state = np.random.get_state()
    plan = pp.PolicyBatchPlan(datasets, B, U)
    got_state = torch.get_rng_state()
    after = np.random.get_state()
    assert numpy_state[0] == after[0] and np.array_equal(numpy_state[1], after[1]) and numpy_state[2:] == after[2:]
    got = list(pp.host_batches(plan))

    assert len(got) == len(want) == U
    for u, (g, w) in enumerate(zip(got, want)):
        sc.same_batch(g, w, f"seed {seed}, B {B}, update {u}")
    assert torch.equal(got_state, want_state), "the global torch generator must end where the loader leaves it"
    assert plan.source.shape == plan.rows.shape == plan.concat_rows.shape == (U, B)
    if B * U >= 32:
        assert set(np.unique(plan.source)) == {0, 1}, "the scenario is meant to draw from both replays"
    assert (plan.concat_rows >= 0).all() and (plan.concat_rows < sum(plan.totals)).all()


def test_plan_refuses_windows_and_empty_replays():
    from pdecontrol.mbrl import policy_phase as pp
    from pdecontrol.surrogates.common.dataset import SubSeqDataset
    datasets = sc.replay_pair()
    windows = SubSeqDataset(data=datasets[0].fields, length=2, stride=1, bootstrapping=False)
    with pytest.raises(ValueError):
        pp.PolicyBatchPlan([windows], 4, 1)
    with pytest.raises(ValueError):
        pp.PolicyBatchPlan([], 4, 1)


# ---------------------------------------------------------------------------------------------------------------------
# the CPU phase equals the loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("auto,interval", [(False, 1), (True, 2)], ids=["fixed-alpha", "auto-alpha"])
def test_cpu_phase_equals_the_reference_loop(auto, interval):
    from pdecontrol.mbrl import policy_phase as pp
    B, U = 33, 4
    datasets = sc.replay_pair(obs_dim=8, act_dim=4, seed=3)
    out = []
    for phase in (False, True):
        logs = []
        agent = sm.build(32, auto=auto, interval=interval, obs_dim=8, act_dim=4, seed=5, logs=logs, low=-2.0, high=1.0)
        torch.manual_seed(11)
        if phase:
            assert pp.update_policy(agent, datasets, B, U) == U
        else:
            for batch in sc.reference_loader(datasets, B, U):
                agent.update(batch)
        state = sm.full_state(agent)
        state["rng"] = torch.get_rng_state()
        out.append((state, logs))
    (loop, loop_logs), (phase, phase_logs) = out
    assert set(loop) == set(phase)
    for k in loop:
        assert torch.equal(loop[k], phase[k]), k
    assert int(phase["updates"]) == U and int(phase["critic_optim.0.step"]) == U
    assert len(loop_logs) == len(phase_logs) == 2 * U
    for (a, ca), (b, cb) in zip(loop_logs, phase_logs):
        assert ca == cb and set(a) == set(b)
        for k in a:
            assert float(a[k]) == float(b[k]), k


def test_cpu_phase_with_zero_updates_does_nothing():
    from pdecontrol.mbrl import policy_phase as pp
    agent = sm.build(32, obs_dim=8, act_dim=4, seed=5)
    before = sm.full_state(agent)
    assert pp.update_policy(agent, sc.replay_pair(), 16, 0) == 0
    after = sm.full_state(agent)
    assert agent.updates == 0 and all(torch.equal(before[k], after[k]) for k in before)


# ---------------------------------------------------------------------------------------------------------------------
# header and binding
# ---------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    """(that the header declares exactly the bound names and the library exports them: tests/test_capi_symbols.py)"""
    from pdecontrol.mbrl import replay_hip
    assert sorted(n for n, _, _ in replay_hip.SYMBOLS) == ["rp_append", "rp_episode_returns", "rp_gather", "rp_last_error",
                                                           "rp_supported"]
    header = open(os.path.join(ROOT, "include", "replay_hip.h")).read()
    for macro, value in (("RP_MAX_SOURCES", replay_hip.MAX_SOURCES), ("RP_MAX_OBS_DIM", replay_hip.MAX_OBS_DIM),
                         ("RP_MAX_ACT_DIM", replay_hip.MAX_ACT_DIM)):
        assert re.search(rf"#define {macro} {value}\b", header), macro
    fields = re.search(r"typedef struct rp_source \{(.*?)\} rp_source;", re.sub(r"/\*.*?\*/", "", header, flags=re.S), re.S).group(1)
    declared = [n for decl in fields.split(";") for n in re.findall(r"\*?\s*([a-z_]+)\s*(?:,|$)", decl.strip())]
    assert declared == [n for n, _ in replay_hip.Source._fields_]


def test_rp_supported_refuses_with_distinct_codes_and_messages():
    from pdecontrol.mbrl import replay_hip
    lib = replay_hip.load()

    def source(**over):
        s = replay_hip.Source(16, 16, 16, 16, 16, 10, 64, 4, 0, 1, None, None)   # pointers are never dereferenced here
        for k, v in over.items():
            setattr(s, k, v)
        return s

    assert lib.rp_supported(1, replay_hip.sources([source()]), 256) == 0
    assert lib.rp_supported(2, replay_hip.sources([source(), source(obs_width=256, sensor_start=2, sensor_stride=4)]), 1) == 0
    codes = {}
    for what, nsrc, srcs, needle in (
            ("zero stride", 1, replay_hip.sources([source(sensor_stride=0)]), "stride"),
            ("wide actions", 1, replay_hip.sources([source(act_width=17)]), "action width 17"),
            ("NULL source", 1, None, "NULL source"),
            ("NULL field", 1, replay_hip.sources([source(nxtobs=None)]), "NULL field"),
            ("no batch", 1, replay_hip.sources([source()]), None),
            ("sensor start", 1, replay_hip.sources([source(sensor_start=64)]), "column 64"),
            ("mismatch", 2, replay_hip.sources([source(), source(obs_width=128)]), "source 0"),
            ("too many", 9, replay_hip.sources([source()] * 9), "9 sources")):
        rc = lib.rp_supported(nsrc, srcs, 0 if what == "no batch" else 32)
        assert rc < 0, what
        message = replay_hip.last_error()
        assert message.startswith("rp_gather") and (needle is None or needle in message), (what, message)
        codes[what] = rc
    assert len({codes["zero stride"], codes["wide actions"], codes["NULL source"]}) == 3, codes
    assert codes["NULL source"] == codes["NULL field"]
    assert replay_hip.supported(replay_hip.sources([source(act_width=0)]), 8) is not None
    # the launch entry validates before it touches the device
    assert lib.rp_gather(None, 1, replay_hip.sources([source(sensor_stride=0)]), 4, 16, 16, 16, 16, 16, 16) == codes["zero stride"]
    assert lib.rp_gather(None, 1, replay_hip.sources([source()]), 4, None, 16, 16, 16, 16, 16) < 0


def test_missing_library_raises(monkeypatch):
    from pdecontrol.mbrl import replay_hip
    monkeypatch.setattr(replay_hip, "LIB_PATH", "/nonexistent/libreplay_hip.so")
    monkeypatch.setattr(replay_hip, "_lib", None)
    with pytest.raises(replay_hip.ReplayHipError):
        replay_hip.load()


# ---------------------------------------------------------------------------------------------------------------------
# transform recognition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_column", [False, True], ids=["scalar-bounds", "per-column-bounds"])
@pytest.mark.parametrize("stride", [1, 4])
def test_controller_connectors_are_recognised_bit_for_bit(stride, per_column):
    from pdecontrol.mbrl import policy_phase as pp
    width, act_dim = 32 * stride, 4
    world_to_agent, to_agent = sc.controller_connectors(act_dim, stride, per_column, width, seed=stride)
    rs = np.random.RandomState(stride)
    obs = (rs.randn(50, 1, 1, width) * 2).astype(np.float32)
    actions = rs.uniform(-2, 1, (50, 1, 1, act_dim)).astype(np.float32)
    for name, stransf, sensor in (("replay_to_agent", to_agent, (stride // 2, stride)), ("world_replay_to_agent", world_to_agent, (0, 1))):
        con = pp.recognize(stransf, width, act_dim)
        assert (con.obs.start, con.obs.stride) == sensor and con.obs.width == len(range(sensor[0], width, sensor[1])), name
        assert (con.actions.start, con.actions.stride, con.actions.width) == (0, 1, act_dim)
        assert con.actions.coef is not None and con.actions.coef.shape == (4, act_dim) and con.actions.coef.dtype == torch.float32
        assert (con.obs.coef is None) == (name == "world_replay_to_agent")
        for i in range(obs.shape[0]):                    # item by item, as the dataset applies its connector
            want_o, want_a = stransf.otransf(obs[i]), stransf.atransf(actions[i])
            got_o, got_a = con.obs.apply_numpy(obs[i]), con.actions.apply_numpy(actions[i])
            assert got_o.dtype == want_o.dtype == np.float32 and got_o.shape == want_o.shape
            assert np.array_equal(got_o, want_o), (name, "obs", i)
            assert np.array_equal(got_a, want_a), (name, "actions", i)
    assert pp.recognize(None, width, act_dim).obs.coef is None


def test_sensor_before_scaling_and_inverse_connectors_are_recognised():
    from pdecontrol.mbrl import policy_phase as pp
    from pdegym.common.transforms import BatchTransform, ScaleTransform, SensorTransform, SampleTransform
    rs = np.random.RandomState(4)
    bounds = lambda n: ((-2 - rs.uniform(0, 1, (1, 1, n))).astype(np.float32), (2 + rs.uniform(0, 1, (1, 1, n))).astype(np.float32))
    oscale = ScaleTransform(bounds=bounds(32), batched=True, frozen=True)      # per column of the 32 the first sensor leaves
    scale = ScaleTransform(bounds=bounds(16), batched=True, frozen=True)
    stransf = SampleTransform(otransf=[BatchTransform(SensorTransform(2)), oscale, SensorTransform(2)], atransf=scale.Inverse)
    con = pp.recognize(stransf, 64, 16)
    assert (con.obs.start, con.obs.stride, con.obs.width) == (1 + 2, 4, 16)    # 64 columns -> 32 from column 1 -> 16 from column 1 of those
    obs, act = rs.randn(1, 1, 64).astype(np.float32), rs.uniform(-1, 1, (1, 1, 16)).astype(np.float32)
    assert np.array_equal(con.obs.apply_numpy(obs), stransf.otransf(obs))
    assert np.array_equal(con.actions.apply_numpy(act), stransf.atransf(act))
    back = SampleTransform(atransf=scale).Inverse                      # Operation([_OperationInverse]) around the inverse
    assert np.array_equal(pp.recognize(back, 64, 16).actions.apply_numpy(act), back.atransf(act))


def test_other_transforms_are_reported_unrecognised():
    from pdecontrol.mbrl import policy_phase as pp
    from pdecontrol.mbrl.recognition import Unrecognized
    from pdegym.common.transforms import (BatchTransform, FuncTransform, GaussianForcing, Normalize, ScaleTransform,
                                          SensorTransform, SampleTransform)
    scale = ScaleTransform(bounds=(-1.0, 1.0), frozen=True)
    forcing = GaussianForcing(np.linspace(0, 22, 64, endpoint=False), [0.2, 0.4, 0.6, 0.8], 0.4, 22.0, 64)
    for what, stransf in (
            ("Normalize", SampleTransform(otransf=[scale, Normalize(aggregate=True, batched=True)])),
            ("FuncTransform", SampleTransform(atransf=[BatchTransform(FuncTransform(lambda v: v * 2))])),
            ("GaussianForcing", SampleTransform(atransf=[BatchTransform(forcing), scale])),
            ("two scalings", SampleTransform(otransf=[scale, SensorTransform(1), BatchTransform(scale)])),
            ("inverse of a SensorTransform", SampleTransform(otransf=SensorTransform(2)).Inverse),
            ("float", lambda sample: sample)):
        with pytest.raises(Unrecognized) as e:
            pp.recognize(stransf, 64, 4)
        assert str(e.value), what
        if what in ("Normalize", "FuncTransform", "GaussianForcing", "two scalings"):
            assert what in str(e.value), (what, str(e.value))
