"""The SAC agent without a GPU: the reference's names, its CPU arithmetic bit for bit (tests/golden/sac_golden.npz is
recorded from the reference's class by tools/gen_sac_golden.py, through the same scenario function), the logger contract,
``update_many`` on the CPU and the host side of libsac_hip.so."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import _sac_models as sm
from conftest import GOLDEN, require_fma_sgemm


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "sac_golden.npz"))


def _agent(logs=None, **kw):
    from pdecontrol.sac.sac import SAC
    logger = None if logs is None else (lambda entry, commit=True: logs.append((dict(entry), commit)))
    hidden = kw.pop("hidden", 32)
    return SAC(*sm.spaces(), sm.config(hidden, **kw), logger=logger)


def test_reference_names_resolve_without_wandb(monkeypatch):
    monkeypatch.setitem(sys.modules, "wandb", None)          # absent, wherever the suite runs
    with pytest.raises(ImportError):
        import wandb  # noqa: F401
    from pdecontrol.sac import policies, sac, utils
    for name in ("GaussianPolicy", "QNetwork", "ValueNetwork", "weights_init_", "LOG_SIG_MAX", "LOG_SIG_MIN", "epsilon"):
        assert hasattr(policies, name), name
    for name in ("soft_update", "hard_update", "create_log_gaussian", "logsumexp"):
        assert hasattr(utils, name), name
    assert (policies.LOG_SIG_MAX, policies.LOG_SIG_MIN, policies.epsilon) == (2, -20, 1e-6)
    agent = _agent()
    assert agent.logger is None, "no wandb: the default logger is none"
    assert callable(agent.select_action) and callable(agent.update) and isinstance(agent, sac.SAC)
    wb = lambda *names: [f"{n}.{s}" for n in names for s in ("weight", "bias")]
    assert list(agent.critic.state_dict()) == wb(*[f"linear{i}" for i in range(1, 7)])
    assert list(agent.critic_target.state_dict()) == list(agent.critic.state_dict())
    assert list(agent.policy.state_dict()) == wb("linear1", "linear2", "mean_linear", "log_std_linear")
    assert list(policies.ValueNetwork(1, 64, 32).state_dict()) == wb("linear1", "linear2", "linear3")
    for opt in (agent.critic_optim, agent.policy_optim):
        assert type(opt) is torch.optim.Adam
    x = torch.linspace(-1, 1, 12).reshape(3, 4)
    assert torch.allclose(utils.logsumexp(x, dim=1), torch.logsumexp(x, dim=1))
    assert utils.create_log_gaussian(x, torch.zeros_like(x), x).shape == (3,)


def _host_reproduces_the_fixture_sgemm():
    """False where torch's CPU matmul cannot reproduce the fixtures' products (MKL's generic sgemm on CPUs of other vendors
    than Intel, oracle/cpu_math.py): conftest's own probe, independent of the code under test."""
    try:
        require_fma_sgemm("n64")
    except pytest.skip.Exception:
        return False
    return True


@pytest.mark.parametrize("tag", list(sm.CASES))
def test_cpu_arithmetic_is_the_references_bit_for_bit(tag, golden):
    """Every recorded array bit for bit.  On a host whose sgemm rounds differently from the one the fixture was recorded
    with, what no matrix product touches (the batch, the initial weights from the seed) is still compared bit for bit and
    the first forward and update within fp32 rounding, and the test then reports itself skipped, as the other fixture tests
    that depend on that sgemm do."""
    from pdecontrol.sac.sac import SAC
    logs = []
    got = sm.scenario(tag, lambda o, a, c: SAC(o, a, c, logger=lambda e, commit=True: logs.append((dict(e), commit))), logs)
    want = {k: golden[k] for k in golden.files if k.startswith(tag + "_") and (tag != "h32" or not k.startswith("h32_auto"))}
    assert want and set(got) == set(want)
    exact = _host_reproduces_the_fixture_sgemm()
    for key in sorted(want):
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, key
        if exact or "_batch_" in key or "_u0_" in key or key.endswith("_act_obs"):
            assert np.array_equal(got[key], want[key]), key
    if not exact:
        np.testing.assert_allclose(got[f"{tag}_action_before"], want[f"{tag}_action_before"], rtol=0, atol=1e-5)
        np.testing.assert_allclose(got[f"{tag}_u1_logged"], want[f"{tag}_u1_logged"], rtol=1e-4)
        pytest.skip("needs MKL's fma sgemm (an Intel CPU) for the bit-for-bit part: this CPU's MKL runs its generic sgemm; "
                    "inputs and initial weights matched bit for bit, the first forward and update within rounding")


def test_logger_gets_the_references_calls_and_terminated_raises():
    logs = []
    agent = _agent(logs, auto=True)
    batch = sm.make_batch(16, 5)
    agent.update(batch)
    assert [(list(e), c) for e, c in logs] == [(["Pol. Rew. Mean"], False), (list(sm.LOG_KEYS[1:]), True)]
    assert all(isinstance(v, float) for v in logs[1][0].values())
    quiet = _agent(None)
    quiet.update(batch)                       # nothing to observe but that it runs without a logger
    bad = list(batch)
    bad[4] = batch[4].clone()
    bad[4][3] = True
    with pytest.raises(AssertionError):
        agent.update(tuple(bad))
    # ``deterministic`` is accepted and ignored: both calls sample, from consecutive generator states
    obs = sm.smooth_fields(4, sm.OBS, 1)[:, 0]
    torch.manual_seed(3)
    a = agent.select_action(obs, deterministic=True)
    torch.manual_seed(3)
    b = agent.select_action(obs, deterministic=False)
    assert np.array_equal(a, b) and a.shape == (4, 1, sm.ACT)
    mean = agent.act(torch.from_numpy(obs), deterministic=True)
    assert not np.array_equal(mean.numpy(), a)


@pytest.mark.parametrize("stacked", [False, True])
def test_update_many_on_the_cpu_is_the_update_loop(stacked):
    batches = [sm.make_batch(16, 20 + i) for i in range(3)]
    agents = []
    for many in (False, True):
        torch.manual_seed(11)
        logs = []
        agent = _agent(logs, auto=True, interval=2)
        if not many:
            for b in batches:
                agent.update(b)
        elif stacked:
            agent.update_many(tuple(torch.stack([b[i] for b in batches]) for i in range(7)))
        else:
            agent.update_many(batches)
        agents.append((agent, [(tuple(e.items()), c) for e, c in logs]))
    (a, la), (b, lb) = agents
    assert [[(k, float(v)) for k, v in e] for e, _ in la] == [[(k, float(v)) for k, v in e] for e, _ in lb]
    for net in sm.NETS:
        for (k, p), q in zip(getattr(a, net).state_dict().items(), getattr(b, net).state_dict().values()):
            assert torch.equal(p, q), (net, k)
    assert torch.equal(a.log_alpha, b.log_alpha) and a.updates == b.updates == 3


# ---------------------------------------------------------------------------------------------------------------------
# the cross-compiled library on the host
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pdecontrol.sac import sac_hip
    return sac_hip.load()


def test_every_prototype_is_bound_and_exported(lib):
    """(that the bound names are the header's prototypes: tests/test_capi_symbols.py)"""
    from pdecontrol.sac import sac_hip
    for name, _, _ in sac_hip.SYMBOLS:
        assert hasattr(lib, name), name
    assert ctypes.sizeof(sac_hip.Config) == 5 * 4 + 3 * 4 + 12 * 4
    assert ctypes.sizeof(sac_hip.State) == 8 * (3 * 8 + 4 * 12 + 7)


def test_supported_geometries_and_refusals(lib):
    for obs_dim in (64, 128, 256):
        for act_dim in range(1, 17):
            assert lib.sac_supported(obs_dim, act_dim, 256) == 0
            assert lib.sac_workspace_floats(obs_dim, act_dim, 256, 257) > 0
    codes, messages = set(), set()
    for args in ((64, 4, 128), (65, 4, 256), (64, 17, 256)):
        rc = lib.sac_supported(*args)
        assert rc < 0
        codes.add(rc)
        messages.add(lib.sac_last_error().decode())
    assert len(codes) == 3 and len(messages) == 3 and all(messages)


def test_bad_arguments_are_refused_before_any_launch(lib):
    from pdecontrol.sac import sac_hip
    cfg = sac_hip.Config(64, 4, 256, 0, 1, 0.99, 0.005, 0.0)
    st = sac_hip.State()
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below is refused on the host
    assert lib.sac_policy_forward(None, None, None, 4, fake, None, fake, None, None) < 0
    assert lib.sac_policy_forward(None, ctypes.byref(cfg), ctypes.byref(st), -1, fake, None, fake, None, None) < 0
    assert lib.sac_policy_forward(None, ctypes.byref(cfg), ctypes.byref(st), 4, fake, None, fake, None, None) < 0   # NULL parameters
    assert "NULL" in lib.sac_last_error().decode()
    assert lib.sac_update(None, ctypes.byref(cfg), ctypes.byref(st), 0, *([fake] * 9)) < 0
    assert lib.sac_update(None, ctypes.byref(cfg), ctypes.byref(st), 4, *([None] * 9)) < 0
    assert lib.sac_grads(None, ctypes.byref(cfg), ctypes.byref(st), 4, *([fake] * 9), None, None, None) < 0
    bad = sac_hip.Config(64, 4, 128, 0, 1, 0.99, 0.005, 0.0)
    assert lib.sac_update(None, ctypes.byref(bad), ctypes.byref(st), 4, *([fake] * 9)) == lib.sac_supported(64, 4, 128)
    assert lib.sac_workspace_floats(64, 4, 256, 0) < 0
