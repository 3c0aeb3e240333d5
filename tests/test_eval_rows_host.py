"""The surrogate test phase on the host: ``ks_eval_rows_device`` / ``ks_eval_fold_device`` on the library's CPU twin
(``device = -1``), the recognition of inverse observation chains, and ``test_surrogate`` on a CPU module.  The cases are
tests/_eval_rows_cases.py's, which tests/test_eval_rows_gpu.py runs on device 0; the yardsticks are the recorded fixture
tests/golden/evalstep_golden.npz, the numpy restatement tests/_eval_metrics_oracle.py and torch's host transforms."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_rows_cases as cases  # noqa: E402
from conftest import require_fma_sgemm  # noqa: E402

TWIN = -1


def test_fixture_case_on_the_twin():
    cases.check_fixture_case(TWIN, "twin")


@pytest.mark.parametrize("columns", [False, True], ids=["scalar", "per-column"])
def test_normalize_inverse_has_the_host_transforms_bits(columns):
    cases.check_normalize_inverse(TWIN, columns)


def test_scale_inverse_has_the_host_transforms_bits():
    cases.check_scale_inverse(TWIN)


def test_shifted_time_major_prediction_equals_the_concatenated_layout():
    cases.check_shift_over_time_major(TWIN)


def test_dissipation_rewards_have_the_reward_kernels_bits():
    cases.check_dissipation_rewards(TWIN)


def test_fold_batch_of_one_accumulator_and_zero_norms():
    cases.check_fold(TWIN)


@pytest.mark.parametrize("N,L,B,T", cases.SHAPES, ids=[f"n{s[0]}-b{s[2]}-t{s[3]}" for s in cases.SHAPES])
def test_rowstats_against_the_numpy_restatement(N, L, B, T):
    cases.check_shape(TWIN, N, L, B, T)


def test_bad_arguments_are_refused_by_name():
    cases.check_bad_arguments(TWIN)


def test_inverse_map_recognises_what_it_says_and_refuses_the_rest():
    from pdecontrol.mbrl.recognition import Unrecognized, field_map, inverse_map
    from pdegym.common import transforms as T
    norm = T.Normalize(aggregate=True, batched=True)
    norm.update(torch.linspace(-1.0, 2.0, 3 * 8).reshape(3, 1, 8))
    chain = T.SampleTransform(norm, None).otransf.Inverse
    kind, coef = inverse_map(chain, 8)
    assert kind == 2 and coef.dtype == torch.float32
    assert torch.equal(coef[0], torch.sqrt(norm.var + norm.epsilon).reshape(1).expand(8))
    assert torch.equal(coef[1], norm.mean.reshape(1).expand(8))
    with pytest.raises(Unrecognized):
        field_map(chain, 8)                                       # field_map keeps refusing a Normalize
    assert inverse_map(T.SampleTransform(None, None).otransf.Inverse, 8) == (0, None)
    assert inverse_map(T.Operation([T.SensorTransform(1)]).Inverse, 8) == (0, None)
    scale = T.ScaleTransform(scale=(-1.0, 1.0), bounds=(-3.0, 5.0))
    kind, coef = inverse_map(T.Operation([T.BatchTransform(scale)]).Inverse, 8)
    assert kind == 1 and torch.equal(coef, field_map(T.Operation([T.BatchTransform(scale)]).Inverse, 8).coef)
    for bad in (T.Operation([norm]),                              # the forward Normalize divides: not the mul-add
                T.Operation([norm, scale]).Inverse,               # two scalings
                T.Operation([T.SensorTransform(2)]),
                T.Operation([T.Normalize()]).Inverse,             # not fitted
                T.Operation([T.FuncTransform(lambda v: v)])):
        with pytest.raises(Unrecognized):
            inverse_map(bad, 8)


# ---- test_surrogate on a CPU module ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_module():
    require_fma_sgemm("n64")   # the action scaling is fitted on forcing products of the default env (n64)
    from _oracle_stepper import OracleStepper
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    from test_surrogate_host import build_eval_module
    return build_eval_module(KuramotoSivashinskyEnv(_stepper_cls=OracleStepper))


def test_test_surrogate_single_batch_equals_the_fixture(cpu_module):
    from pdecontrol.surrogates import test_phase
    module, g = cpu_module
    s, a = torch.from_numpy(g["states"]), torch.from_numpy(g["actions"])
    module.train()
    report = test_phase.test_surrogate(module, dataloaders=[(s, a)])
    assert module.training                                       # the mode it was in is restored
    module.eval()
    assert test_phase.test_surrogate(module, dataloaders=[(s, a)], nstore=1).states.shape[0] == 1
    assert not module.training
    assert (report.tier, report.batches, report.samples, module.last_test_tier) == ("torch", 1, 3, "torch")
    names = sorted(list(report.scalars) + list(report.tables) + ["states", "outputs", "actions"])
    assert names == sorted(k[len("test_"):] for k in g.files if k.startswith("test_"))
    for name, value in {**report.scalars, **report.tables}.items():
        np.testing.assert_allclose(value, g["test_" + name], rtol=1e-6, atol=1e-7, err_msg=name)
    for name in ("states", "outputs", "actions"):
        np.testing.assert_allclose(getattr(report, name), g["test_" + name], rtol=1e-6, atol=1e-7, err_msg=name)


def test_test_surrogate_two_batches_is_the_callbacks_weighted_mean(cpu_module):
    from pdecontrol.surrogates import test_phase
    module, g = cpu_module
    report = test_phase.test_surrogate(module, dataloaders=cases.two_batch_loader(g), nstore=2)
    assert (report.tier, report.batches, report.samples) == ("torch", 2, 3)
    # weighted means of row means are the whole batch's row means
    np.testing.assert_allclose(report.scalars["MSE"], g["test_MSE"], rtol=1e-6, atol=1e-7)
    for name in cases.ROW_MEAN_KEYS:
        np.testing.assert_allclose(report.tables[name], g["test_" + name], rtol=1e-6, atol=1e-7, err_msg=name)
    # the reward tables are norms over a batch: the weighted mean of the per-batch norms
    for name, want in cases.reward_tables_of_two_batches(g).items():
        np.testing.assert_allclose(report.tables[name], want, rtol=1e-6, atol=1e-7, err_msg=name)
    for name in ("states", "outputs", "actions"):
        np.testing.assert_allclose(getattr(report, name), g["test_" + name][:2], rtol=1e-6, atol=1e-7, err_msg=name)
    report = test_phase.test_surrogate(module, dataloaders=cases.two_batch_loader(g), nstore=20)
    assert report.states.shape[0] == report.outputs.shape[0] == report.actions.shape[0] == 3


def test_test_surrogate_refuses_batches_of_different_length(cpu_module):
    from pdecontrol.surrogates import test_phase
    module, g = cpu_module
    s, a = torch.from_numpy(g["states"]), torch.from_numpy(g["actions"])
    with pytest.raises(ValueError, match="share T"):
        test_phase.test_surrogate(module, dataloaders=[(s, a), (s[:, :8], a[:, :8])])
    with pytest.raises(ValueError):
        test_phase.test_surrogate(module, dataloaders=[(s, a)], tier="fastest")
