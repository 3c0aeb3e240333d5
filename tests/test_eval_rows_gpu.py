"""The surrogate test phase on the MI355X: the cases of tests/_eval_rows_cases.py on device 0 (the host suite runs them on
the CPU twin), the kernels against the twin, ``PDETrainingModule.test_step``'s kernel tier and ``test_surrogate`` against
the recorded fixture tests/golden/evalstep_golden.npz at the bar the existing GPU test of ``test_step`` uses
(rtol 2e-4, atol 2e-5: the fused rollout's fp32 against the reference's CPU rollout)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _eval_rows_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu
GPU, TWIN = 0, -1
RTOL, ATOL = 2e-4, 2e-5


def test_fixture_case_on_the_device():
    cases.check_fixture_case(GPU, "gfx950")


@pytest.mark.parametrize("columns", [False, True], ids=["scalar", "per-column"])
def test_normalize_inverse_has_the_host_transforms_bits(columns):
    cases.check_normalize_inverse(GPU, columns)


def test_scale_inverse_has_the_host_transforms_bits():
    cases.check_scale_inverse(GPU)


def test_shifted_time_major_prediction_equals_the_concatenated_layout():
    cases.check_shift_over_time_major(GPU)


def test_dissipation_rewards_have_the_reward_kernels_bits():
    cases.check_dissipation_rewards(GPU)


def test_fold_batch_of_one_accumulator_and_zero_norms():
    cases.check_fold(GPU)


def test_bad_arguments_are_refused_by_name():
    cases.check_bad_arguments(GPU)


@pytest.mark.parametrize("N,L,B,T", cases.SHAPES, ids=[f"n{s[0]}-b{s[2]}-t{s[3]}" for s in cases.SHAPES])
def test_rowstats_against_the_numpy_restatement_and_the_twin(N, L, B, T):
    """One N per lane-group width of the launcher (16 lanes up to N = 64, 32 up to 512, 64 above), an N that is no
    multiple of its width (100 = 3 * 32 + 4), and B * T that does not fill the last workgroup (21 and 17 rows of 16, 21 of 8)."""
    got = cases.check_shape(GPU, N, L, B, T)
    twin = cases.check_shape(TWIN, N, L, B, T)
    np.testing.assert_allclose(got, twin, rtol=1e-12, atol=0)


# ---- the module and the epoch ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_module():
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    from test_surrogate_host import build_eval_module
    return build_eval_module(KuramotoSivashinskyEnv(), torch.device("cuda", GPU))


def test_test_step_runs_its_kernel_tier_and_matches_the_fixture(gpu_module):
    module, g = gpu_module
    dev = torch.device("cuda", GPU)
    s, a = torch.from_numpy(g["states"]).to(dev), torch.from_numpy(g["actions"]).to(dev)
    with torch.no_grad():
        tst = module.test_step((s, a), 0)
    assert module.last_test_tier == "kernel"
    assert sorted("test_" + k for k in tst) == sorted(k for k in g.files if k.startswith("test_"))
    for k, v in tst.items():
        assert isinstance(v, np.ndarray) and v.dtype == np.float32, (k, type(v))
        np.testing.assert_allclose(v, g["test_" + k], rtol=RTOL, atol=ATOL, err_msg=k)
    from pdecontrol.surrogates import ops
    with ops.fused(False), torch.no_grad():
        module.test_step((s, a), 0)
    assert module.last_test_tier == "torch"


def test_test_surrogate_on_the_device(gpu_module):
    from pdecontrol.surrogates import test_phase
    module, g = gpu_module
    dev = torch.device("cuda", GPU)
    loader = cases.two_batch_loader(g, dev)
    want = {name: g["test_" + name] for name in cases.ROW_MEAN_KEYS}
    want.update(cases.reward_tables_of_two_batches(g))
    reports = {}
    for tier in (None, "torch"):
        report = reports[tier] = test_phase.test_surrogate(module, dataloaders=loader, nstore=2, tier=tier)
        assert (report.tier, report.batches, report.samples) == ("kernel" if tier is None else "torch", 2, 3)
        np.testing.assert_allclose(report.scalars["MSE"], g["test_MSE"], rtol=RTOL, atol=ATOL)
        for name, value in want.items():
            np.testing.assert_allclose(report.tables[name], value, rtol=RTOL, atol=ATOL, err_msg=f"{tier} {name}")
        for name in ("states", "outputs", "actions"):
            np.testing.assert_allclose(getattr(report, name), g["test_" + name][:2], rtol=RTOL, atol=ATOL, err_msg=name)
    for name, value in reports[None].tables.items():
        np.testing.assert_allclose(value, reports["torch"].tables[name], rtol=RTOL, atol=ATOL, err_msg=name)
    s, a = loader[0]
    with pytest.raises(ValueError, match="share T"):
        test_phase.test_surrogate(module, dataloaders=[(s, a), (s[:, :8], a[:, :8])])
