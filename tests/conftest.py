import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "model-based-pde-control_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

# the fixtures are bit-for-bit records: pin the CPU arithmetic they were recorded with (before anything imports torch)
from oracle import cpu_math  # noqa: E402

cpu_math.pin_env()
cpu_math.pin_torch()

GOLDEN = os.path.join(ROOT, "tests", "golden")

# (tag -> (L, N)) of the configurations the golden fixtures were generated for
KS_CONFIGS = {"n64": (22.0, 64), "n256": (88.0, 256), "n48": (16.5, 48), "n128": (44.0, 128)}


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def ks_golden():
    return np.load(os.path.join(GOLDEN, "ks_golden.npz"))


@pytest.fixture(scope="session")
def sur_golden():
    return np.load(os.path.join(GOLDEN, "surrogate_golden.npz"))


def require_fma_sgemm(tag):
    """Skips the calling test where torch's CPU matmul cannot reproduce the forcing products of the fixtures: they hold
    actions @ F as one fma chain (MKL on an Intel CPU); MKL on other vendors' CPUs runs a generic sgemm that rounds some
    of them differently (oracle/cpu_math.py).  Checked on configuration ``tag``'s actions against the oracle's fma chain,
    before the test does any work."""
    import torch
    from oracle import ks_oracle as ko
    g = np.load(os.path.join(GOLDEN, "ks_golden.npz"))
    a, F = g[f"{tag}_actions"], g[f"{tag}_F"]    # one [1, 4] action at a time, as the env's transform multiplies
    got = np.concatenate([(torch.from_numpy(x) @ torch.from_numpy(F)).numpy() for x in a])
    if not np.array_equal(got, ko.phi_from_actions(a, F)):
        pytest.skip("needs MKL's fma sgemm (an Intel CPU): this CPU's MKL runs its generic sgemm")


@pytest.fixture(autouse=True)
def _default_cuda_path():
    """Every test starts on the process default of the surrogate's CUDA path (fused HIP kernels)."""
    try:
        from pdecontrol.surrogates import ops
    except ImportError:
        yield
        return
    ops.reset_fused()
    yield
    ops.reset_fused()


# ---------------------------------------------------------------------------------------------------------------------
# gradient parity against the reference's recorded gradients (pdecontrol/surrogates/training.py:64-130 backward)
# ---------------------------------------------------------------------------------------------------------------------
#: per-tensor tolerance on max|g - g_ref| / max|g_ref| (the error relative to the TENSOR's scale: single near-zero entries
#: of a gradient carry fp32 summation-order noise of the whole contraction, so an element-wise rtol says nothing).
#: Observed on MI355X against the reference's recorded gradients (profiles/r03_grad_parity_observed.json, written by
#: tools/grad_parity_report.py from a GRAD_PARITY_COLLECT=1 run): <= 5.2e-5 on every path (fused, plain, pipelined; N = 64
#: and 256; B = 4 ... 64), the worst tensor always a decoder bias in front of a LayerNorm.  Tolerance = 4x that.
GRAD_TOL = 2e-4
GRAD_LOG = os.path.join(ROOT, "gpurun_out", "grad_parity_observed.jsonl")


def check_grads(label, grads, ref_of, tol=None):
    """grads: {parameter name: array}; ref_of(name) -> the reference's gradient.  Asserts every tensor within ``tol`` of
    the reference relative to that tensor's scale, and appends the observed maxima per parameter group to GRAD_LOG."""
    import json
    tol = GRAD_TOL if tol is None else tol
    if os.environ.get("GRAD_PARITY_COLLECT"):      # observation run (tools/grad_parity_report.py): record, do not judge
        tol = float("inf")
    groups, worst = {}, (0.0, None)
    for name, got in grads.items():
        ref = np.asarray(ref_of(name))
        got = np.asarray(got)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        scale = float(np.abs(ref).max())
        err = float(np.abs(got - ref).max()) / scale if scale > 0 else float(np.abs(got).max())
        grp = name.split(".")[0]
        groups[grp] = max(groups.get(grp, 0.0), err)
        if err > worst[0]:
            worst = (err, name)
    rec = {"label": label, "max_err_over_tensor_scale": groups, "worst": {"name": worst[1], "err": worst[0]}, "tol": tol}
    print("grad parity", json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(GRAD_LOG), exist_ok=True)
        with open(GRAD_LOG, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass
    assert worst[0] <= tol, f"{label}: {worst[1]} off by {worst[0]:.3e} of its scale (tolerance {tol:.1e})"
