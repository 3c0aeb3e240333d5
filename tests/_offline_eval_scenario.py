"""Shared pieces of the offline-evaluation tests (tests/test_offline_eval_host.py, tests/test_offline_eval_gpu.py): a toy
KS env with four-step episodes, the toy command line at the size of tests/_controller_scenario.py's run, fitted
``Normalize`` transforms with chosen statistics, the values the affine form of a frozen ``Normalize`` is checked on, and
the inputs of the ``rpn_moments`` matrix."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _collect_scenario as csc  # noqa: E402

ENV_ID = "KuramotoSivashinskyEnv-v0"
EPISODES, TAU, TARGET = 6, 2, 1           # four-step episodes: a window of tau + 1 = 3 steps fits twice


def toy_env(device=-1):
    """The single env the evaluation reads the scenario, the forcing and the test metrics from (never stepped)."""
    from pdegym.kuramoto import KuramotoSivashinskyEnv
    return KuramotoSivashinskyEnv(L=22.0, N=64, Tmax=1.0, device=device)


def toy_dataset(episodes=EPISODES, device=None, seed=5, tier=None):
    from pdecontrol.surrogates.evaluation.generate import generate_dataset
    ordinal = -1 if device in (None, "cpu") else torch.empty(0, device=device).device.index
    return generate_dataset(ENV_ID, episodes, device=device, seed=seed, tier=tier, make_envs=lambda n: csc.make_env(n, 64, ordinal))


def toy_argv(data, output, device="cpu", splits=2, untransformed=False, batch_size=4, max_epochs=1):
    argv = ["--project", "unused", "--offline", "--factory_module", "unused", "--env_id", ENV_ID, "--data", str(data),
            "--factory", "KSAutoRegConvolutionalLSTM", "--splits", str(splits), "--val", "0.34", "--target_length", str(TARGET),
            "--seed", "3", "--training", json.dumps(dict(tau=TAU, tbtt=10, batch_size=batch_size, patience=5)),
            "--trainer", json.dumps(dict(max_epochs=max_epochs, gradient_clip_val=0.5)), "--output", str(output), "--device", device]
    return argv + (["--untransformed"] if untransformed else [])


def fitted(mean, var, frozen=True, aggregate=True):
    """A ``Normalize(batched=True)`` with these statistics: scalars ([1, 1, 1]) or one value per column ([1, 1, W])."""
    from pdegym.common.transforms import Normalize
    norm = Normalize(aggregate=aggregate, batched=True)
    norm.mean = torch.as_tensor(np.asarray(mean, np.float32)).reshape(1, 1, -1)
    norm.var = torch.as_tensor(np.asarray(var, np.float32)).reshape(1, 1, -1)
    norm.count, norm.frozen = 10, frozen
    return norm


def probe_values(rs, mean, width, rows=2000):
    """[rows, 1, width] fp32: random values over many magnitudes, then +-0, +-inf, NaN, the mean itself, its two
    neighbours, subnormals and the largest finite values."""
    mean = np.broadcast_to(np.asarray(mean, np.float32).reshape(-1), (width,))
    body = (rs.standard_normal((rows, width)) * 10.0 ** rs.uniform(-6, 6, (rows, width))).astype(np.float32)
    tiny = np.float32(1e-45)
    special = [np.full(width, v, np.float32) for v in (0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, 1e-40, -1e-40,
                                                      np.finfo(np.float32).max, -np.finfo(np.float32).max)]
    special += [mean.copy(), np.nextafter(mean, np.float32(np.inf)), np.nextafter(mean, np.float32(-np.inf)), mean - tiny, mean + tiny]
    return np.concatenate([body, np.stack(special)])[:, None, :]


def same_bits(a, b):
    a, b = (np.ascontiguousarray(torch.as_tensor(v).detach().cpu().numpy()) for v in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- rpn_moments ------------------------------------------------------------------------------------------------------
def fit_case(n, N, A, rows, moments, seed, dead=37):
    """Host inputs of one ``rpn_moments`` case: slabs of n + ``dead`` rows with NaN in every row that is not listed, the
    listed rows ("packed": 0 ... n - 1, else a permutation's first n), and a forcing matrix.  Observations have the
    (mean, std) ``moments``; actions and the forcing matrix are positive, so no column of any field cancels."""
    rs = np.random.RandomState(seed)
    total = n + dead
    live = np.arange(n) if rows == "packed" else rs.permutation(total)[:n].astype(np.int64)
    obs = np.full((total, N), np.nan, np.float32)
    actions = np.full((total, A), np.nan, np.float32)
    obs[live] = (moments[0] + moments[1] * rs.standard_normal((n, N))).astype(np.float32)
    actions[live] = rs.uniform(0.2, 1.0, (n, A)).astype(np.float32)
    F = rs.uniform(0.1, 1.0, (A, N)).astype(np.float32)
    return obs, actions, F, live


def cancellation(values):
    """The smallest |sum v| / sum |v| over the columns and over all of them."""
    v = np.asarray(values, dtype=np.float64).reshape(-1, values.shape[-1])
    return float(np.append(np.abs(v.sum(0)) / np.abs(v).sum(0), abs(v.sum()) / np.abs(v).sum()).min())
