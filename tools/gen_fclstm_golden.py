#!/usr/bin/env python3
"""Golden vectors of the autoregressive fully-connected LSTM ablation -> tests/golden/fclstm_golden.npz (run in the build
container).

Runs the reference's own ``KSAutoRegFullyConnectedLSTM`` (pdecontrol/architectures/autoreg.py:10-41),
``AutoRegPDESurrogate`` (pdecontrol/surrogates/surrogate.py:58-133) and ``PDETrainingModule.training_step``
(pdecontrol/surrogates/training.py:64-130) from the reference checkout, behind the stubs of oracle/gen_golden.py, on seeded
inputs, and records only numbers.  N = 64, B = 8, T = 20, tau = 5, tbtt = 10, MSELoss(reduction="none"), seed 0.  The
latent factory's fixture (``KSLatentLSTM``) is ``lstm_*`` of latent_golden.npz (tools/gen_latent_golden.py).

What is recorded (keys):
  (the batch)       states: surrogate_golden.npz's b8_states; actions [8, 20, 1, 4]: latent_golden.npz's lstm_actions (the
                    seeded draw is checked here against both, not stored again)
  id_*              training_step with identity dscaling / undscaling: loss, hsteploss, outputs, grad/<name> of every
                    parameter that received a gradient
  nz_*              the same with Normalize(mean 0.01, var 0.5) undscaling and its inverse as dscaling

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_fclstm_golden.py
"""
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference checkout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import gen_golden  # noqa: E402  (pins the CPU arithmetic before torch is imported)
import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "fclstm_golden.npz")
SHARED = os.path.join(ROOT, "tests", "golden", "surrogate_golden.npz")
LATENT = os.path.join(ROOT, "tests", "golden", "latent_golden.npz")


def fixtures():
    from pdecontrol.architectures.autoreg import KSAutoRegFullyConnectedLSTM
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.common.transforms import BatchTransform, Normalize

    def build(dscaling=None, undscaling=None):
        torch.manual_seed(0)
        factory = KSAutoRegFullyConnectedLSTM()
        surrogate = factory.surrogate(delta=0.25, dscaling=dscaling, tau=5, **factory.model())
        module = PDETrainingModule(surrogate=surrogate, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25,
                                   undscaling=undscaling, tau=5, tbtt=10)
        return surrogate, module

    g = torch.Generator().manual_seed(1)
    s8 = (torch.rand(64, 20, 1, 64, generator=g) * 2 - 1)[:8].clone()
    g = torch.Generator().manual_seed(2)
    a8 = torch.rand(8, 20, 1, 4, generator=g) * 2 - 1
    assert np.array_equal(s8.numpy(), np.load(SHARED)["b8_states"])
    assert np.array_equal(a8.numpy(), np.load(LATENT)["lstm_actions"])

    norm = Normalize(aggregate=True, batched=True)
    norm.mean, norm.var, norm.count = torch.full((1, 1, 1), 0.01), torch.full((1, 1, 1), 0.5), 100
    undscaling = BatchTransform(norm)
    out = {}
    for prefix, kw in (("id_", {}), ("nz_", dict(dscaling=undscaling.Inverse, undscaling=undscaling))):
        surrogate, module = build(**kw)
        res = module.training_step((s8, a8), 0)
        res["loss"].backward()
        out[prefix + "loss"] = np.float64(res["loss"].item())
        for k in ("hsteploss", "outputs"):
            out[prefix + k] = res[k].detach().numpy().copy()
        for k, p in surrogate.named_parameters():
            if p.grad is not None:
                out[prefix + "grad/" + k] = p.grad.numpy().copy()
    return out


def main():
    if not os.path.isdir(os.path.join(gen_golden.REF, "pdecontrol")):
        sys.exit(f"reference checkout not found at {gen_golden.REF}: the FC-LSTM fixture can only be generated where it is")
    gen_golden._install_stubs()
    fx = fixtures()
    assert all(np.asarray(v).dtype.kind in "fib" for v in fx.values())
    np.savez_compressed(OUT, **fx)
    size = os.path.getsize(OUT)
    assert size < 250 * 1024, size
    print(f"{os.path.relpath(OUT, ROOT)}: {len(fx)} arrays, {size} bytes")


if __name__ == "__main__":
    main()
