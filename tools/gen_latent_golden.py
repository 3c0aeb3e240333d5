#!/usr/bin/env python3
"""Golden vectors of the latent-space surrogate ablations -> tests/golden/latent_golden.npz (run in the build container).

Runs the reference's own ``KSLatentConvolutionalLSTM`` / ``KSLatentLSTM`` (pdecontrol/architectures/latent.py),
``LatentAutoRegPDESurrogate`` (pdecontrol/surrogates/surrogate.py:136-206) and ``PDETrainingModule.training_step``
(pdecontrol/surrogates/training.py:64-130) from the reference checkout, behind the stubs of oracle/gen_golden.py, on seeded
inputs, and records only numbers.  N = 64, B = 8, T = 20, tau = 5, tbtt = 10, MSELoss(reduction="none").

What is recorded (keys):
  sd/<name>                     the seeded (torch.manual_seed(0)) state_dict of KSLatentConvolutionalLSTM
  (the batch)                   [8, 20, 1, 64] states and actions: the first 8 rows of oracle/gen_golden.py's seeded B = 64
                                batch, stored in surrogate_golden.npz as b8_states / b8_actions (checked here, not
                                stored twice: a committed fixture stays under 300 KB)
  id_*                          training_step with identity dscaling / undscaling: loss, hsteploss, outputs, outdeltas,
                                grad/<name>.  Its true deltas are surrogate_golden.npz's b8_deltas (checked here).
  nz_*                          the same with Normalize(scalar stats) undscaling and its inverse as dscaling.  In decoded
                                mode the loss reads the outputs only, so the outputs, the loss and every gradient are
                                bit-identical to id_* (checked here).  Stored: nz_loss, and every NZ_PICK-th element of
                                the flattened nz_outdeltas (nz_outdeltas_pick; the whole tensor is the Normalize of
                                id_outdeltas); the true deltas are surrogate_golden.npz's b8n_deltas (checked here).
  ro1_*, ro2_*                  rollout API: warm-up on 5 given states over 10 steps, then the hidden state carried into a
                                second call from the last prediction; outputs, deltas, inlatents, outlatents, H, C of the
                                first RO_B samples (the inlatent / outlatent tensors are 16 x 16 per step)
  lstm_*                        KSLatentLSTM (seed 0): its actions [8, 20, 1, 4], training_step loss and hsteploss; the
                                gradient of every parameter up to LSTM_FULL elements in full (grad/<name>), of the two
                                LSTM weight matrices (1 024 x 4 and 1 024 x 256: 1 MB) the fp64 sum, sum of squares and every
                                97th element (gradsum/, gradsq/, gradpick/)

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_latent_golden.py
"""
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference checkout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import gen_golden  # noqa: E402  (pins the CPU arithmetic before torch is imported)
import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "latent_golden.npz")
SHARED = os.path.join(ROOT, "tests", "golden", "surrogate_golden.npz")
RO_B = 1
LSTM_FULL = 4096
PICK = 97
NZ_PICK = 5


def _step(module, surrogate, batch, prefix, out, keys=("loss", "hsteploss", "outputs", "outdeltas", "deltas")):
    res = module.training_step(batch, 0)
    res["loss"].backward()
    if "loss" in keys:
        out[prefix + "loss"] = np.float64(res["loss"].item())
    for k in keys:
        if k != "loss":
            out[prefix + k] = res[k].numpy().copy()
    return res, {k: p.grad.numpy().copy() for k, p in surrogate.named_parameters() if p.grad is not None}


def fixtures():
    from pdecontrol.architectures.latent import KSLatentConvolutionalLSTM, KSLatentLSTM
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.common.transforms import BatchTransform, Normalize

    def build(factory_cls, dscaling=None, undscaling=None):
        torch.manual_seed(0)
        factory = factory_cls()
        model = factory.model()
        surrogate = factory.surrogate(delta=0.25, dscaling=dscaling, tau=5, **model)
        module = PDETrainingModule(surrogate=surrogate, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25,
                                   undscaling=undscaling, tau=5, tbtt=10)
        return surrogate, module

    out = {}
    surrogate, module = build(KSLatentConvolutionalLSTM)
    for k, v in surrogate.state_dict().items():
        out["sd/" + k] = v.numpy().copy()

    g = torch.Generator().manual_seed(1)
    states64 = torch.rand(64, 20, 1, 64, generator=g) * 2 - 1
    actions64 = torch.rand(64, 20, 1, 64, generator=g) * 2 - 1
    s8, a8 = states64[:8].clone(), actions64[:8].clone()
    shared = np.load(SHARED)
    assert np.array_equal(s8.numpy(), shared["b8_states"]) and np.array_equal(a8.numpy(), shared["b8_actions"])

    res_id, grads_id = _step(module, surrogate, (s8, a8), "id_", out, keys=("loss", "hsteploss", "outputs", "outdeltas"))
    assert np.array_equal(res_id["deltas"].numpy(), shared["b8_deltas"])
    for k, v in grads_id.items():
        out["id_grad/" + k] = v

    norm = Normalize(aggregate=True, batched=True)
    norm.mean, norm.var, norm.count = torch.full((1, 1, 1), 0.01), torch.full((1, 1, 1), 0.5), 100
    undscaling = BatchTransform(norm)
    surrogate, module = build(KSLatentConvolutionalLSTM, dscaling=undscaling.Inverse, undscaling=undscaling)
    res_nz, grads_nz = _step(module, surrogate, (s8, a8), "nz_", out, keys=("loss",))
    out["nz_outdeltas_pick"] = res_nz["outdeltas"].numpy().reshape(-1)[::NZ_PICK].copy()
    assert np.array_equal(res_nz["deltas"].numpy(), shared["b8n_deltas"])
    assert res_nz["loss"].item() == res_id["loss"].item()
    assert torch.equal(res_nz["outputs"], res_id["outputs"]) and torch.equal(res_nz["hsteploss"], res_id["hsteploss"])
    assert grads_nz.keys() == grads_id.keys() and all(np.array_equal(grads_nz[k], grads_id[k]) for k in grads_id)

    surrogate, module = build(KSLatentConvolutionalLSTM)
    with torch.no_grad():
        times, targets = 0.25 * torch.arange(10), 0.25 * (torch.arange(10) + 1)
        r1 = surrogate.rollout(states=s8[:RO_B, :5], actions=a8[:RO_B, :10], times=times, targets=targets, hidden=None)
        r2 = surrogate.rollout(states=r1.outputs[:, -1, None], actions=a8[:RO_B, 10:], times=times, targets=targets,
                               hidden=r1.hidden)
    for tag, r in (("ro1_", r1), ("ro2_", r2)):
        for name in ("outputs", "deltas", "inlatents", "outlatents"):
            out[tag + name] = getattr(r, name).numpy().copy()
        out[tag + "H"], out[tag + "C"] = r.hidden[0].numpy().copy(), r.hidden[1].numpy().copy()

    g = torch.Generator().manual_seed(2)
    la = torch.rand(8, 20, 1, 4, generator=g) * 2 - 1
    out["lstm_actions"] = la.numpy().copy()
    surrogate, module = build(KSLatentLSTM)
    _, grads = _step(module, surrogate, (s8, la), "lstm_", out, keys=("loss", "hsteploss"))
    for k, v in grads.items():
        if v.size <= LSTM_FULL:
            out["lstm_grad/" + k] = v
        else:
            v64 = v.astype(np.float64)
            out["lstm_gradsum/" + k], out["lstm_gradsq/" + k] = np.float64(v64.sum()), np.float64((v64 * v64).sum())
            out["lstm_gradpick/" + k] = v.reshape(-1)[::PICK].copy()
    return out


def main():
    if not os.path.isdir(os.path.join(gen_golden.REF, "pdecontrol")):
        sys.exit(f"reference checkout not found at {gen_golden.REF}: the latent fixtures can only be generated where it is")
    gen_golden._install_stubs()
    fx = fixtures()
    assert all(np.asarray(v).dtype.kind in "fib" for v in fx.values())
    np.savez_compressed(OUT, **fx)
    print(f"{os.path.relpath(OUT, ROOT)}: {len(fx)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
