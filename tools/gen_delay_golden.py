#!/usr/bin/env python3
"""Golden vectors of the delay-embedding surrogate ablation -> tests/golden/delay_golden.npz (run in the build container).

Runs the reference's own ``KSDelayCNNSurrogateFactory`` (pdecontrol/architectures/delay.py:19-79), ``DelayTransitionModel``
(pdecontrol/surrogates/transition.py:299-382), ``AutoRegPDESurrogate`` (pdecontrol/surrogates/surrogate.py:58-133) and
``PDETrainingModule.training_step`` (pdecontrol/surrogates/training.py:64-130) from the reference checkout, behind the stubs
of oracle/gen_golden.py, on seeded inputs, and records only numbers.  N = 64, B = 8, T = 20, tau = 5, tbtt = 10,
MSELoss(reduction="none").

What is recorded (keys):
  sd/<name>                     the seeded (torch.manual_seed(0)) state_dict, in full up to FULL elements
  sdsum/, sdsq/, sdpick/        for the two larger MLP weights (288 x 96 and 96 x 64): fp64 sum, sum of squares and every
                                PICK-th element
  (the batch)                   states: surrogate_golden.npz's b8_states [8, 20, 1, 64]; actions: latent_golden.npz's
                                lstm_actions [8, 20, 1, 4] (checked here, not stored twice)
  id_*, nz_*                    training_step with identity dscaling / undscaling, and with Normalize(scalar stats)
                                undscaling and its inverse as dscaling: loss, hsteploss, outputs, outdeltas, and every
                                gradient (grad/<name> in full up to FULL elements; gradsum/, gradsq/, gradpick/ otherwise)
  ro1_*, ro2_*                  rollout API: warm-up on 5 given states over 10 steps, then the context carried into a
                                second call from the last prediction; outputs, deltas, inlatents, outlatents and both
                                context tensors (S, A) of the first RO_B samples.  The reference writes slot 0 of a context
                                passed in, so ro1's is copied before the second call.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_delay_golden.py
"""
import os
import sys

sys.dont_write_bytecode = True  # never write __pycache__ into the reference checkout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import gen_golden  # noqa: E402  (pins the CPU arithmetic before torch is imported)
import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "delay_golden.npz")
SHARED = os.path.join(ROOT, "tests", "golden", "surrogate_golden.npz")
SHARED_ACTIONS = os.path.join(ROOT, "tests", "golden", "latent_golden.npz")
RO_B = 1
FULL = 4096
PICK = 97


def _store(out, prefix, name, v):
    if v.size <= FULL:
        out[prefix + "/" + name] = v.copy()
    else:
        v64 = v.astype(np.float64)
        out[prefix + "sum/" + name], out[prefix + "sq/" + name] = np.float64(v64.sum()), np.float64((v64 * v64).sum())
        out[prefix + "pick/" + name] = v.reshape(-1)[::PICK].copy()


def fixtures():
    from pdecontrol.architectures.delay import KSDelayCNNSurrogateFactory
    from pdecontrol.surrogates.training import PDETrainingModule
    from pdegym.common.transforms import BatchTransform, Normalize

    def build(dscaling=None, undscaling=None):
        torch.manual_seed(0)
        factory = KSDelayCNNSurrogateFactory()
        model = factory.model()
        surrogate = factory.surrogate(delta=0.25, dscaling=dscaling, tau=5, **model)
        module = PDETrainingModule(surrogate=surrogate, loss=torch.nn.MSELoss(reduction="none"), tstep=0.25, delta=0.25,
                                   undscaling=undscaling, tau=5, tbtt=10)
        return surrogate, module

    out = {}
    surrogate, module = build()
    for k, v in surrogate.state_dict().items():
        _store(out, "sd", k, v.numpy())

    shared, shared_a = np.load(SHARED), np.load(SHARED_ACTIONS)
    s8, a8 = torch.from_numpy(shared["b8_states"]), torch.from_numpy(shared_a["lstm_actions"])

    norm = Normalize(aggregate=True, batched=True)
    norm.mean, norm.var, norm.count = torch.full((1, 1, 1), 0.01), torch.full((1, 1, 1), 0.5), 100
    undscaling = BatchTransform(norm)
    for tag, (dsc, und) in (("id_", (None, None)), ("nz_", (undscaling.Inverse, undscaling))):
        surrogate, module = build(dscaling=dsc, undscaling=und)
        res = module.training_step((s8, a8), 0)
        res["loss"].backward()
        out[tag + "loss"] = np.float64(res["loss"].item())
        for k in ("hsteploss", "outputs", "outdeltas"):
            out[tag + k] = res[k].numpy().copy()
        assert np.array_equal(res["deltas"].numpy(), shared["b8_deltas" if tag == "id_" else "b8n_deltas"])
        for k, p in surrogate.named_parameters():
            if p.grad is not None:
                _store(out, tag + "grad", k, p.grad.numpy())

    surrogate, module = build()
    with torch.no_grad():
        times, targets = 0.25 * torch.arange(10), 0.25 * (torch.arange(10) + 1)
        r1 = surrogate.rollout(states=s8[:RO_B, :5], actions=a8[:RO_B, :10], times=times, targets=targets, hidden=None)
        h1 = tuple(h.clone() for h in r1.hidden)
        r2 = surrogate.rollout(states=r1.outputs[:, -1, None], actions=a8[:RO_B, 10:], times=times, targets=targets,
                               hidden=r1.hidden)
    for tag, r, h in (("ro1_", r1, h1), ("ro2_", r2, r2.hidden)):
        for name in ("outputs", "deltas", "inlatents", "outlatents"):
            out[tag + name] = getattr(r, name).numpy().copy()
        out[tag + "S"], out[tag + "A"] = h[0].numpy().copy(), h[1].numpy().copy()
    return out


def main():
    if not os.path.isdir(os.path.join(gen_golden.REF, "pdecontrol")):
        sys.exit(f"reference checkout not found at {gen_golden.REF}: the delay fixtures can only be generated where it is")
    gen_golden._install_stubs()
    fx = fixtures()
    assert all(np.asarray(v).dtype.kind in "fib" for v in fx.values())
    np.savez_compressed(OUT, **fx)
    print(f"{os.path.relpath(OUT, ROOT)}: {len(fx)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
