"""The decoded-mode loss of the latent surrogate without a GPU: header, binding and library agree on the two entry points of
csrc/sur_decoded.hip; every refusal happens on the host; the numpy oracle of tests/_sur_decoded_oracle.py is the reference's
expression (pdecontrol/surrogates/training.py:100-121, decoded mode) on a chunk-loop rollout that crosses chunk boundaries;
and the routing of the layers above the kernel (module hook, kernel tier, world env) is decided by host-side predicates."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import _latent_models as lm
import _sur_decoded_oracle as do

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "model-based-pde-control_amd", "lib", "libsurrogate_hip.so")
NEW = ("sur_tbptt_decoded_loss", "sur_latent_deltas")


def _lib():
    if not os.path.exists(LIB):
        pytest.skip("libsurrogate_hip.so not built")
    from pdecontrol.surrogates import hipops
    return hipops.load()


def test_header_binding_and_library_agree_on_the_decoded_entry_points():
    from pdecontrol.surrogates import hipops
    text = open(os.path.join(ROOT, "include", "surrogate_hip.h")).read()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)
    table = {name: (res, args) for name, res, args in hipops.SYMBOLS}
    for name in NEW:
        decl = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", text)
        assert decl, f"{name} is not declared in include/surrogate_hip.h"
        assert name in table, f"{name} is not in hipops.SYMBOLS"
        res, args = table[name]
        assert res is ctypes.c_int and len(args) == len(decl.group(1).split(",")), name
    lib = _lib()
    assert all(hasattr(lib, name) for name in NEW)
    assert os.path.exists(os.path.join(ROOT, "model-based-pde-control_amd", "csrc", "sur_decoded.hip"))


def _loss_args(**bad):
    """The arguments of a well-formed sur_tbptt_decoded_loss call on fake pointers, with ``bad`` replacing some."""
    fake = ctypes.c_void_p(16)   # never dereferenced: every call made with these fails its host-side checks first
    a = dict(states=fake, bs=128, ts=64, out_all=fake, b=2, t=2, n=64, delta=0.25, mean=0.0, stdv=1.0, outdeltas=fake,
             deltas=fake, dout_all=fake, hstep=fake, loss=fake, stats=fake, partial=fake, ticket=fake)
    a.update(bad)
    return tuple(a.values())


REFUSALS = [dict(states=None), dict(out_all=None), dict(outdeltas=None), dict(deltas=None), dict(hstep=None), dict(loss=None),
            dict(stats=None), dict(partial=None), dict(ticket=None), dict(b=0), dict(t=1), dict(n=0), dict(b=1 << 20, n=1 << 11),
            dict(bs=63), dict(ts=63), dict(delta=0.0), dict(delta=float("nan")), dict(stdv=0.0), dict(stdv=-1.0),
            dict(stdv=float("nan"))]


@pytest.mark.parametrize("bad", REFUSALS, ids=[",".join(f"{k}={v}" for k, v in r.items()) for r in REFUSALS])
def test_decoded_loss_refuses_bad_arguments_on_the_host(bad):
    lib = _lib()
    assert lib.sur_tbptt_decoded_loss(None, *_loss_args(**bad)) == -1
    assert lib.sur_last_error().decode().startswith("sur_tbptt_decoded_loss:")


def test_latent_deltas_refuses_bad_arguments_on_the_host():
    lib = _lib()
    fake = ctypes.c_void_p(16)
    good = dict(state0=fake, bs=64, out_all=fake, k=3, b=2, n=64, delta=0.25, mean=0.0, stdv=1.0, d_all=fake)
    for bad in (dict(state0=None), dict(out_all=None), dict(d_all=None), dict(k=0), dict(b=0), dict(n=0), dict(bs=63),
                dict(b=1 << 20, n=1 << 11), dict(delta=0.0), dict(stdv=0.0), dict(stdv=float("nan"))):
        assert lib.sur_latent_deltas(None, *dict(good, **bad).values()) == -1, bad
        assert lib.sur_last_error().decode().startswith("sur_latent_deltas:"), bad


# ----------------------------------------------------------------------------------------------------------------------
# the oracle against the reference's expression
# ----------------------------------------------------------------------------------------------------------------------
def _chunk_loop(scaled):
    """A CPU fp32 chunk-loop rollout with T = 13, tbtt = 5, tau = 2: chunks of 5, 5 and 3 steps."""
    sur, module = lm.build(scaled=scaled, perturb=True)
    module.tau, module.tbtt = 2, 5
    g = torch.Generator().manual_seed(3)
    states = torch.rand(3, 13, 1, 64, generator=g) * 2 - 1
    actions = torch.rand(3, 13, 1, 64, generator=g) * 2 - 1
    with torch.no_grad():
        rollouts = module.tbptt_forward(states, actions)
    assert [r.outputs.shape[1] for r in rollouts] == [5, 5, 3]
    return module, states, rollouts


@pytest.mark.parametrize("scaled", [False, True], ids=["identity", "affine"])
def test_oracle_is_the_reference_expression_on_a_chunk_loop_rollout(scaled):
    from pdecontrol.surrogates import hipops
    module, states, rollouts = _chunk_loop(scaled)
    assert module._latent_constants() == hipops.undscale_constants(module.undscaling)
    mean, stdv = module._latent_constants()
    # training.py:100-121 with training_mode == "decoded", on the fp32 rollout
    outputs = torch.cat([r.outputs for r in rollouts], dim=1)
    outdeltas = torch.cat([r.deltas for r in rollouts], dim=1)[:, :-1]
    deltas = module.undscaling(torch.diff(states, dim=1) / module.delta)
    ref = do.decoded_loss_oracle(states[:, :, 0].numpy(), outputs[:, :, 0].transpose(0, 1).contiguous().numpy(), module.delta,
                                 mean, stdv)
    assert np.array_equal(do.bits(ref["outdeltas"]), do.bits(outdeltas[:, :, 0].numpy())), "outdeltas across the chunk boundaries"
    assert np.array_equal(do.bits(ref["deltas"]), do.bits(deltas[:, :, 0].numpy()))
    # ... and the same lines in fp64 on the same values
    out64 = outputs.double().requires_grad_(True)
    decoded = torch.cat((states[:, :1].double(), out64[:, :-1]), dim=1)
    loss = module.loss(decoded, states.double())
    hsteploss = loss.mean(dim=(0, 2, 3)).detach()
    loss = loss.mean()
    loss.backward()
    # fp32 error and square against the exact ones: two roundings on the error's square, one on each term's conversion
    assert do.rel_err([ref["loss"]], [float(loss.detach())]) <= 4 * do.U
    assert ref["hsteploss"][0] == 0.0 and float(hsteploss[0]) == 0.0
    assert do.rel_err(ref["hsteploss"][1:], hsteploss[1:].detach().numpy()) <= 4 * do.U
    want = [outdeltas.double().mean(), outdeltas.double().std(), deltas.double().mean(), deltas.double().std()]
    assert do.rel_err(ref["stats"], [float(v) for v in want]) <= 1e-12
    grad = out64.grad[:, :, 0].transpose(0, 1).numpy()
    assert not ref["dout_all"][-1].any() and not grad[-1].any(), "the last output has no target"
    scale = np.abs(grad).max()
    assert np.all(np.abs(ref["dout_all"] - grad) <= 4 * do.U * np.abs(grad) + 1e-30 * scale)


def test_oracle_summation_orders_agree_within_one_rounding():
    s, o = do.decoded_inputs(5, 7, 205, 40, "padded")
    a, b = do.decoded_loss_oracle(s, o, 0.25, 0.01, math.sqrt(0.5)), do.decoded_loss_oracle(s, o, 0.25, 0.01, math.sqrt(0.5), order=1)
    for key in ("outdeltas", "deltas", "dout_all"):
        assert np.array_equal(do.bits(a[key]), do.bits(b[key]))
    assert do.rel_err(np.float32(b["loss"]), a["loss"]) <= do.U and do.rel_err(b["stats"].astype(np.float32), a["stats"]) <= do.U
    assert do.rel_err(b["hsteploss"][1:].astype(np.float32), a["hsteploss"][1:]) <= do.U and a["hsteploss"][0] == b["hsteploss"][0] == 0.0
    d = do.latent_deltas_oracle(s[:, 0], o, 0.25, 0.01, math.sqrt(0.5))
    assert np.array_equal(do.bits(d[:-1].transpose(1, 0, 2)), do.bits(a["outdeltas"])), "sur_latent_deltas: the same rows"


# ----------------------------------------------------------------------------------------------------------------------
# routing
# ----------------------------------------------------------------------------------------------------------------------
def test_latent_constants_follow_the_configuration():
    from pdegym.common.transforms import BatchTransform, ScaleTransform
    _, plain = lm.build()
    _, scaled = lm.build(scaled=True)
    assert plain._latent_constants() == (0.0, 1.0)
    mean, stdv = scaled._latent_constants()
    assert mean == float(np.float32(0.01)) and stdv == float(np.sqrt(np.float32(0.5) + np.float32(1e-4)))
    # the loss, a scaling the kernels do not take, two scalings that differ, another architecture
    _, m = lm.build()
    m.loss = torch.nn.MSELoss()
    assert m._latent_constants() is None
    _, m = lm.build()
    m.surrogate.dscaling = BatchTransform(ScaleTransform())
    assert m._latent_constants() is None
    _, m = lm.build(scaled=True)
    m.surrogate.dscaling = plain.surrogate.dscaling
    assert m._latent_constants() is None
    import _grad_contract_models as gm
    assert gm.ks_module(64, False)._latent_constants() is None
    # on the CPU the hook never takes the step
    s = torch.zeros(2, 13, 1, 64)
    assert plain._latent_training_step((s, s)) is None


def test_fused_supported_stays_false_for_latent_members():
    from pdecontrol.surrogates import hipops
    sur, _ = lm.build()
    assert hipops.fused_latent_supported(sur) and not hipops.fused_supported(sur)
    assert hipops.latent_scale_constants(sur) == (0.0, 1.0)
