"""The fp64 oracle of the whole-network FNO kernels (tests/_fno_oracle.py) against the module it is built on -- no GPU.

tests/test_fno_kernels_gpu.py compares what csrc/fno.hip saves and emits per (step, sample) pair with this oracle; here the
oracle's per-pair tensors are tied to ``FNO1d.double()``'s own autograd, the fp32 yardstick's GELU to the exact one, and the
stress weight set to the GELU argument range it is there to reach."""
import math

import numpy as np
import pytest
import torch

import _fno_oracle as fo

PAIRS = 6


def _module_grads(model, u, act, gdelta):
    """autograd gradients of sum(gdelta * delta) through the module itself, over the whole batch"""
    model.zero_grad(set_to_none=True)
    delta = model(torch.stack((u.double(), act.double()), 1))[:, 0]
    (gdelta.double() * delta).sum().backward()
    return {k: p.grad.numpy().copy() for k, p in model.named_parameters()}, delta.detach().numpy()


@pytest.fixture(scope="module", params=[("default", 64), ("stress", 64), ("stress", 128)], ids=lambda p: f"{p[0]}-N{p[1]}")
def case(request):
    weights, n = request.param
    model = fo.make_model(weights)
    u, act, gdelta, _ = fo.inputs(n, PAIRS)
    w = fo.walk(model, u, act, gdelta=gdelta)
    grads, delta = _module_grads(model, u, act, gdelta)
    return w, grads, delta


def _assert_rel(got, ref, tol, what):
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max()) / scale
    assert err <= tol, f"{what}: {err:.3e} of its scale"


def test_rows_summed_over_pairs_are_the_module_gradients(case):
    w, grads, delta = case
    _assert_rel(w["delta"], delta, 1e-12, "delta")
    total = w["rows"].sum(0)
    assert total.shape == (fo.ROW_DEFINED,) and fo.ROW_DEFINED == 5409
    covered = np.zeros(fo.ROW_DEFINED, dtype=int)
    for name, sl in fo.row_slices().items():
        covered[sl] += 1
        _assert_rel(total[sl], grads[name].reshape(-1), 1e-12, name)
    assert (covered == 1).all(), "the named slices tile the defined columns exactly once"


def test_saved_spectra_contract_to_the_spectral_weight_gradients(case):
    """dWr = sum_p Gr Xr + Gi Xi, dWi = sum_p Gi Xr - Gr Xi from the oracle's xspec / gspec [4][32 k][P][32 c] == autograd's
    weight_real.grad / weight_imag.grad: the definition of the saved spectra (re | im split, unscaled X, s_0 = 1/N and
    s_m = 2/N on G, rfft's sign) is the module's."""
    w, grads, _ = case
    X, G = w["xspec"], w["gspec"]
    assert X.shape == G.shape == (fo.LAYERS, fo.K2, PAIRS, fo.WIDTH)
    for l in range(fo.LAYERS):
        xr, xi, gr, gi = X[l, :fo.MODES], X[l, fo.MODES:], G[l, :fo.MODES], G[l, fo.MODES:]      # [m, p, c]
        dwr = np.einsum("mpo,mpi->iom", gr, xr) + np.einsum("mpo,mpi->iom", gi, xi)
        dwi = np.einsum("mpo,mpi->iom", gi, xr) - np.einsum("mpo,mpi->iom", gr, xi)
        _assert_rel(dwr, grads[f"spectral.{l}.weight_real"], 1e-12, f"layer {l} weight_real")
        # the imaginary part of mode 0 is dropped by irfft: its weight has no gradient, and the formula agrees (Xi = Gi = 0)
        _assert_rel(dwi, grads[f"spectral.{l}.weight_imag"], 1e-12, f"layer {l} weight_imag")


def test_saved_spectra_are_rfft_of_the_layer_inputs_and_of_d_pre(case):
    w, _, _ = case
    n = w["x"].shape[-1]
    for l in range(fo.LAYERS):
        f = np.fft.rfft(w["x"][:, l], axis=-1)[..., :fo.MODES]                                  # [p, c, m]
        np.testing.assert_allclose(w["xspec"][l, :fo.MODES], f.real.transpose(2, 0, 1), rtol=0, atol=1e-11)
        np.testing.assert_allclose(w["xspec"][l, fo.MODES:], f.imag.transpose(2, 0, 1), rtol=0, atol=1e-11)
        g = np.fft.rfft(w["dpre"][:, l], axis=-1)[..., :fo.MODES] * (np.r_[1.0, np.full(fo.MODES - 1, 2.0)] / n)
        np.testing.assert_allclose(w["gspec"][l, :fo.MODES], g.real.transpose(2, 0, 1), rtol=0, atol=1e-12)
        np.testing.assert_allclose(w["gspec"][l, fo.MODES:], g.imag.transpose(2, 0, 1), rtol=0, atol=1e-12)


def test_gout_and_given_pre_activations():
    """dbase carries gout through (out = u + cscale * delta + cshift), gout acts on delta with weight cscale, and a walk that
    is handed its own pre-activations is the same walk."""
    model = fo.make_model("stress")
    u, act, gdelta, gout = fo.inputs(64, 3)
    cs = 0.37
    plain = fo.walk(model, u, act, cscale=cs, cshift=-0.2, gdelta=gdelta)
    fused = fo.walk(model, u, act, cscale=cs, cshift=-0.2, gdelta=gdelta.double() + cs * gout.double())
    w = fo.walk(model, u, act, cscale=cs, cshift=-0.2, gdelta=gdelta, gout=gout)
    np.testing.assert_allclose(w["out"], u.double().numpy() + cs * w["delta"] - 0.2, rtol=0, atol=1e-15)
    np.testing.assert_allclose(w["rows"], fused["rows"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(w["dbase"], fused["dbase"] + gout.double().numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(w["dact"], fused["dact"], rtol=1e-12, atol=1e-14)
    assert np.abs(w["rows"] - plain["rows"]).max() > 1e-3          # and gout is not a no-op
    again = fo.walk(model, u, act, cscale=cs, cshift=-0.2, gdelta=gdelta, gout=gout, pre_given=torch.from_numpy(w["pre"]))
    for k in ("rows", "gspec", "dbase", "dact", "delta"):
        np.testing.assert_array_equal(again[k], w[k], err_msg=k)


def test_yardstick_gelu_within_the_abramowitz_stegun_bound():
    """The yardstick's GELU (the kernels' formula in torch fp32: A&S 7.1.26, |erf error| <= 1.5e-7, from one exponential)
    against the exact erf form in fp64 on a grid of 480 001 points over [-12, 12].

    Bounds, from the formula alone: the cdf is off by half the erf bound (0.75e-7) plus at most four fp32 roundings of a
    value <= 1 (polynomial, the fma with the exponential, the sum, the halving: 4 * 2^-24); the value x * cdf scales that by
    |x| and rounds once more; the derivative adds |x| * pdf, whose relative error is the exponential's (argument rounding
    x^2 / 2 * 2^-24 plus two roundings), at most 2^-22 in absolute terms.
    Measured here (libm's exp): max |gelu error| 4.61e-7 (at x = 4.03), max |gelu' error| 2.64e-7 (at x = 0.03); a numpy
    emulation without the fp64 fma gives 4.6e-7 / 3.2e-7, which the two flat caps at the end round up."""
    x = torch.linspace(-12.0, 12.0, 480001, dtype=torch.float64).float()
    xd = x.double()
    cdf = 0.5 * (1.0 + torch.erf(xd / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * xd * xd) / math.sqrt(2.0 * math.pi)
    ev = (fo.as_gelu(x).double() - xd * cdf).abs()
    ed = (fo.as_gelu_grad(x).double() - (cdf + xd * pdf)).abs()
    print(f"yardstick GELU: max |value error| {float(ev.max()):.3e} at x = {float(x[ev.argmax()]):.3f}, "
          f"max |derivative error| {float(ed.max()):.3e} at x = {float(x[ed.argmax()]):.3f}")
    eps = 2.0 ** -24
    ax = xd.abs()
    assert bool((ev <= (0.75e-7 + 4 * eps) * ax + eps * (xd * cdf).abs() + 1e-12).all())
    assert bool((ed <= 0.75e-7 + 4 * eps + 4 * eps + 1e-12).all())
    assert float(ev.max()) <= 5.0e-7 and float(ed.max()) <= 4.0e-7
    # the autograd.Function's backward is gelu_grad: x * pdf + cdf
    xg = x[::1000].clone().requires_grad_(True)
    fo.as_gelu(xg).sum().backward()
    np.testing.assert_array_equal(xg.grad.numpy(), fo.as_gelu_grad(x[::1000]).numpy())


@pytest.mark.parametrize("n", [64, 128, 512])
def test_stress_weights_reach_the_gelu_tails(n):
    """Every GELU argument set (pre_0, pre_1, pre_2, z1) of the stress set has >= 16 entries in [1, 2) and in [2, 4) on
    each sign, and at least one set reaches [4, 8); the default set stays at |x| <= 1.05 (what the older tests cover)."""
    u, act, _, _ = fo.inputs(n, PAIRS)
    cov = fo.coverage(fo.walk(fo.make_model("stress"), u, act))
    assert sorted(cov) == ["pre_0", "pre_1", "pre_2", "z1"]
    for name, c in cov.items():
        for lo, hi in ((1, 2), (2, 4)):
            for sg in (1, -1):
                assert c[(lo, hi, sg)] >= 16, (n, name, lo, hi, sg, c[(lo, hi, sg)])
    assert any(c[(4, 8, sg)] > 0 for c in cov.values() for sg in (1, -1))
    args = fo.gelu_arguments(fo.walk(fo.make_model("default"), u, act))
    assert max(float(np.abs(v).max()) for v in args.values()) <= 1.05


def test_yardstick_walk_is_the_oracle_walk_in_fp32():
    """Dense transforms and the A&S GELU change nothing beyond fp32 noise: every tensor of the yardstick within 1e-5 of its
    scale of the oracle (a wrong sign, scale or layout in the yardstick's own spelling would show at order 1)."""
    u, act, gdelta, gout = fo.inputs(64, 3)
    for weights in fo.WEIGHT_SETS:
        ref = fo.walk(fo.make_model(weights), u, act, cscale=0.5, cshift=0.1, gdelta=gdelta, gout=gout)
        got = fo.fp32_as_walk(fo.make_model(weights, torch.float32), u, act, cscale=0.5, cshift=0.1, gdelta=gdelta, gout=gout)
        for k in ("pre", "xspec", "delta", "out", "gspec", "dbase", "dact"):
            _assert_rel(got[k], ref[k], 1e-5, f"{weights} {k}")
        for name, sl in fo.row_slices().items():
            _assert_rel(got["rows"][:, sl], ref["rows"][:, sl], 1e-5, f"{weights} rows {name}")
