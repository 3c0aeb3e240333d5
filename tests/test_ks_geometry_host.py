"""The KS stepper's CPU twin (device = -1) at every grid size the geometry tests use on the GPU, against the oracle: the
layout table itself, both modes and objectives, the actions and subset entries, and zeros of both signs under the upwind
switch.  Runs without a GPU; it also shows that the inputs of test_ks_geometry_gpu.py keep the contract's tolerances for a
correct implementation.

Observed on the twin over all 19 sizes (ks_geometry_observed.jsonl, "where": "cpu"): fast mode state L_inf
<= 8.4e-16, l2 accumulator <= 2.1e-15 and dissipation accumulator <= 2.3e-14 relative; exact mode l2 accumulator equal,
dissipation accumulator <= 2.6e-15 relative.
"""
import numpy as np
import pytest

import _ks_geometry as g
from oracle import ks_oracle as ko

TWIN_N = g.MATRIX_N + (9, 63, 65, 333, 1637, 1638, 2048)


@pytest.fixture(scope="module")
def kspde():
    import kspde
    kspde.load()
    return kspde


def test_layout_table_has_forty_layouts_and_the_two_hybrids():
    fused = {(v, p) for v, p in g.LAYOUT_TABLE if v in g.FUSED}
    assert len(fused) == 40 and len(g.LAYOUT_TABLE) == 42
    # section 1's sizes reach every pair
    reached = {(v, N // g.lanes_of(v)) for N in g.MATRIX_N for v in g.FUSED + g.HYBRID if g.supported(v, N)}
    assert reached == g.LAYOUT_TABLE
    # the table the two older GPU test files used to restate, value for value
    def old(variant, N):
        if variant.startswith("wave64_hybrid"):
            return N == 64
        P = {"row16": 16, "wave64": 64, "half32": 32}.get(variant.split("_")[0])
        if P is None:
            return 9 <= N <= 2048
        return N % P == 0 and (N // P) in (1, 2, 3, 4, 6, 8, 12, 16)
    for v in g.VARIANTS:
        for N in range(1, 2100):
            assert g.supported(v, N) == old(v, N), (v, N)


def test_expected_layout_grid_formula():
    assert g.expected_layout("row16_dpp", 64, 5, 0) == {"variant": "row16_dpp", "lanes_per_env": 16, "points_per_lane": 4,
                                                        "block": 64, "grid": 2}
    assert g.expected_layout("wave64_bperm", 192, 5, 128)["grid"] == 3
    assert g.expected_layout("half32_bperm", 96, 5, 256)["grid"] == 1
    assert g.expected_layout("lds", 100, 5, 0) == {"variant": "lds", "lanes_per_env": 0, "points_per_lane": 0,
                                                   "block": 128, "grid": 5}


@pytest.mark.parametrize("N", TWIN_N)
def test_cpu_twin_against_the_oracle(kspde, N):
    u0, phi, ref = g.case(N, 5, (1, 20))
    s = kspde.KSStepper(5, N, g.length_of(N), g.DT, device=-1)
    for mode in ("exact", "fast"):
        seen = g.check_steps(s, u0, phi, ref, mode, label=f"cpu N={N}")
        g.record(where="cpu", N=N, variant="cpu", block=0, mode=mode, **seen)


@pytest.mark.parametrize("N", TWIN_N)
def test_cpu_twin_actions_and_subset_entries(kspde, N):
    s = kspde.KSStepper(5, N, g.length_of(N), g.DT, device=-1)
    g.check_actions_path(s, N, 5, label=f"cpu N={N}")
    t = kspde.KSStepper(g.subset_envs(N), N, g.length_of(N), g.DT, device=-1)
    g.check_step_rows(t, N, label=f"cpu N={N}")
    g.check_step_device_subset(t, N, *g.host_buffers(), label=f"cpu N={N}")


@pytest.mark.parametrize("N", g.ZERO_N)
def test_cpu_twin_zeros_under_the_upwind_switch(kspde, N):
    s = kspde.KSStepper(6, N, g.length_of(N), g.DT, device=-1)
    for forced in (False, True):
        u0, phi, ref = g.zero_case(N, forced)
        for mode in ("exact", "fast"):
            g.check_steps(s, u0, phi, ref, mode, label=f"cpu N={N} zeros forced={forced}")
            if not forced:
                g.check_zero_rows_stay_zero(s, u0, phi, mode, label=f"cpu N={N}")
        for got, want, name in zip(s.rhs(u0, phi), ko.rhs(u0, phi, g.length_of(N) / N), ("rhs", "ux", "uxx", "uxxxx")):
            np.testing.assert_array_equal(got, want, err_msg=f"N={N} {name}")


def test_zero_inputs_hold_the_zeros_they_claim():
    for N in g.ZERO_N:
        u0, phi, _ = g.zero_case(N, False)
        assert (u0[0, ::5] == 0).all() and not np.signbit(u0[0, ::5]).any()
        assert (u0[1, ::3] == 0).all() and np.signbit(u0[1, ::3]).all()
        assert not u0[2].any() and not np.signbit(u0[2]).any()
        assert not u0[3].any() and np.signbit(u0[3]).all()
        assert (u0[4, [0, N - 1]] == 0).all() and not np.signbit(u0[4, [0, N - 1]]).any()
        assert (u0[5, [0, N - 1]] == 0).all() and np.signbit(u0[5, [0, N - 1]]).all()
        assert not phi[list(g.ZERO_ROWS)].any()
        assert np.count_nonzero(u0[0]) == N - len(range(0, N, 5)) and np.count_nonzero(u0[4]) == N - 2
        # a wrong pick at a zero is visible: forward and backward derivatives differ there by far more than the bound
        _, ux, _, _ = ko.rhs(u0, phi, g.length_of(N) / N)
        flipped = np.where(u0 == 0, np.nextafter(0, -1), u0)      # the same state, the zeros a hair below: forward
        _, ux_f, _, _ = ko.rhs(flipped, phi, g.length_of(N) / N)
        at = (u0[0] == 0)
        assert np.abs(ux[0, at] - ux_f[0, at]).max() * 0.5 * g.DT > 1e-6


@pytest.mark.parametrize("N", (9, 64, 333, 2048))
def test_cpu_twin_reward_rows(kspde, N):
    s = kspde.KSStepper(1, N, g.length_of(N), g.DT, device=-1)
    for n_rows in g.REWARD_ROWS:
        obs, phi, refs = g.reward_case(N, n_rows)
        for (objective, with_phi), (ref, bound) in refs.items():
            out = np.full(n_rows + 1, g.SENTINEL)
            s.reward_rows_device(objective, obs.ctypes.data, phi.ctypes.data if with_phi else 0, n_rows, out.ctypes.data)
            assert out[n_rows] == g.SENTINEL
            err = np.abs(out[:n_rows] - ref)
            assert (err <= bound).all(), (N, n_rows, objective, with_phi, float((err / bound).max()))
