"""Every instantiated KS stepper layout, block size and grid size on the MI355X against the oracle.

  1. layout matrix   all 40 (variant, points per lane) layouts of ks_rk4_fused, the two hybrids and the LDS kernel, each
                     at block 0 / 64 / 128 / 256 (whole inactive waves and tail groups inside a multi-wave workgroup), both
                     modes, both objectives; a closing test fails if any layout of the table was not run
  2. entries         in-kernel actions @ F, step_rows and step_device(d_env_ids) under every layout
  3. LDS kernel      N from 9 to 2048 (more than 64 KiB of dynamic LDS from N = 1638 on), refusal at 2049
  4. per-row reward  every lane-group width, N that is no multiple of it, ragged rows, phi = NULL
  5. zeros           +0.0 / -0.0 under the upwind switch: u == 0 selects the backward stencil

Inputs, references, tolerances and the recorder: _ks_geometry.py.  What was observed goes to stdout and to
ks_geometry_observed.jsonl beside the suite's other observation logs (_ks_geometry.OBSERVED), one line per (N, variant, block, mode).
"""
import numpy as np
import pytest
import torch

import _ks_geometry as g
from oracle import ks_oracle as ko

pytestmark = pytest.mark.gpu

E = 5
SEEN = set()        # (variant, points per lane) as layout() reported them, filled by test_layout_matrix


@pytest.fixture(scope="module")
def kspde():
    import kspde
    kspde.load()
    return kspde


def _torch_buffers():
    def to_device(a):
        t = torch.from_numpy(np.array(a, copy=True)).cuda()
        torch.cuda.synchronize()
        return t, t.data_ptr()
    return to_device, lambda t: t.cpu().numpy()


def _refused(kspde, call):
    with pytest.raises(kspde.KSError) as e:
        call()
    assert f"error {g.KS_ERR_UNSUPPORTED}" in str(e.value), str(e.value)


# ---- 1. layout matrix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", g.MATRIX_N)
def test_layout_matrix(kspde, N):
    u0, phi, ref = g.case(N, E, (1, 20))
    s = kspde.KSStepper(E, N, g.length_of(N), g.DT)
    for variant in g.VARIANTS:
        if not g.supported(variant, N):
            _refused(kspde, lambda: s.set_variant(variant))
            continue
        s.set_variant(variant)
        objectives = ("l2control",) if variant in g.HYBRID else ("l2control", "dissipation")
        for block in g.BLOCKS:
            s.set_block_size(block)
            lay = s.layout()
            assert lay == g.expected_layout(variant, N, E, block), (variant, block, lay)
            for mode in ("exact", "fast"):
                seen = g.check_steps(s, u0, phi, ref, mode, objectives, label=f"N={N} {variant} block={block}")
                g.record(where="gpu", section="matrix", N=N, variant=variant, P=lay["points_per_lane"], block=lay["block"],
                         block_set=block, grid=lay["grid"], mode=mode, **seen)
        if variant != "lds":
            SEEN.add((lay["variant"], lay["points_per_lane"]))
        s.set_block_size(0)


def test_every_instantiated_layout_ran():
    """Closes section 1: the layouts test_layout_matrix ran (as layout() named them) are the whole table -- the 40
    (variant, P) pairs of the five fused families and the two hybrids at P = 1.  A layout that was silently skipped fails
    here.  (Needs test_layout_matrix to have run in this session.)"""
    missing, extra = sorted(g.LAYOUT_TABLE - SEEN), sorted(SEEN - g.LAYOUT_TABLE)
    print(f"ks geometry: {len(SEEN & g.LAYOUT_TABLE)} of {len(g.LAYOUT_TABLE)} layouts run "
          f"({len({x for x in SEEN if x[0] in g.FUSED})} of 40 fused)")
    assert not missing and not extra, f"not run: {missing}; not in the table: {extra}"


# ---- 2. entries per layout -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", g.MATRIX_N)
def test_entries_per_layout(kspde, N):
    s = kspde.KSStepper(E, N, g.length_of(N), g.DT)
    t = kspde.KSStepper(g.subset_envs(N), N, g.length_of(N), g.DT)
    bufs = _torch_buffers()
    for variant in g.VARIANTS:
        if not g.supported(variant, N):
            continue
        for h in (s, t):
            h.set_variant(variant)
            h.set_block_size(256)
            assert h.layout()["variant"] == variant and h.layout()["block"] == 256
        label = f"N={N} {variant}"
        g.check_actions_path(s, N, E, label=label)
        g.check_step_rows(t, N, label=label)
        g.check_step_device_subset(t, N, *bufs, label=label)


# ---- 3. LDS kernel range ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (9, 63, 65, 1637, 1638, 2048))
def test_lds_kernel_range(kspde, N):
    """N = 1638 is the first size whose dynamic LDS (8 * (5 N + block / 64) bytes) passes 64 KiB at 256 threads; 2048
    needs 81 952 B."""
    u0, phi, ref = g.case(N, 3, (1, 5))
    s = kspde.KSStepper(3, N, g.length_of(N), g.DT, variant="lds")
    for block in (64, 128, 256):
        s.set_block_size(block)
        assert s.layout() == g.expected_layout("lds", N, 3, block)
        for mode in ("exact", "fast"):
            seen = g.check_steps(s, u0, phi, ref, mode, label=f"N={N} lds block={block}")
            g.record(where="gpu", section="lds", N=N, variant="lds", P=0, block=block, block_set=block, grid=3, mode=mode,
                     **seen)


def test_lds_kernel_refuses_beyond_its_range(kspde):
    N = g.LDS_N[1] + 1
    _refused(kspde, lambda: kspde.KSStepper(3, N, g.length_of(N), g.DT, variant="lds"))
    s = kspde.KSStepper(3, N, g.length_of(N), g.DT)         # auto: no layout serves this N
    u0, phi, _ = g.inputs(N, 3)
    s.set_state(u0)
    _refused(kspde, lambda: s.step(phi, 1))
    _refused(kspde, s.layout)
    np.testing.assert_array_equal(s.get_state(), u0)        # nothing was launched
    # and the last size inside the range is served
    assert kspde.KSStepper(3, g.LDS_N[1], g.length_of(g.LDS_N[1]), g.DT, variant="lds").layout()["variant"] == "lds"


# ---- 4. per-row reward kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", g.REWARD_N)
def test_reward_rows_kernel(kspde, N):
    """G = 16 serves N <= 64, G = 32 up to 512, G = 64 above; the bound is derived in _ks_geometry.reward_case."""
    s = kspde.KSStepper(1, N, g.length_of(N), g.DT)
    worst = 0.0
    for n_rows in g.REWARD_ROWS:
        obs, phi, refs = g.reward_case(N, n_rows)
        d_obs, d_phi = torch.from_numpy(obs.copy()).cuda(), torch.from_numpy(phi.copy()).cuda()
        for (objective, with_phi), (ref, bound) in refs.items():
            out = torch.full((n_rows + 1,), g.SENTINEL, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            s.reward_rows_device(objective, d_obs.data_ptr(), d_phi.data_ptr() if with_phi else 0, n_rows, out.data_ptr())
            s.sync()
            got = out.cpu().numpy()
            assert got[n_rows] == g.SENTINEL, "the element behind the last row was written"
            err = np.abs(got[:n_rows] - ref)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (N, n_rows, objective, with_phi, float((err / bound).max()))
    g.record(where="gpu", section="reward_rows", N=N, worst_error_over_bound=worst)


# ---- 5. zeros under the upwind switch --------------------------------------------------------------------------------
@pytest.mark.parametrize("N", g.ZERO_N)
def test_zeros_under_the_upwind_switch(kspde, N):
    s = kspde.KSStepper(6, N, g.length_of(N), g.DT)
    for variant in g.VARIANTS:
        if not g.supported(variant, N):
            continue
        s.set_variant(variant)
        objectives = ("l2control",) if variant in g.HYBRID else ("l2control", "dissipation")
        for forced in (False, True):
            u0, phi, ref = g.zero_case(N, forced)
            for mode in ("exact", "fast"):
                label = f"N={N} {variant} zeros forced={forced}"
                seen = g.check_steps(s, u0, phi, ref, mode, objectives, label=label)
                if not forced:
                    g.check_zero_rows_stay_zero(s, u0, phi, mode, label=label)
                g.record(where="gpu", section="zeros", N=N, variant=variant, forced=forced, block=s.layout()["block"],
                         mode=mode, **seen)
    for forced in (False, True):
        u0, phi, _ = g.zero_case(N, forced)
        for got, want, name in zip(s.rhs(u0, phi), ko.rhs(u0, phi, g.length_of(N) / N), ("rhs", "ux", "uxx", "uxxxx")):
            np.testing.assert_array_equal(got, want, err_msg=f"N={N} {name}")
