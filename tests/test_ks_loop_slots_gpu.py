"""The fast-mode sub-step loop with its non-arithmetic issue slots shed (csrc/ks_kernels.hip) against the loop as it was.

libkspde.so waits for the prologue's loads once in front of the loop and lands the stage-4 update in u's registers
without a copy (a three-address v_fma_f64 in an asm statement); libkspde_loop0.so (the same sources with -DKS_LOOP0) keeps
the earlier form.  No floating-point operation, operand or order differs, so every output must agree bit for bit: this
process steps with libkspde.so, one child process (KSPDE_LIB = libkspde_loop0.so) steps the same inputs, and state, fp32
obs, reward accumulator and status are compared on their raw bytes.  (The cases are the ones that also caught the form
in which a tile's first compare wrote EXEC itself, DESIGN 4.1: masks of every kind at the first point of every tile.)

  layouts     every fused fast-mode layout with a tile of more than one point: N = 32, 48, 64, 96, 128, 192, 256 at
              16 lanes per env (2, 3, 4, 6, 8, 12, 16 points per lane; tiles of 2, 3, 4, 3, 4, 4, 4), N = 128 and 256 at
              32 and at 64 lanes per env, every variant with that many lanes; and N = 64 at one point per lane (no tile
              select, the same loop), the two hybrid layouts included
  envs        E = 5: the last wave has a tail group that redoes the last env
  sub-steps   1 and 3 (the loop-carried registers go round more than once; the reward accumulator after 3)
  objectives  l2control and dissipation
  rows        0 all positive (empty masks), 1 all negative (full masks), 2 sign alternating per point, 3 mixed signs
              with +0.0 / -0.0 alternating at the first point of every tile, 4 mixed signs from U(-2, 2) (mixed masks
              at the first point of the tiles)
  non-finite  the same with a NaN in env 1 and an inf in env 3: the two libraries agree on every byte, the status
              flags are set for exactly these envs, and the finite envs equal the run without them

Run as a script (the child): ``python tests/test_ks_loop_slots_gpu.py OUT.npz`` steps every case with the library
KSPDE_LIB names and saves the outputs.
"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "model-based-pde-control_amd")

VARIANTS = {16: ("row16_dpp", "row16_bperm"), 32: ("half32_bperm",), 64: ("wave64_dpp", "wave64_bperm")}
HYBRID = ("wave64_hybrid", "wave64_hybrid1")        # N = 64 only, one point per lane, l2control only
# (64, 64) is one point per lane: no tile select, but the same loop (waits, stage-4 update), and the hybrid layouts
LAYOUTS = [(N, 16) for N in (32, 48, 64, 96, 128, 192, 256)] + [(N, G) for G in (32, 64) for N in (128, 256)] + [(64, 64)]
SUBSTEPS = (1, 3)
OBJECTIVES = ("l2control", "dissipation")
E = 5
DT = 1e-3
L_PER_POINT = 0.34375
NAN_ENV, INF_ENV = 1, 3
FIELDS = ("state", "obs", "acc", "status")
CHILD_TIMEOUT = 240


def variants(N, G):
    return VARIANTS[G] + (HYBRID if (N, G) == (64, 64) else ())


def tile(P):
    return 4 if P % 4 == 0 else (3 if P % 3 == 0 else (2 if P % 2 == 0 else 1))


def inputs(N, G):
    """(u0 [E, N] f64, phi [E, N] f32): one row per sign pattern of the module docstring."""
    rs = np.random.RandomState(2000 + N + G)
    u0 = rs.uniform(-2.0, 2.0, (E, N))
    phi = rs.uniform(-0.5, 0.5, (E, N)).astype(np.float32)
    u0[0] = np.abs(u0[0]) + 0.5                      # stays positive over 3 sub-steps of dt = 1e-3
    u0[1] = -np.abs(u0[1]) - 0.5
    u0[2] = np.abs(u0[2]) * np.where(np.arange(N) % 2, -1.0, 1.0)
    first = np.arange(0, N, tile(N // G))            # P is a multiple of the tile: the tiles start at multiples of it
    u0[3, first[0::2]] = 0.0
    u0[3, first[1::2]] = -0.0
    return u0, phi


def nonfinite_inputs(N, G):
    u0, phi = inputs(N, G)
    u0 = u0.copy()
    u0[NAN_ENV, N // 3] = np.nan
    u0[INF_ENV, (2 * N) // 3] = np.inf
    return u0, phi


def run_all(kspde):
    """{(N, variant, objective, n, case): (state, obs, acc, status)} with whatever library kspde has loaded."""
    out = {}
    for N, G in LAYOUTS:
        s = kspde.KSStepper(E, N, L_PER_POINT * N, DT, mode="fast")
        for case, (u0, phi) in (("finite", inputs(N, G)), ("nonfinite", nonfinite_inputs(N, G))):
            for variant in variants(N, G):
                s.set_variant(variant)
                assert s.layout()["variant"] == variant, s.layout()
                for obj in (OBJECTIVES[:1] if variant in HYBRID else OBJECTIVES):
                    s.set_objective(obj)
                    for n in SUBSTEPS:
                        s.set_state(u0)
                        obs, acc, st = s.step(phi, n)
                        out[N, variant, obj, n, case] = (s.get_state(), obs, acc, st)
        s.close()
    return out


def _key(k):
    return "|".join(str(x) for x in k)


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


if __name__ == "__main__":
    for p in (ROOT, PKG):
        sys.path.insert(0, p)
    import kspde as _kspde
    _kspde.load()
    res = run_all(_kspde)
    np.savez(sys.argv[1], **{f"{_key(k)}|{f}": a for k, v in res.items() for f, a in zip(FIELDS, v)})
    print(f"{len(res)} runs with {os.environ.get('KSPDE_LIB')}")
    sys.exit(0)


import pytest  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shed():
    import kspde
    lib = os.environ.get("KSPDE_LIB")
    assert not lib or os.path.basename(lib) == "libkspde.so", f"this process must step with libkspde.so, not {lib}"
    kspde.load()
    return run_all(kspde)


@pytest.fixture(scope="module")
def loop0(tmp_path_factory):
    lib = os.path.join(PKG, "lib", "libkspde_loop0.so")
    assert os.path.exists(lib), f"{lib} is not built (make -C csrc)"
    out = str(tmp_path_factory.mktemp("loop0") / "out.npz")
    env = dict(os.environ, KSPDE_LIB=lib)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, timeout=CHILD_TIMEOUT,
                       capture_output=True, text=True)
    assert r.returncode == 0, f"child exited with {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return np.load(out)


def _runs(N, G, case):
    return [(N, v, o, n, case) for v in variants(N, G) for o in (OBJECTIVES[:1] if v in HYBRID else OBJECTIVES)
            for n in SUBSTEPS]


def test_layouts_covered():
    """Every points-per-lane count with a tile of more than one point, and tiles of 2, 3 and 4 points."""
    tiled = [(N, G) for N, G in LAYOUTS if tile(N // G) > 1]
    assert sorted({N // G for N, G in tiled}) == [2, 3, 4, 6, 8, 12, 16]
    assert {tile(N // G) for N, G in tiled} == {2, 3, 4}
    for N, G in tiled:
        u0, _ = inputs(N, G)
        first = np.arange(0, N, tile(N // G))
        assert (u0[0] > 0).all() and (u0[1] < 0).all() and (u0[3, first] == 0).all()
        assert np.signbit(u0[3, first]).any() and not np.signbit(u0[3, first]).all()
        assert (u0[4, first] < 0).any() and (u0[4, first] > 0).any()


@pytest.mark.parametrize("N,G", LAYOUTS)
def test_bit_equal_to_loop0(shed, loop0, N, G):
    for k in _runs(N, G, "finite"):
        for f, a in zip(FIELDS, shed[k]):
            np.testing.assert_array_equal(_raw(a), _raw(loop0[f"{_key(k)}|{f}"]), err_msg=f"{k} {f}")
        state, obs, _, st = shed[k]
        assert not st.any() and np.isfinite(state).all(), k
        np.testing.assert_array_equal(obs, state.astype(np.float32), err_msg=str(k))


@pytest.mark.parametrize("N,G", LAYOUTS)
def test_nonfinite_envs(shed, loop0, N, G):
    rest = [e for e in range(E) if e not in (NAN_ENV, INF_ENV)]
    for k in _runs(N, G, "nonfinite"):
        for f, a in zip(FIELDS, shed[k]):
            np.testing.assert_array_equal(_raw(a), _raw(loop0[f"{_key(k)}|{f}"]), err_msg=f"{k} {f}")
        st = shed[k][3]
        assert st[NAN_ENV] and st[INF_ENV] and not st[rest].any(), (k, st)
        clean = shed[k[:4] + ("finite",)]
        for f, a, b in zip(FIELDS, shed[k], clean):
            np.testing.assert_array_equal(_raw(a[rest]), _raw(b[rest]), err_msg=f"{k} {f}: a finite env changed")
