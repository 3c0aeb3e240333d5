"""``fno_forward_select`` (csrc/fno.hip, include/spectral/forward_select.h) on the GPU: every row is, byte for byte, the
row of ``fno_forward`` with the picked member's weights, scale and shift; a step outside the slots writes nothing; a member
index outside the ensemble poisons its row alone; a second launch gives the same bytes.  The per-member ``fno_forward``
outputs of a case are computed once and shared by its tests."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

T_SLOTS, T_NOW = 3, 1
CASES = [(64, nb, members) for nb in (1, 5, 257) for members in (1, 3, 8)] + [(512, 2, 3)]
_cache = {}


def _case(n, nb, members):
    """Inputs of one case on the device and the members' ``fno_forward`` outputs [members, nb, n] (numpy)."""
    key = (n, nb, members)
    if key in _cache:
        return _cache[key]
    from pdecontrol.architectures.fno import FNO1d
    from pdecontrol.surrogates import fno_hip
    dev = torch.device("cuda", 0)
    lib = fno_hip.load()
    rs = np.random.RandomState(1000 * n + 10 * nb + members)
    x = np.linspace(0, 2 * np.pi, n, endpoint=False)
    rows = lambda: np.stack([sum(rs.uniform(-1, 1) * np.sin((k + 1) * x + rs.uniform(0, 6)) for k in range(4))
                             for _ in range(nb)]).astype(np.float32)
    u, act = torch.from_numpy(rows()).to(dev), torch.from_numpy(rows()).to(dev)
    structs, keep = [], []
    for m in range(members):
        torch.manual_seed(100 + m)
        w, ps = fno_hip._weights_struct(fno_hip.parameters_of(FNO1d().to(dev)))
        structs.append(w)
        keep.append(ps)
    cscale = np.asarray([0.05 * (1.0 + 0.37 * m) for m in range(members)], dtype=np.float32)
    cshift = np.asarray([0.01 * m - 0.02 for m in range(members)], dtype=np.float32)
    chosen = rs.randint(0, members, (T_SLOTS, nb)).astype(np.int32)
    chosen[T_NOW, 0] = 0                                       # member 0 and the last member are hit at least once
    chosen[T_NOW, nb - 1] = members - 1 if nb > 1 else chosen[T_NOW, 0]
    ref = np.empty((members, nb, n), dtype=np.float32)
    st = fno_hip._stream()
    for m in range(members):
        delta, out = torch.empty((nb, n), device=dev), torch.empty((nb, n), device=dev)
        fno_hip._check(lib.fno_forward(st, ctypes.byref(structs[m]), 32, 16, 4, n, nb, nb, fno_hip._ptr(u), 0, n, fno_hip._ptr(act),
                                       0, n, float(cscale[m]), float(cshift[m]), fno_hip._ptr(delta), fno_hip._ptr(out), None,
                                       None, 0, 0))
        ref[m] = out.cpu().numpy()
    assert np.isfinite(ref).all()
    if members > 1:     # the members differ: picking the wrong one cannot pass
        assert all(not np.array_equal(ref[0], ref[m]) for m in range(1, members))
    case = dict(n=n, nb=nb, members=members, u=u, act=act, structs=structs, keep=keep, cscale=cscale, cshift=cshift,
                chosen=chosen, ref=ref, dev=dev)
    _cache[key] = case
    return case


def _select(case, chosen="case", step=(T_NOW, 9), out=None, members=None):
    """One launch; returns (out [nb, n] numpy, step after the call, the device output tensor)."""
    from pdecontrol.surrogates import fno_hip
    dev, n, nb = case["dev"], case["n"], case["nb"]
    members = case["members"] if members is None else members
    ws = (fno_hip.FnoWeights * members)(*case["structs"][:members])
    cs = (ctypes.c_float * members)(*case["cscale"][:members].tolist())
    ch = (ctypes.c_float * members)(*case["cshift"][:members].tolist())
    chosen = case["chosen"] if isinstance(chosen, str) else chosen
    chosen_d = None if chosen is None else torch.from_numpy(np.ascontiguousarray(chosen, dtype=np.int32)).to(dev)
    step_d = None if step is None else torch.tensor(list(step), dtype=torch.int32, device=dev)
    out = torch.full((nb, n), 7.0, device=dev) if out is None else out
    a = fno_hip.FnoSelectArgs(ws, cs, ch, members, None if chosen_d is None else chosen_d.data_ptr(),
                              None if step_d is None else step_d.data_ptr(), T_SLOTS, case["u"].data_ptr(), case["act"].data_ptr(),
                              out.data_ptr())
    fno_hip.forward_select(fno_hip._stream(), n, nb, a)
    torch.cuda.synchronize()
    return out.cpu().numpy(), None if step_d is None else step_d.tolist(), out


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("n,nb,members", CASES, ids=[f"n{n}_b{nb}_m{m}" for n, nb, m in CASES])
def test_rows_are_the_picked_members_fno_forward_rows(n, nb, members):
    """n = 512 takes 156 KB of dynamic LDS: the new kernel symbol carries its own attribute."""
    case = _case(n, nb, members)
    got, step, _ = _select(case)
    want = case["ref"][case["chosen"][T_NOW], np.arange(nb)]
    np.testing.assert_array_equal(_bytes(got), _bytes(want))
    assert step == [T_NOW, 9], "the counter is read, never written"
    # a second launch from the same inputs gives the same bytes
    again, _, _ = _select(case)
    np.testing.assert_array_equal(_bytes(again), _bytes(got))
    if members == 1:                                # one member needs no chosen array; without a counter the slot is 0
        alone, _, _ = _select(case, chosen=None)
        np.testing.assert_array_equal(_bytes(alone), _bytes(case["ref"][0]))
        slot0, step0, _ = _select(case, step=None)
        np.testing.assert_array_equal(_bytes(slot0), _bytes(case["ref"][0]))
    else:
        slot0, _, _ = _select(case, step=None)
        np.testing.assert_array_equal(_bytes(slot0), _bytes(case["ref"][case["chosen"][0], np.arange(nb)]))


@pytest.mark.gpu
@pytest.mark.parametrize("t", [-1, T_SLOTS])
def test_a_step_outside_the_slots_writes_nothing(t):
    case = _case(64, 5, 3)
    got, step, _ = _select(case, step=(t, 9))
    assert (got == 7.0).all(), "a workgroup wrote outside [0, T)"
    assert step == [t, 9]


@pytest.mark.gpu
def test_a_member_index_outside_the_ensemble_poisons_its_row_alone():
    case = _case(64, 5, 3)
    chosen = case["chosen"].copy()
    chosen[T_NOW] = [0, -1, 2, 3, 1]
    got, step, _ = _select(case, chosen=chosen)
    assert np.isnan(got[1]).all() and np.isnan(got[3]).all()
    for b in (0, 2, 4):
        np.testing.assert_array_equal(_bytes(got[b]), _bytes(case["ref"][chosen[T_NOW, b], b]))
    assert step == [T_NOW, 9]
    # with fewer members in the call, an index the larger ensemble knows is outside too
    got, _, _ = _select(case, chosen=np.full_like(chosen, 2), members=2)
    assert np.isnan(got).all()
