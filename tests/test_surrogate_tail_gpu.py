"""The tail of the surrogate's training step on an MI355X, each kernel at its own entry point against the fp64 oracles of
tests/_sur_tail_oracle.py: the gradient reduction (flush_grads_kernel, flush_all_kernel), the row fold (fold_rows_kernel),
Adam in its three spellings (adam_all_kernel, the Adam branch of either flush kernel) and the delta loss
(delta_loss_kernel, delta_loss_finalize_kernel) in its three call forms.

The packs are synthetic (any size list, guard sentinels between the tensors and around every buffer), so the code's own
boundaries -- 32 columns per block, 32 row groups x 8 loads per round, 256 elements per Adam block, the block-to-pack split
of the three-pack kernels, nsplit <= 8, TPB partials per finishing round -- are placed on purpose.  Bounds:
  reduction / fold   (ceil(rows / 32) + 32) u sum |partial[r][t]| per element: the depth of the two summation chains
  Adam               UNIT_BOUND units of tests/_sac_models.adam_units against adam_replay(fp32_hyper=True), per update;
                     p' also within P_BOUND units (below), which bias corrections that cancel do not meet
  delta loss         deltas / dd_all bit-equal to the fp32 numpy spelling; loss, hsteploss, means and stds within one fp32
                     rounding (relative 2^-24) of the fp64 oracle; the three call forms bit-identical
Worst observed figures are appended to sur_tail_parity_observed.jsonl next to conftest's gradient parity log
(tools/sur_tail_parity_report.py collects them into profiles/sur_tail_parity_observed.json)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _sur_tail_oracle as so
from _sac_models import HYPERS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
HYPER = [dict(lr=h["lr"], beta1=h["betas"][0], beta2=h["betas"][1], eps=h["eps"]) for h in HYPERS.values()]
KINDS = ("enc", "enc", "chunk")
#: layouts of the packs (e0, e1, c2) of one three-pack call: three different block counts each
TRIPLES = [("odd", "even", "tiny"), ("tiny", "wide", "odd"), ("even", "odd", "wide"), ("wide", "tiny", "even"), ("odd", "wide", "tiny")]


def _lib():
    from pdecontrol.surrogates import hipops
    return hipops.load()


def _stream():
    import hipbind
    return hipbind.stream()


def _ok(rc):
    assert rc == 0, (rc, _lib().sur_last_error().decode())


def _host(t):
    return t.detach().cpu().numpy().copy()


def _packs(names, rows, surplus=3):
    return [so.synthetic_pack(kind, so.layout(name, kind), r, r + surplus, DEV) for kind, name, r in zip(KINDS, names, rows)]


def _flush_single(pack, adam, overwrite):
    fn = _lib().sur_flush_encoder_grads if pack.kind == "enc" else _lib().sur_flush_chunk_grads
    _ok(fn(_stream(), pack.ref(), adam, overwrite))


def _flush_all(packs, adams, mask):
    _ok(_lib().sur_flush_all_grads(_stream(), packs[0].ref(), adams[0], packs[1].ref(), adams[1], packs[2].ref(), adams[2], mask))


# ----------------------------------------------------------------------------------------------------------------------
# reduction
# ----------------------------------------------------------------------------------------------------------------------
def _fill_for_flush(packs, mask, seed):
    """Random partial rows [0, rows), random weights; g random where pack j accumulates, NaN where bit j of mask is set."""
    rs = np.random.RandomState(seed)
    for j, p in enumerate(packs):
        p.partial[:p.rows] = torch.from_numpy(so.mixed_rows(rs, p.rows, p.psize)).to(DEV)
        p.put(p.wflat, rs.standard_normal(p.psize))
        p.put(p.gflat, np.full(p.psize, np.nan) if mask >> j & 1 else so.mixed_rows(rs, 1, p.psize)[0])


@pytest.mark.parametrize("mask", [0, 1, 2, 4, 5])
@pytest.mark.parametrize("k", range(len(so.ROWS)), ids=[f"rows{r}" for r in so.ROWS])
def test_reduction_against_fp64_and_one_launch_against_three(k, mask):
    """sur_flush_all_grads on three packs of different layouts and row counts (pack j reduces ROWS[k + j]), bit j of the
    mask chooses g = sum (from NaN) or g += sum; then the three single-pack launches from the same inputs."""
    names = TRIPLES[[0, 1, 2, 4, 5].index(mask)]
    rows = [so.ROWS[(k + j) % len(so.ROWS)] for j in range(3)]
    one, three = _packs(names, rows), _packs(names, rows)
    for packs in (one, three):
        _fill_for_flush(packs, mask, 1000 * k + mask)
    before = [(_host(p.partial), _host(p.get(p.gflat)), so.bits(p.wflat)) for p in one]
    _flush_all(one, [None] * 3, mask)
    for j, p in enumerate(three):
        _flush_single(p, None, mask >> j & 1)
    torch.cuda.synchronize(DEV)
    worst = 0.0
    for j, (p, q, (partial, g_old, w_bits)) in enumerate(zip(one, three, before)):
        overwrite = bool(mask >> j & 1)
        s, a = so.reduce_rows(partial, p.rows)
        want = s if overwrite else s + g_old.astype(np.float64)
        bound = so.depth_bound(p.rows, a) + (0.0 if overwrite else so.U * np.abs(g_old))
        got = _host(p.get(p.gflat))
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= bound), (j, names[j], p.rows, float(np.nanmax(err / bound)))
        worst = max(worst, float(np.max(err / bound)))
        assert not so.bits(p.partial[:p.rows]).any(), "every reduced row is exactly zero afterwards"
        assert p.gaps_intact() and np.array_equal(so.bits(p.wflat), w_bits), "surplus rows, guard gaps and w are untouched"
        assert np.array_equal(so.bits(q.gflat), so.bits(p.gflat)) and np.array_equal(so.bits(q.partial_flat), so.bits(p.partial_flat)) \
            and np.array_equal(so.bits(q.wflat), w_bits), "one launch = three launches, bit for bit"
    so.record(case=f"reduction-rows{rows}-mask{mask}", layouts=names, worst_err_over_bound=worst)


# ----------------------------------------------------------------------------------------------------------------------
# fold
# ----------------------------------------------------------------------------------------------------------------------
#: count -> (rows, base, dst)
FOLD_CASES = {"dst below the range": lambda n: (n + 8, 5, 3), "dst above the range": lambda n: (n + 6, 1, n + 3),
              "dst = 0": lambda n: (n + 2, 1, 0), "dst = rows - 1": lambda n: (n + 3, 0, n + 2)}
COUNTS = (1, 33, 257)


@pytest.mark.parametrize("variant", range(4))
@pytest.mark.parametrize("c", range(3), ids=[f"count{n}" for n in COUNTS])
def test_fold_rows_against_fp64(c, variant):
    """One sur_fold_rows launch folds a different (base, count, dst) case in each of the three packs; every row holds
    random content before, the destination row included."""
    names = TRIPLES[variant]
    counts = [COUNTS[(c + j) % 3] for j in range(3)]
    cases = [list(FOLD_CASES)[(variant + j) % 4] for j in range(3)]
    geo = [FOLD_CASES[name](n) for name, n in zip(cases, counts)]
    packs = _packs(names, [g[0] for g in geo])
    rs = np.random.RandomState(77 + 10 * c + variant)
    for p in packs:
        p.partial[:p.rows] = torch.from_numpy(so.mixed_rows(rs, p.rows, p.psize)).to(DEV)
        p.put(p.wflat, rs.standard_normal(p.psize))
    before = [(_host(p.partial), so.bits(p.wflat), so.bits(p.gflat)) for p in packs]
    arr = lambda i: (ctypes.c_int * 3)(*[g[i] for g in geo])
    bases, dsts = arr(1), arr(2)
    _ok(_lib().sur_fold_rows(_stream(), packs[0].ref(), packs[1].ref(), packs[2].ref(), bases, (ctypes.c_int * 3)(*counts), dsts))
    torch.cuda.synchronize(DEV)
    worst = 0.0
    for p, (rows, base, dst), n, (partial, w_bits, g_bits) in zip(packs, geo, counts, before):
        want, mag = so.fold_rows(partial[:rows], base, n, dst)
        got = _host(p.partial)
        bound = so.depth_bound(n, mag)
        err = np.abs(got[dst].astype(np.float64) - want[dst])
        assert np.all(err <= bound), (base, n, dst, float(np.max(err / bound)))
        worst = max(worst, float(np.max(err / bound)))
        assert not so.bits(got[base:base + n]).any(), "the folded rows are exactly zero"
        others = [r for r in range(p.alloc_rows) if r != dst and not base <= r < base + n]
        assert np.array_equal(so.bits(got[others]), so.bits(partial[others])), "every other row is untouched"
        assert p.gaps_intact() and np.array_equal(so.bits(p.wflat), w_bits) and np.array_equal(so.bits(p.gflat), g_bits)
    # a flush after the fold: the sum of all original rows.  Two reductions in a row: the fold's chains over `count` rows,
    # then the flush's over `rows`, each bounded on the magnitudes of all original rows.
    _flush_all(packs, [None] * 3, 7)
    torch.cuda.synchronize(DEV)
    for p, (rows, base, dst), n, (partial, _, _) in zip(packs, geo, counts, before):
        s, a = so.reduce_rows(partial, rows)
        bound = so.depth_bound(n, a) + so.depth_bound(rows, a)
        err = np.abs(_host(p.get(p.gflat)).astype(np.float64) - s)
        assert np.all(err <= bound), (base, n, dst, float(np.nanmax(err / bound)))
        worst = max(worst, float(np.max(err / bound)))
        assert not so.bits(p.partial[:rows]).any() and p.gaps_intact()
    so.record(case=f"fold-counts{counts}-variant{variant}", cases=cases, layouts=names, worst_err_over_bound=worst)


# ----------------------------------------------------------------------------------------------------------------------
# Adam, update by update
# ----------------------------------------------------------------------------------------------------------------------
FLUSH_ROWS = 33                      # more rows than row groups
SPREAD = {0: 0.5, 5: 0.25, 32: 0.25}  # the partial rows that carry a gradient in the flush spellings (the rest are zero)
LATE = (100, 1000, 10000)
#: p' = p - step with step = (lr / bc1) (m' / (sqrt(v') / sqrt(bc2) + eps)): 7 fp32 roundings on the step (u |step| each),
#: m' and v' carried in with 3 and 4 roundings (3 u and, under the root, 2 u where m' does not cancel -- the inputs see to
#: that next to small parameters), bc1 and sqrt(bc2) from expm1f / logf with 5 u and 2.5 u, one rounding u (|p| + |step|) on
#: the result: u |p| + 20.5 u |step| <= 1.3 units of u |p| + 16 u |step|.  Bias corrections 1.0f - powf(beta, t) alone put
#: 57 u |step| = 3.6 units on top at t = 2 ... 4 (tests/test_surrogate_tail_host.py).
P_BOUND = 2.0
_late_cache = {}


def _late_moments(j):
    """{t - 1: (m, v)} for t in LATE: the moments of pack j's hyper-parameters after t - 1 updates of an fp64 run on 300
    elements of so.gradient_classes (sign per element fixed next to a small parameter), rounded to fp32."""
    if j not in _late_cache:
        rs = np.random.RandomState(500 + j)
        n, h = 300, HYPER[j]
        b1, b2 = float(np.float32(h["beta1"])), float(np.float32(h["beta2"]))
        fixed, small = rs.choice([-1.0, 1.0], n), so.small_parameter(n)
        m, v, out = np.zeros(n), np.zeros(n), {}
        for t in range(1, LATE[-1]):
            g = so.gradient_classes(rs, n, np.where(small, fixed, rs.choice([-1.0, 1.0], n))).astype(np.float64)
            m = m + (g - m) * (1.0 - b1)
            v = b2 * v + (1.0 - b2) * g * g
            if t + 1 in LATE:
                out[t] = (m.astype(np.float32), v.astype(np.float32), fixed)
        _late_cache[j] = out
    return _late_cache[j]


def _launch_adam(spelling, packs, states, live=(True, True, True)):
    ads = [s.ref() if on else None for s, on in zip(states, live)]
    if spelling == "apply":
        _ok(_lib().sur_adam_apply(_stream(), packs[0].ref(), ads[0], packs[1].ref(), ads[1], packs[2].ref(), ads[2]))
    elif spelling == "flush_all":
        _flush_all(packs, ads, 0)
    else:
        for p, a in zip(packs, ads):
            _flush_single(p, a, 0)


def _set_gradient(spelling, p, g):
    """The gradient tensors themselves (sur_adam_apply), or partial rows that sum to about g; g is then NaN beforehand."""
    if spelling == "apply":
        p.put(p.gflat, g)
        return
    p.put(p.gflat, np.full(p.psize, np.nan))
    p.partial[:p.rows] = 0.0
    for r, share in SPREAD.items():
        p.partial[r] = torch.from_numpy((np.float32(share) * g).astype(np.float32)).to(DEV)


def _judge_update(spelling, t, j, p, st, lr, inputs, bad):
    """One pack after one launch against adam_replay from the same inputs; returns the units."""
    w0, m0, v0, g_in = inputs
    g = _host(p.get(p.gflat))                       # the fp32 gradient the launch consumed (flush: the one it wrote)
    if spelling == "apply":
        assert np.array_equal(so.bits(g), so.bits(g_in)), "sur_adam_apply leaves the gradients alone"
    else:
        assert np.all(np.abs(g.astype(np.float64) - g_in) <= so.depth_bound(p.rows, np.abs(g_in.astype(np.float64)))), "reduced gradient"
        assert not so.bits(p.partial[:p.rows]).any()
    h = st.hyper
    w1, m1, v1 = _host(p.get(p.wflat)), _host(st.m), _host(st.v)
    assert not (np.isnan(w1).any() or np.isnan(m1).any() or np.isnan(v1).any() or np.isnan(g).any())
    ref = so.adam_replay(w0, m0, v0, g, t, lr, h["beta1"], h["beta2"], h["eps"], fp32_hyper=True)
    units = so.adam_units(w0, m0, v0, g, w1, m1, v1, ref)
    still = (g == 0) & (m0 == 0) & (v0 == 0)
    assert still.any() and np.array_equal(so.bits(w1[still]), so.bits(w0[still])), "g = 0 on zero moments keeps the parameter's bits"
    assert int(st.step) == t and int(st.ticket) == 0, (int(st.step), int(st.ticket))
    assert p.gaps_intact() and st.gaps_intact()
    so.record(case=f"adam-{spelling}", t=t, pack=j, layout_psize=p.psize, **units, bound=so.UNIT_BOUND, p_bound=P_BOUND)
    if max(units.values()) > so.UNIT_BOUND or units["p"] > P_BOUND:
        bad.append((t, j, units))
    return units


@pytest.mark.parametrize("spelling", ["apply", "flush_single", "flush_all"])
def test_adam_update_by_update_against_fp64(spelling):
    """Updates t = 1 ... 12 in sequence on three packs with distinct hyper-parameters, then one update each at step counts
    100, 1000 and 10000 from preset counters and moments.  Each update is judged from its own inputs (the kernel's previous
    moments; parameters re-drawn, so that every update sees parameters of order 0.1, of order 1e-7 and exact zeros); the
    device learning rate is halved before update 7 without touching the descriptor."""
    names = {"apply": ("wide", "odd", "tiny"), "flush_single": ("odd", "wide", "even"), "flush_all": ("tiny", "even", "wide")}[spelling]
    packs = _packs(names, [FLUSH_ROWS] * 3)
    states = [so.AdamState(p, device=DEV, **h) for p, h in zip(packs, HYPER)]
    rs = np.random.RandomState({"apply": 1, "flush_single": 2, "flush_all": 3}[spelling])
    fixed = [rs.choice([-1.0, 1.0], p.psize) for p in packs]
    lrs = [float(np.float32(h["lr"])) for h in HYPER]
    bad = []

    def update(t):
        inputs = []
        for p, st, sign in zip(packs, states, fixed):
            n = p.psize
            w0 = so.parameter_classes(rs, n)
            # next to a small parameter the gradient keeps its sign from update to update: m' does not cancel, so its own
            # roundings stay small against the step that p' is judged by there
            g = so.gradient_classes(rs, n, np.where(so.small_parameter(n), sign, rs.choice([-1.0, 1.0], n)))
            p.put(p.wflat, w0)
            _set_gradient(spelling, p, g)
            inputs.append((w0, _host(st.m), _host(st.v), g))
        _launch_adam(spelling, packs, states)
        torch.cuda.synchronize(DEV)
        for j, (p, st) in enumerate(zip(packs, states)):
            _judge_update(spelling, t, j, p, st, lrs[j], inputs[j], bad)

    for t in range(1, 13):
        if t == 7:
            for j, st in enumerate(states):
                lrs[j] = float(np.float32(lrs[j]) * np.float32(0.5))
                st.lr.fill_(lrs[j])
        update(t)
    for t in LATE:
        for j, (p, st) in enumerate(zip(packs, states)):
            m, v, sign = _late_moments(j)[t - 1]
            st.m.copy_(torch.from_numpy(m[:p.psize]))
            st.v.copy_(torch.from_numpy(v[:p.psize]))
            st.step.fill_(t - 1)
            fixed[j] = sign[:p.psize]
        update(t)
    assert not bad, f"{spelling}: over UNIT_BOUND = {so.UNIT_BOUND} (p': P_BOUND = {P_BOUND}) at (t, pack, units): {bad}"


def test_adam_apply_skips_a_pack_without_a_descriptor():
    packs = _packs(("odd", "wide", "tiny"), [4] * 3)
    states = [so.AdamState(p, device=DEV, **h) for p, h in zip(packs, HYPER)]
    rs = np.random.RandomState(9)
    for live in [(True, False, True), (False, True, False), (True, True, False)]:
        for p, st in zip(packs, states):
            p.put(p.wflat, so.parameter_classes(rs, p.psize))
            p.put(p.gflat, so.gradient_classes(rs, p.psize))
        before = [(so.bits(p.wflat), so.bits(p.gflat), so.bits(st.mflat), so.bits(st.vflat), _host(st.iflat)) for p, st in zip(packs, states)]
        _launch_adam("apply", packs, states, live)
        torch.cuda.synchronize(DEV)
        for on, p, st, (w, g, m, v, ints) in zip(live, packs, states, before):
            assert np.array_equal(so.bits(p.gflat), g) and int(st.ticket) == 0 and p.gaps_intact() and st.gaps_intact()
            if on:
                assert int(st.step) == ints[so.GAP] + 1 and not np.array_equal(so.bits(p.wflat), w)
            else:
                assert np.array_equal(so.bits(p.wflat), w) and np.array_equal(so.bits(st.mflat), m) \
                    and np.array_equal(so.bits(st.vflat), v) and np.array_equal(_host(st.iflat), ints), "a skipped pack is untouched"
    # a skipped pack needs no parameter struct either
    _ok(_lib().sur_adam_apply(_stream(), packs[0].ref(), states[0].ref(), None, None, None, None))
    torch.cuda.synchronize(DEV)
    assert int(states[0].step) == 3 and int(states[1].step) == 2 and int(states[2].step) == 1


def test_adam_apply_and_flush_agree_bit_for_bit_from_equal_inputs():
    """sur_adam_apply and the flush from the same parameters, moments and (the flush's own) gradient, three updates.  Both
    launches run the one adam_update of csrc/sur_tail.h, so p', m' and v' agree bit for bit on every update; the outcome
    (and, should they ever part, the largest difference in units) is recorded as well."""
    names = ("wide", "odd", "tiny")
    a, b = _packs(names, [FLUSH_ROWS] * 3), _packs(names, [FLUSH_ROWS] * 3)
    sa = [so.AdamState(p, device=DEV, **h) for p, h in zip(a, HYPER)]
    sb = [so.AdamState(p, device=DEV, **h) for p, h in zip(b, HYPER)]
    rs = np.random.RandomState(21)
    equal, apart, parted = True, 0.0, []
    for t in (1, 2, 3):
        for p, q, s, r in zip(a, b, sa, sb):
            w0, g = so.parameter_classes(rs, p.psize), so.gradient_classes(rs, p.psize)
            p.put(p.wflat, w0)
            q.put(q.wflat, w0)
            r.m.copy_(s.m)
            r.v.copy_(s.v)
            _set_gradient("flush_all", p, g)
        _launch_adam("flush_all", a, sa)
        for p, q in zip(a, b):
            q.put(q.gflat, p.get(p.gflat))
        _launch_adam("apply", b, sb)
        torch.cuda.synchronize(DEV)
        for p, q, s, r in zip(a, b, sa, sb):
            assert int(s.step) == int(r.step) == t
            pairs = [(_host(p.get(p.wflat)), _host(q.get(q.wflat))), (_host(s.m), _host(r.m)), (_host(s.v), _host(r.v))]
            for (x, y), what in zip(pairs, ("p'", "m'", "v'")):
                assert not (np.isnan(x).any() or np.isnan(y).any())
                same = np.array_equal(so.bits(x), so.bits(y))
                equal = equal and same
                parted.extend([] if same else [(t, what, p.psize)])
                scale = np.maximum(np.abs(x), np.abs(y)).astype(np.float64)
                diff = np.abs(x.astype(np.float64) - y)
                apart = max(apart, float(np.max(np.where(scale > 0, diff / np.where(scale > 0, scale * so.U, 1.0), 0.0))))
    so.record(case="adam-apply-vs-flush-equal-inputs", bit_equal=bool(equal), worst_difference_in_u_of_the_value=apart)
    assert equal and not parted, (parted, apart)


# ----------------------------------------------------------------------------------------------------------------------
# delta loss
# ----------------------------------------------------------------------------------------------------------------------
LOSS_CASES = [(1, 2, 64),        # minimum T, per_t < TPB
              (10, 5, 100),      # tail inside the unroll, nsplit 1
              (5, 7, 205),       # per_t = 1025: nsplit 2
              (32, 4, 256),      # nsplit 8 exactly
              (33, 40, 256),     # capped, a second round per thread, nq = 312 > TPB
              (1, 258, 64)]      # T - 1 > TPB
DELTA = 0.25


class _LossOut:
    """The outputs of one loss, each between guard sentinels."""

    def __init__(self, B, T, N):
        self.flat, self.view = {}, {}
        for name, n in (("deltas", B * (T - 1) * N), ("dd_all", T * B * N), ("hstep", T - 1), ("loss", 1), ("stats", 4)):
            self.flat[name], self.view[name] = so.guarded(n, DEV)

    def host(self):
        return {k: _host(v) for k, v in self.view.items()}

    def gaps_intact(self):
        f = so.bits(np.float32(so.SENTINEL).reshape(1))[0]
        return all(bool(np.all(so.bits(x[:so.GAP]) == f) and np.all(so.bits(x[-so.GAP:]) == f)) for x in self.flat.values())


def _device_view(view):
    """The strided fp32 view ``view`` of a host array, rebuilt on the device over a copy of its whole storage."""
    base = view
    while base.base is not None:
        base = base.base
    storage = torch.from_numpy(np.ascontiguousarray(base).reshape(-1)).to(DEV)
    offset = (view.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // 4
    assert base.flags["C_CONTIGUOUS"] and view.strides[2] == 4
    return storage, torch.as_strided(storage, view.shape, [s // 4 for s in view.strides], offset)


def _loss(form, states, d_all, B, T, N, mean, stdv, out, partial, ticket, rs, dd=True):
    lib = _lib()
    head = (ctypes.c_void_p(states.data_ptr()), states.stride(0), states.stride(1), ctypes.c_void_p(d_all.data_ptr()), B, T, N, DELTA,
            mean, stdv, *(ctypes.c_void_p(out.view[k].data_ptr()) if k != "dd_all" or dd else None
                          for k in ("deltas", "dd_all", "hstep", "loss", "stats")),
            ctypes.c_void_p(partial.data_ptr()), ctypes.c_void_p(ticket.data_ptr()))
    if form == "one":
        _ok(lib.sur_tbptt_delta_loss(_stream(), *head))
        return
    edges = np.linspace(0, T, min(T, 4) + 1).astype(int)                 # four uneven chunks that tile [0, T) (T = 2: its two rows)
    chunks = [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]
    if form == "ranges":
        for i in rs.permutation(len(chunks)):
            _ok(lib.sur_tbptt_delta_loss_range(_stream(), *head, *chunks[i]))
        return
    for c in chunks[:-1]:
        _ok(lib.sur_tbptt_delta_loss_range(_stream(), *head, *c))
    _ok(lib.sur_tbptt_delta_loss_rows(_stream(), *head, *chunks[-1]))
    _ok(lib.sur_tbptt_delta_loss_finalize(_stream(), B, T, N, *head[12:15], *head[15:17]))


@pytest.mark.parametrize("mean,stdv", [(0.0, 1.0), (0.01, math.sqrt(0.5))], ids=["identity", "scaled"])
@pytest.mark.parametrize("storage", ["batch", "time", "padded"])
@pytest.mark.parametrize("B,T,N", LOSS_CASES)
def test_delta_loss_against_fp64_in_all_call_forms(B, T, N, storage, mean, stdv):
    rs = np.random.RandomState(B + T + N)
    s_np, d_np = so.loss_inputs(B, T, N, 40, storage)
    ref = so.delta_loss_oracle(s_np, d_np, DELTA, mean, stdv)
    alt = so.delta_loss_oracle(s_np, d_np, DELTA, mean, stdv, order=1)
    assert abs(ref["stats"][0]) <= ref["stats"][1] and abs(ref["stats"][2]) <= ref["stats"][3], "|mean| <= std for both populations"
    for key in ("loss", "hsteploss", "stats"):
        assert so.rel_err(np.asarray(alt[key]).astype(np.float32), ref[key]) <= so.U, f"the bound holds for another summation order: {key}"
    keep, states = _device_view(s_np)
    keep_bits = so.bits(keep)
    d_all = torch.from_numpy(d_np).to(DEV)
    pflat, partial = so.guarded(40 * T, DEV, dtype=torch.float64, fill=float("nan"))
    tflat, ticket = so.guarded(1, DEV, dtype=torch.int32, fill=0)
    got = {}
    for form in ("one", "ranges", "rows+finalize"):
        partial.fill_(float("nan"))
        out = _LossOut(B, T, N)
        _loss(form, states, d_all, B, T, N, mean, stdv, out, partial, ticket, rs)
        torch.cuda.synchronize(DEV)
        assert int(ticket) == 0 and out.gaps_intact(), form
        assert np.all(_host(tflat)[[0, 1, 2, -3, -2, -1]] == int(np.int32(float(so.SENTINEL)))), form
        assert np.all(_host(pflat)[:so.GAP] == float(so.SENTINEL)) and np.all(_host(pflat)[-so.GAP:] == float(so.SENTINEL)), form
        got[form] = out.host()
    assert np.array_equal(so.bits(keep), keep_bits) and np.array_equal(so.bits(d_all), so.bits(d_np)), "the inputs are read only"
    one = got["one"]
    for form in ("ranges", "rows+finalize"):
        for key, value in got[form].items():
            assert np.array_equal(so.bits(value), so.bits(one[key])), f"{form}: {key} differs from the single call"
    assert np.array_equal(so.bits(one["deltas"]), so.bits(ref["deltas"].reshape(-1))), "deltas: the fp32 spelling, bit for bit"
    assert np.array_equal(so.bits(one["dd_all"]), so.bits(ref["dd_all"].reshape(-1))), "dd_all: the fp32 spelling, bit for bit"
    assert not so.bits(one["dd_all"].reshape(T, -1)[T - 1]).any(), "row T - 1 of dd_all is exactly zero"
    errs = dict(loss=so.rel_err(one["loss"], [ref["loss"]]), hsteploss=so.rel_err(one["hstep"], ref["hsteploss"]),
                means=so.rel_err(one["stats"][[0, 2]], ref["stats"][[0, 2]]), stds=so.rel_err(one["stats"][[1, 3]], ref["stats"][[1, 3]]))
    so.record(case=f"delta-loss-B{B}-T{T}-N{N}-{storage}-mean{mean}", **{k: v / so.U for k, v in errs.items()}, unit="2^-24 relative")
    for key, e in errs.items():
        assert e <= so.U, (key, e / so.U)
    # without dd_all: nothing is written where it would be, everything else is the same
    out = _LossOut(B, T, N)
    _loss("one", states, d_all, B, T, N, mean, stdv, out, partial, ticket, rs, dd=False)
    torch.cuda.synchronize(DEV)
    f = so.bits(np.float32(so.SENTINEL).reshape(1))[0]
    assert np.all(so.bits(out.flat["dd_all"]) == f) and out.gaps_intact() and int(ticket) == 0
    for key, value in out.host().items():
        assert key == "dd_all" or np.array_equal(so.bits(value), so.bits(one[key])), key
    # a second loss on other data through the same scratch (left as the first loss left it)
    s2_np, d2_np = so.loss_inputs(B, T, N, 41, storage)
    ref2 = so.delta_loss_oracle(s2_np, d2_np, DELTA, mean, stdv)
    _, states2 = _device_view(s2_np)
    out2 = _LossOut(B, T, N)
    _loss("one", states2, torch.from_numpy(d2_np).to(DEV), B, T, N, mean, stdv, out2, partial, ticket, rs)
    torch.cuda.synchronize(DEV)
    two = out2.host()
    assert int(ticket) == 0 and np.array_equal(so.bits(two["deltas"]), so.bits(ref2["deltas"].reshape(-1)))
    assert so.rel_err(two["loss"], [ref2["loss"]]) <= so.U and so.rel_err(two["hstep"], ref2["hsteploss"]) <= so.U
    assert so.rel_err(two["stats"], ref2["stats"]) <= so.U
