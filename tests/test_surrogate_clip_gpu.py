"""Gradient-norm clipping inside the surrogate step on an MI355X.

Kernels (``sur_flush_all_grads_sumsq``, ``sur_clip_adam_apply``; include/surrogate_hip.h) on the synthetic packs of
tests/_sur_tail_oracle.py, judged against the entry points they are built from:
  reduction     g bit-equal to ``sur_flush_all_grads`` (no Adam, overwrite mask 7); rows re-zeroed; guards intact; the sum
                of ``sumsq`` within 4 fp64 ulps of the fp64 sum of the squares of those g (every square is exact in fp64,
                only the adds round; both sums here are correctly rounded ``math.fsum``s, so the figure is the kernel's
                own adds: five deep per block), each block's own entry within 3 ulps (5 adds of half an ulp each)
  clip + Adam   ``total_norm`` within 1 fp32 ulp of the fp64 norm; g bit-equal to ``g_sum * coef`` with ``coef`` from the
                kernel's own ``total_norm`` by the header's formula in numpy fp32; w, m, v and the step counters bit-equal to
                ``sur_adam_apply`` on a copy of the packs that holds ``g_sum * coef``
then the captured step (``fused_step(batch, clip=c)``) against the eager fused closure with ``clip_grad_norm_``, and the
surrogate-update phase's two tiers against each other.  Observed figures go to clip_parity_observed.jsonl next to
conftest's gradient parity log (tools/clip_parity_report.py collects them into profiles/clip_parity_observed.json)."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import _sur_tail_oracle as so
import _surrogate_phase_scenario as sc
from _sac_models import HYPERS
from conftest import GRAD_LOG

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OBSERVED = os.path.join(os.path.dirname(GRAD_LOG), "clip_parity_observed.jsonl")
HYPER = [dict(lr=h["lr"], beta1=h["betas"][0], beta2=h["betas"][1], eps=h["eps"]) for h in HYPERS.values()]
KINDS = ("enc", "enc", "chunk")
TRIPLES = [("odd", "tiny", "wide"), ("even", "even", "odd"), ("tiny", "tiny", "tiny")]
ROWS = (1, 33, 257)


def record(**rec):
    """Append one observation to OBSERVED, stamped with the library build it was made on (as ``_sur_tail_oracle.record``)."""
    rec["lib"] = so.library_stamp()
    print("clip parity", json.dumps(rec))
    try:
        os.makedirs(os.path.dirname(OBSERVED), exist_ok=True)
        with open(OBSERVED, "a") as f:
            f.write(json.dumps(rec) + "\n")
    except OSError:
        pass


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


# ----------------------------------------------------------------------------------------------------------------------
# synthetic packs
# ----------------------------------------------------------------------------------------------------------------------
class Case:
    """Three packs with their Adam states and clip buffers, filled from ``seed``: two Cases of the same arguments hold the
    same bits.  ``scale`` multiplies pack j's rows; ``zero`` makes every row zero; ``inf_at`` = (pack, row, column) puts one
    +inf into the rows."""

    def __init__(self, names, rows, seed, scale=(1.0, 1.0, 1.0), zero=False, inf_at=None):
        self.packs = [so.synthetic_pack(kind, so.layout(name, kind), r, r + 3, DEV) for kind, name, r in zip(KINDS, names, rows)]
        self.adam = [so.AdamState(p, device=DEV, **HYPER[j]) for j, p in enumerate(self.packs)]
        self.seed, self.scale, self.zero, self.inf_at = seed, scale, zero, inf_at
        rs = np.random.RandomState(seed)
        for p in self.packs:
            p.put(p.wflat, so.parameter_classes(rs, p.psize))
        self.fill_rows(0)
        self.count = sum(so.flush_blocks(p.psize) for p in self.packs)
        self.sumsq_flat, self.sumsq = so.guarded(self.count, DEV, dtype=torch.float64, fill=-1.0)
        self.norm_flat, self.norm = so.guarded(1, DEV, fill=-1.0)

    def fill_rows(self, call):
        """The partial rows of call number ``call`` (and g = NaN: both launches overwrite it)."""
        rs = np.random.RandomState(7919 * self.seed + call + 1)
        for j, p in enumerate(self.packs):
            rows = so.mixed_rows(rs, p.rows, p.psize) * np.float32(self.scale[j])
            if self.zero:
                rows[:] = 0.0
            if self.inf_at is not None and self.inf_at[0] == j:
                rows[self.inf_at[1] % p.rows, self.inf_at[2] % p.psize] = np.inf
            p.partial[:p.rows] = torch.from_numpy(rows).to(DEV)
            p.put(p.gflat, np.full(p.psize, np.nan))

    def clip_params(self, max_norm):
        from pdecontrol.surrogates import hipops
        return hipops.ClipParams(self.sumsq.data_ptr(), self.count, max_norm, self.norm.data_ptr())

    def refs(self):
        return [p.ref() for p in self.packs]

    def adam_refs(self, live=(True, True, True)):
        return [a.ref() if on else None for a, on in zip(self.adam, live)]

    def reduce_sumsq(self):
        r = self.refs()
        _ok(_lib().sur_flush_all_grads_sumsq(_stream(), r[0], r[1], r[2], self.sumsq.data_ptr()))

    def clip_adam(self, max_norm, live=(True, True, True)):
        r, a, clip = self.refs(), self.adam_refs(live), self.clip_params(max_norm)
        _ok(_lib().sur_clip_adam_apply(_stream(), r[0], a[0], r[1], a[1], r[2], a[2], ctypes.byref(clip)))

    def reduce_plain(self, live=(False, False, False)):
        r, a = self.refs(), self.adam_refs(live)
        _ok(_lib().sur_flush_all_grads(_stream(), r[0], a[0], r[1], a[1], r[2], a[2], 0 if any(live) else 7))

    def adam_apply(self, live=(True, True, True)):
        r, a = self.refs(), self.adam_refs(live)
        _ok(_lib().sur_adam_apply(_stream(), r[0], a[0], r[1], a[1], r[2], a[2]))

    def grads(self):
        return [_host(p.get(p.gflat)) for p in self.packs]

    def guards_intact(self):
        d, f = float(so.SENTINEL), so.bits(np.float32(so.SENTINEL).reshape(1))[0]
        return (all(p.gaps_intact() for p in self.packs) and all(a.gaps_intact() for a in self.adam)
                and bool(torch.all(self.sumsq_flat[:so.GAP] == d)) and bool(torch.all(self.sumsq_flat[-so.GAP:] == d))
                and bool(np.all(so.bits(self.norm_flat[:so.GAP]) == f)) and bool(np.all(so.bits(self.norm_flat[-so.GAP:]) == f)))

    def state_bits(self):
        """Everything the launches may write: the bit patterns of g and w with their gaps and of the moments (int32 views
        of fp32), then [step, ticket] with their guards (int64, so that the two kinds cannot be confused)."""
        out = []
        for p, a in zip(self.packs, self.adam):
            out += [so.bits(p.gflat), so.bits(p.wflat), so.bits(a.mflat), so.bits(a.vflat), _host(a.iflat).astype(np.int64)]
        return out


def _same(a, b, nan_ok=False):
    """Bit-equal; with ``nan_ok`` a NaN equals a NaN of any payload (the host's and the device's default NaNs differ in sign)."""
    if not nan_ok:
        return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    f = lambda x: x.view(np.float32) if x.dtype == np.int32 else x
    return len(a) == len(b) and all(np.array_equal(f(x), f(y), equal_nan=True) for x, y in zip(a, b))


def _ulps64(got, want):
    return abs(got - want) / np.spacing(abs(want)) if want != 0.0 else (0.0 if got == 0.0 else math.inf)


def _coef(total, max_norm):
    """The header's formula in numpy fp32, one rounding per operation."""
    total = np.float32(total)
    with np.errstate(all="ignore"):
        coef = np.float32(max_norm) / (total + np.float32(1e-6))
    assert coef.dtype == np.float32
    return np.float32(1.0) if coef > np.float32(1.0) else coef


# ----------------------------------------------------------------------------------------------------------------------
# the reduction with per-block sums of squares
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(3), ids=[f"rows{r}" for r in ROWS])
@pytest.mark.parametrize("t", range(3), ids=["-".join(n) for n in TRIPLES])
def test_reduction_with_sums_of_squares(t, k):
    rows = [ROWS[(k + j) % 3] for j in range(3)]
    new, old = Case(TRIPLES[t], rows, 10 * t + k), Case(TRIPLES[t], rows, 10 * t + k)
    w_bits = [so.bits(p.wflat) for p in new.packs]
    new.reduce_sumsq()
    old.reduce_plain()
    torch.cuda.synchronize(DEV)
    for p, q, w in zip(new.packs, old.packs, w_bits):
        assert np.array_equal(so.bits(p.gflat), so.bits(q.gflat)), "g differs from sur_flush_all_grads"
        assert not so.bits(p.partial[:p.rows]).any(), "every reduced row is exactly zero afterwards"
        assert np.array_equal(so.bits(p.partial_flat), so.bits(q.partial_flat)) and np.array_equal(so.bits(p.wflat), w)
    assert new.guards_intact() and float(new.norm[0]) == -1.0
    sumsq, worst_block, k0 = _host(new.sumsq), 0.0, 0
    for g in new.grads():
        g64 = g.astype(np.float64)
        for b in range(so.flush_blocks(g.size)):
            want = math.fsum(g64[32 * b:32 * b + 32] ** 2)
            worst_block = max(worst_block, _ulps64(float(sumsq[k0]), want))
            k0 += 1
    assert k0 == new.count
    total = _ulps64(math.fsum(sumsq), math.fsum(np.concatenate(new.grads()).astype(np.float64) ** 2))
    record(case=f"sumsq-{'-'.join(TRIPLES[t])}-rows{rows}", total_ulps=total, worst_block_ulps=worst_block)
    assert worst_block <= 3.0 and total <= 4.0, (worst_block, total)


# ----------------------------------------------------------------------------------------------------------------------
# clip + Adam
# ----------------------------------------------------------------------------------------------------------------------
def _clipped_step_against_its_parts(names, rows, seed, max_norm, live=(True, True, True), calls=1, **fill):
    """``calls`` clipped steps on one Case against [sur_flush_all_grads, g * coef on the host, sur_adam_apply] on a second
    one.  Returns the Case, the norms the kernel reported and the coefficients."""
    got, ref = Case(names, rows, seed, **fill), Case(names, rows, seed, **fill)
    nan_ok = fill.get("inf_at") is not None
    norms, coefs = [], []
    for call in range(calls):
        if call:
            got.fill_rows(call)
            ref.fill_rows(call)
        got.reduce_sumsq()
        got.clip_adam(max_norm, live)
        ref.reduce_plain()
        torch.cuda.synchronize(DEV)
        g_sum = ref.grads()
        total = _host(got.norm)[0]
        assert total.dtype == np.float32
        sq = math.fsum(np.concatenate(g_sum).astype(np.float64) ** 2)
        if math.isfinite(sq):
            want = np.float32(math.sqrt(sq))
            assert abs(float(total) - math.sqrt(sq)) <= float(np.spacing(want)), (float(total), math.sqrt(sq))
        else:
            assert np.isinf(total) and total > 0
        coef = _coef(total, max_norm)
        with np.errstate(all="ignore"):
            for p, g in zip(ref.packs, g_sum):
                scaled = g * coef
                assert scaled.dtype == np.float32
                p.put(p.gflat, scaled)
        ref.adam_apply(live)
        torch.cuda.synchronize(DEV)
        assert _same(got.state_bits(), ref.state_bits(), nan_ok), f"call {call}: the clipped step is not its parts"
        for p in got.packs:
            assert not so.bits(p.partial[:p.rows]).any()
        assert got.guards_intact()
        for a, on in zip(got.adam, live):
            assert int(a.step[0]) == (call + 1 if on else 0) and int(a.ticket[0]) == 0
        norms.append(float(total))
        coefs.append(float(coef))
    return got, norms, coefs


@pytest.mark.parametrize("t", range(3), ids=["-".join(n) for n in TRIPLES])
def test_a_norm_above_the_bound_is_clipped(t):
    rows = [ROWS[(t + j) % 3] for j in range(3)]
    _, norms, coefs = _clipped_step_against_its_parts(TRIPLES[t], rows, 100 + t, 0.5)
    assert norms[0] > 0.5 and 0.0 < coefs[0] < 1.0
    record(case=f"clip-above-{'-'.join(TRIPLES[t])}", norm=norms[0], coef=coefs[0])


@pytest.mark.parametrize("t", range(3), ids=["-".join(n) for n in TRIPLES])
def test_a_norm_below_the_bound_is_the_unclipped_adam_flush(t):
    rows = [ROWS[(t + 1 + j) % 3] for j in range(3)]
    got, norms, coefs = _clipped_step_against_its_parts(TRIPLES[t], rows, 200 + t, 1e9)
    assert coefs[0] == 1.0 and norms[0] < 1e9
    flush = Case(TRIPLES[t], rows, 200 + t)
    flush.reduce_plain(live=(True, True, True))
    torch.cuda.synchronize(DEV)
    assert _same(got.state_bits(), flush.state_bits()), "coef = 1 is not sur_flush_all_grads with Adam descriptors"


def test_an_all_zero_gradient_gives_no_nan():
    got, norms, coefs = _clipped_step_against_its_parts(TRIPLES[0], [33, 1, 257], 300, 0.5, zero=True)
    assert norms[0] == 0.0 and coefs[0] == 1.0
    for p, a in zip(got.packs, got.adam):
        assert not _host(p.get(p.gflat)).any() and not _host(a.m).any() and not _host(a.v).any()
        assert np.all(np.isfinite(_host(p.get(p.wflat))))


def test_a_large_chunk_gradient_scales_both_encoders_by_the_same_coefficient():
    got, norms, coefs = _clipped_step_against_its_parts(TRIPLES[1], [33, 257, 1], 400, 0.5, scale=(1e-3, 1e-3, 1e3))
    enc = math.sqrt(sum(float(np.sum(g.astype(np.float64) ** 2)) for g in got.grads()[:2]))
    # the encoders' own norm AFTER the scaling is far below the bound: a per-pack norm would not have touched them
    assert coefs[0] < 1e-3 and enc < 0.5 * 1e-3, (coefs, enc)


@pytest.mark.parametrize("j", (0, 1, 2))
def test_a_pack_without_a_descriptor_is_scaled_and_not_updated(j):
    live = tuple(i != j for i in range(3))
    before = Case(TRIPLES[0], [257, 33, 1], 500 + j)
    got, norms, coefs = _clipped_step_against_its_parts(TRIPLES[0], [257, 33, 1], 500 + j, 0.5, live=live)
    assert coefs[0] < 1.0
    assert np.array_equal(so.bits(got.packs[j].wflat), so.bits(before.packs[j].wflat))
    assert not _host(got.adam[j].m).any() and not _host(got.adam[j].v).any() and int(got.adam[j].step[0]) == 0
    assert np.all(np.isfinite(got.grads()[j])), "the pack is still scaled"


@pytest.mark.parametrize("where", [(0, 0, 5), (2, 40, 100)])
def test_an_infinite_partial_entry_goes_through_the_arithmetic_as_written(where):
    got, norms, coefs = _clipped_step_against_its_parts(TRIPLES[0], [33, 1, 257], 600 + where[0], 0.5, inf_at=where)
    assert math.isinf(norms[0]) and coefs[0] == 0.0
    flat = np.concatenate(got.grads())
    assert int(np.isnan(flat).sum()) == 1 and not flat[~np.isnan(flat)].any()      # inf * 0 and finite * 0


def test_two_consecutive_steps_repeat_bit_for_bit():
    runs = [_clipped_step_against_its_parts(TRIPLES[0], [257, 33, 33], 700, 0.5, calls=2) for _ in range(2)]
    assert _same(runs[0][0].state_bits(), runs[1][0].state_bits()) and runs[0][1] == runs[1][1]
    assert all(int(a.step[0]) == 2 for a in runs[0][0].adam)


# ----------------------------------------------------------------------------------------------------------------------
# the captured step
# ----------------------------------------------------------------------------------------------------------------------
B, T, N, K = 4, 9, 64, 4


def _module(seed=0):
    """The N = 64 training module at tau = 2, tbtt = 4: T = 9 is three chunks (4 + 4 + 1)."""
    from pdecontrol.surrogates.bench_tbptt import build_module
    m = build_module(DEV, seed=seed)
    m.tau, m.tbtt = 2, 4
    return m


def _batches():
    """K seeded batches whose amplitudes alternate: the gradient norm follows the amplitude, so one bound between the
    norms clips some steps and leaves others alone."""
    out = []
    for k in range(K):
        g = torch.Generator().manual_seed(40 + k)
        amp = 1.0 if k % 2 == 0 else 0.25
        out.append(tuple(((torch.rand(B, T, 1, N, generator=g) * 2 - 1) * amp).to(DEV) for _ in range(2)))
    return out


def _grad_norm(module):
    grads = [p.grad.detach().double().reshape(-1) for p in module.surrogate.parameters() if p.grad is not None]
    return float(torch.linalg.vector_norm(torch.cat(grads)))


def _eager(batches, clip):
    """The eager fused closure: training_step -> zero_grad -> backward -> clip_grad_norm_ -> PackAdam.step."""
    from pdecontrol.surrogates import hipops
    m = _module()
    opt = m.configure_optimizers()[0][0]
    assert isinstance(opt, hipops.PackAdam)
    norms = []
    for batch in batches:
        out = m.training_step(batch, 0)
        opt.zero_grad(set_to_none=True)
        out["loss"].backward()
        norms.append(_grad_norm(m))
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(m.surrogate.parameters(), clip)
        opt.step()
    torch.cuda.synchronize(DEV)
    return m, norms


def _flat(m):
    return torch.cat([p.detach().reshape(-1) for p in m.surrogate.parameters()]).double()


def test_the_captured_step_clips_as_the_eager_closure_does():
    from pdecontrol.surrogates.graph_step import GraphedTBPTTStep
    batches = _batches()
    eager0, free = _eager(batches, None)
    clip = math.sqrt(min(free) * max(free))               # between the norms of the two amplitudes
    assert min(free) < 0.8 * clip and 1.25 * clip < max(free), f"scenario unsuitable: unclipped norms {free}"
    eager1, _ = _eager(batches, clip)

    cap0 = _module()
    for batch in batches:
        cap0.fused_step(batch)
    torch.cuda.synchronize(DEV)
    d0 = float((_flat(cap0) - _flat(eager0)).abs().max())

    cap1, seen, grads = _module(), [], []
    for batch in batches:
        cap1.fused_step(batch, clip=clip)
        step = cap1.__dict__["_last_graphed_step"]
        assert step.clip == clip and step.adam_in_flush and step.grad_norm is cap1.surrogate._fused_packs.grad_norm
        seen.append(float(step.grad_norm[0]))
        grads.append(_grad_norm(cap1))
    d1 = float((_flat(cap1) - _flat(eager1)).abs().max())
    lr = cap1.lr
    record(case="captured-step", d0=d0, d1=d1, bound=2 * d0 + K * lr * 1e-5, clip=clip, unclipped_norms=free, norms=seen,
           grad_norms_after=grads)
    assert any(n > clip for n in seen) and any(n < clip for n in seen), (clip, seen)
    for n, g in zip(seen, grads):                         # param.grad after a replay is the clipped gradient
        if n > clip:
            assert g <= clip * (1 + 1e-6), (n, g, clip)
        else:
            assert abs(g - n) <= 1e-6 * n, (n, g)
    assert d1 <= 2 * d0 + K * lr * 1e-5, (d0, d1)
    assert cap1.surrogate._fused_packs.adam_step_count() == K

    # the cache: no clip is today's key and today's object; a clip value and a second shape get graphs of their own over
    # the surrogate's one Adam state
    shapes = (tuple(batches[0][0].shape), tuple(batches[0][1].shape))
    plain = cap1.graphed_step_for(*shapes)
    assert plain is cap1.graphed_step_for(*shapes, clip=None) is cap1.graphed_step_for(*shapes, clip=0) \
        is cap1.graphed_step_for(*shapes, clip=-1.0)
    assert plain is cap1.__dict__["_graphed_steps"][shapes] and plain.clip is None and plain.grad_norm is None
    clipped = cap1.graphed_step_for(*shapes, clip=clip)
    assert clipped is not plain and clipped is cap1.__dict__["_graphed_steps"][shapes + (clip,)]
    small = tuple(t[:2].contiguous() for t in batches[0])
    cap1.fused_step(small, clip=clip)
    other = cap1.__dict__["_last_graphed_step"]
    assert other is not clipped and other.g_main is not clipped.g_main and other.clip == clip
    assert cap1.surrogate._fused_packs.adam_step_count() == K + 1
    with pytest.raises(ValueError, match="data-parallel"):
        GraphedTBPTTStep(cap1, shapes[0], shapes[1], distributed=True, clip=clip)


def test_the_shim_trainers_clip_value_reaches_the_captured_step():
    """``graphed=True`` under ``Trainer(gradient_clip_val=...)``: manual optimization, so the Trainer's own clip never runs
    and the module's captured step takes the value."""
    from pdecontrol._compat.lightning import IS_SHIM, pl
    from pdecontrol.surrogates.bench_tbptt import build_module, synthetic_batch
    if not IS_SHIM:
        pytest.skip("pytorch-lightning is installed: its Trainer is not the shim")
    batch = synthetic_batch(B=4, T=12, device=DEV)
    m = build_module(DEV, graphed=True)
    pl.Trainer(max_steps=2, max_epochs=1, gradient_clip_val=0.5).fit(m, train_dataloaders=[batch] * 2)
    torch.cuda.synchronize(DEV)
    keys = list(m.__dict__["_graphed_steps"])
    assert len(keys) == 1 and keys[0][2] == 0.5
    step = m.__dict__["_graphed_steps"][keys[0]]
    norm = float(step.grad_norm[0])
    assert step.clip == 0.5 and math.isfinite(norm) and norm > 0.5
    assert _grad_norm(m) <= 0.5 * (1 + 1e-6)
    assert m.surrogate._fused_packs.adam_step_count() == 2
    plain = build_module(DEV, graphed=True)
    pl.Trainer(max_steps=2, max_epochs=1).fit(plain, train_dataloaders=[batch] * 2)
    assert [len(k) for k in plain.__dict__["_graphed_steps"]] == [2]


def test_the_torch_kernel_route_clips_inside_its_graph():
    """With the fused kernels switched off the captured function is backward -> ``clip_grad_norm_`` -> ``opt.step()``."""
    from pdecontrol.surrogates import ops
    from pdecontrol.surrogates.graph_step import GraphedTBPTTStep
    batch = _batches()[0]
    with ops.fused(False):
        free = GraphedTBPTTStep(_module(), tuple(batch[0].shape))
        free.step(*batch)
        torch.cuda.synchronize(DEV)
        first = _grad_norm(free.module)
        clip = 0.5 * first
        step = GraphedTBPTTStep(_module(), tuple(batch[0].shape), clip=clip)
        assert not step.adam_in_flush and not free.adam_in_flush and free.grad_norm is None
        step.step(*batch)
        torch.cuda.synchronize(DEV)
    seen = float(step.grad_norm[0])
    # plain torch kernels: the backward reductions are not bit-reproducible between two captures (tests/test_surrogate_gpu.py)
    assert abs(seen - first) <= 1e-4 * first, (seen, first)
    assert _grad_norm(step.module) <= clip * (1 + 1e-6)


# ----------------------------------------------------------------------------------------------------------------------
# the phase: kernel tier against the loop tier, both clipped
# ----------------------------------------------------------------------------------------------------------------------
LOSS_RTOL, HSTEP_RTOL = 1e-5, 1e-4            # the kernel-versus-loop tolerances of tests/test_surrogate_phase_gpu.py


def _datamodule(M, env, tf):
    from pdecontrol.mbrl.device_replay import DeviceExperienceReplay
    from pdecontrol.surrogates.common.datamodule import PDEDataModule
    sink = DeviceExperienceReplay(device="cuda")
    for part in sc.split_replay(M, sc.scripted_episodes(env.N)):
        sink.extend(part)
    keys = list(sink.episodes)
    return PDEDataModule(data=sink.data, curriculum=sc.curriculum(), device_data="cuda", train=keys[:4], val=keys[4:],
                         bootstrapping=True, stransf=tf.replay_to_world, tau=5, batch_size=8)


def _phase(M, env, tf, clip, tier, max_steps):
    from pdecontrol.mbrl import surrogate_phase as sp
    module, fit = sc.training_module(M, env, tf, "cuda", seed=5), sp.FitState()
    np.random.seed(17)
    torch.manual_seed(17)
    value = sp.update_surrogate(module, _datamodule(M, env, tf), fit, max_steps=max_steps, min_steps=0, patience=1,
                                gradient_clip_val=clip, tier=tier)
    torch.cuda.synchronize(DEV)
    return module, fit, value


def test_the_phase_clips_on_both_tiers(monkeypatch):
    import _rollout_scenario as rsc
    monkeypatch.setenv("PDECONTROL_PIPELINED", "1")
    M = rsc.repo_namespace()
    env = M.Env()
    tf = rsc.transforms(M, env)
    probe, fit, _ = _phase(M, env, tf, 1e30, None, 1)     # one step under a bound nothing reaches: the norm, measured
    assert fit.tier == "kernel", fit.tier_reason
    first = float(probe.surrogate._fused_packs.grad_norm[0])
    assert math.isfinite(first) and first > 0
    clip = 0.5 * first
    kernel, kfit, kvalue = _phase(M, env, tf, clip, None, 5)
    loop, lfit, lvalue = _phase(M, env, tf, clip, "loop", 5)
    assert kfit.tier == "kernel" and lfit.tier == "loop"
    for m in (kernel, loop):                              # both trained through clipped captured steps, and only those
        keys = list(m.__dict__["_graphed_steps"])
        assert keys and all(len(k) == 3 and k[2] == clip for k in keys), keys
    assert (kfit.current_epoch, kfit.global_step, kfit.wait_count) == (lfit.current_epoch, lfit.global_step, lfit.wait_count)
    assert len(kfit.history) == len(lfit.history)
    for g, w in zip(kfit.history, lfit.history):
        for name in ("Val. Loss", "Val. Scaled Loss", "Val. Delta Loss"):
            assert abs(g[name] - w[name]) <= LOSS_RTOL * abs(w[name]), (name, g[name], w[name])
        np.testing.assert_allclose(g["hsteploss"], w["hsteploss"], rtol=HSTEP_RTOL)
    assert abs(kvalue - lvalue) <= LOSS_RTOL * abs(lvalue)
    diff = float((_flat(kernel) - _flat(loop)).abs().max())
    unclipped, _, _ = _phase(M, env, tf, None, None, 5)
    moved = float((_flat(kernel) - _flat(unclipped)).abs().max())
    record(case="phase-kernel-vs-loop", clip=clip, first_norm=first, max_parameter_difference=diff, clipped_vs_unclipped=moved,
           val_loss=[kvalue, lvalue])
    # the two tiers replay the same captured steps on the same batches (the gather is the host loader's batch bit for bit):
    # parameters and Adam state (moments, step counters) byte for byte, as tests/test_surrogate_phase_gpu.py asks of its loop
    (kp, ka), (lp, la) = sc.optimizer_state(kernel), sc.optimizer_state(loop)
    assert len(kp) == len(lp) and all(a.tobytes() == b.tobytes() for a, b in zip(kp, lp)), "parameters differ"
    assert len(ka) == len(la) and all(a.tobytes() == b.tobytes() for a, b in zip(ka, la)), "Adam state differs"
    assert moved > 0.0, "the clip changed nothing"
