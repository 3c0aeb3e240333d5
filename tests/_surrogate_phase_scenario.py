"""Shared pieces of the surrogate-update phase tests (tests/test_surrogate_phase_host.py, tests/test_surrogate_phase_gpu.py):
the numpy twin of ``sur_gather_windows`` -- the CPU statement of the kernel's contract --, the inputs of its test matrix,
a scripted ragged replay with the controller's connector, and the hand-written fit loop the phase is compared with."""
import types

import numpy as np
import torch

import _rollout_scenario as rsc
from pdecontrol.mbrl.recognition import FieldMap

FILL = -7.5                                     # what the tests put around the outputs and into unmapped slab rows


# ----------------------------------------------------------------------------------------------------------------------
# the numpy twin of sur_gather_windows
# ----------------------------------------------------------------------------------------------------------------------
def gather_twin(obs, actions, first, L, obs_map, act_maps, rowmap=None, rows=None):
    """``sur_gather_windows`` in numpy: (states [B, L, No], actions [B, L, Na]) of the windows that start at the logical
    rows ``first``.  ``obs`` [rows, obs_width] and ``actions`` [rows, A] are the packed fields, ``rowmap`` the logical to
    physical map or None; the logical row count is ``len(rowmap)`` (``len(obs)`` without one).  The affine map is
    ``FieldMap.apply_numpy``'s four separately rounded fp32 steps and the forcing product is the fma chain in action
    order.  A logical row outside [0, total) or a mapped row outside [0, rows) gives a NaN row."""
    act_in, F, act_out = act_maps
    obs, actions = np.asarray(obs, np.float32), np.asarray(actions, np.float32)
    total = len(obs) if rowmap is None else len(rowmap)
    rows = len(obs) if rows is None else rows
    logical = np.asarray(first, np.int64)[:, None] + np.arange(L, dtype=np.int64)[None, :]
    ok = (logical >= 0) & (logical < total)
    phys = np.where(ok, logical, 0)
    if rowmap is not None:
        phys = np.asarray(rowmap, np.int64)[phys]
        ok &= (phys >= 0) & (phys < rows)
        phys = np.where(ok, phys, 0)
    states = obs_map.apply_numpy(obs[phys])
    a = actions[phys]
    if F is not None:
        a = rsc.fma_chain(act_in.apply_numpy(a), np.asarray(F, np.float32))
    acts = act_out.apply_numpy(a)
    states[~ok], acts[~ok] = np.nan, np.nan
    return states, acts


def _coef(rs, width):
    """Random [4, width] coefficients (a, b - a, d - c, c) with b - a away from zero."""
    return torch.from_numpy(np.stack([rs.uniform(-1, 1, width), rs.uniform(0.5, 2.0, width) * rs.choice([-1, 1], width),
                                      rs.uniform(0.25, 3.0, width), rs.uniform(-1, 1, width)]).astype(np.float32))


def gather_case(seed, N, A, B, L, forcing, stride, start, coefs, permuted, total=None):
    """Numpy inputs of one ``sur_gather_windows`` case: a replay of ``total`` logical rows (obs width N, action width A),
    the maps of a connector with the sensor (start, stride) on both outputs, ``first`` of B windows inside the replay."""
    rs = np.random.RandomState(seed)
    total = (B * L + 9) if total is None else total
    rows = total + 7 if permuted else total
    obs = np.full((rows, N), FILL, np.float32)
    actions = np.full((rows, A), FILL, np.float32)
    rowmap = rs.permutation(rows)[:total].astype(np.int64) if permuted else None
    where = rowmap if permuted else np.arange(total)
    obs[where] = rs.standard_normal((total, N)).astype(np.float32)
    actions[where] = rs.uniform(-1, 1, (total, A)).astype(np.float32)
    width = lambda n, s0: len(range(s0, n, stride))
    F = rs.standard_normal((A, N)).astype(np.float32) if forcing else None
    act_row = N if forcing else A
    astart = start if start < act_row else 0                       # (A = 1 without forcing: the only column)
    obs_map = FieldMap(start, stride, width(N, start), _coef(rs, width(N, start)) if coefs else None)
    act_in = FieldMap(0, 1, A, _coef(rs, A) if coefs and forcing else None)
    act_out = FieldMap(astart, stride, width(act_row, astart), _coef(rs, width(act_row, astart)) if coefs else None)
    first = rs.randint(0, total - L + 1, B).astype(np.int64)
    return types.SimpleNamespace(obs=obs, actions=actions, rowmap=rowmap, rows=rows, total=total, first=first, L=L, B=B,
                                 obs_map=obs_map, act_maps=(act_in, None if F is None else torch.from_numpy(F), act_out))


def case_twin(c, first=None):
    act_in, F, act_out = c.act_maps
    return gather_twin(c.obs, c.actions, c.first if first is None else first, c.L, c.obs_map,
                       (act_in, None if F is None else F.numpy(), act_out), c.rowmap, c.rows)


# ----------------------------------------------------------------------------------------------------------------------
# a scripted ragged replay under the controller's connector
# ----------------------------------------------------------------------------------------------------------------------
def scripted_episodes(N, A=4, lengths=(30, 45, 33, 41, 38, 36), seed=3):
    """Per episode (obs [T + 1, 1, N], actions [T, 1, A]): a smooth travelling field and uniform actions."""
    rs = np.random.RandomState(seed)
    x = np.linspace(0, 2 * np.pi, N, endpoint=False)
    out = []
    for T in lengths:
        phase, amp = rs.uniform(0, 6), rs.uniform(0.5, 1.5)
        t = np.arange(T + 1)[:, None]
        field = amp * np.sin(x[None, :] + phase + 0.3 * t) + 0.5 * np.cos(2 * x[None, :] - 0.2 * t)
        out.append((field.astype(np.float32)[:, None, :], rs.uniform(-1, 1, (T, 1, A)).astype(np.float32)))
    return out


def host_replay(M, episodes):
    """The episodes in an ``ExperienceReplay``, one env, each ending truncated."""
    rp = M.Replay()
    for field, acts in episodes:
        T = len(acts)
        for t in range(T):
            rp.add([M.Sample(field[t], acts[t], field[t + 1], np.float32(-1.0), False, t == T - 1, np.int32(t + 1))])
    return rp


def packed(rp):
    """(obs [total, N], actions [total, A], starts {key: first logical row}) of a host replay in packed order."""
    keys = list(rp.obs.keys())
    starts, off = {}, 0
    for k in keys:
        starts[k] = off
        off += len(rp.obs[k])
    obs = np.concatenate([np.asarray(rp.obs[k], np.float32).reshape(len(rp.obs[k]), -1) for k in keys])
    acts = np.concatenate([np.asarray(rp.actions[k], np.float32).reshape(len(rp.actions[k]), -1) for k in keys])
    return obs, acts, starts


def firsts(dataset, starts, indices=None):
    """First logical rows of the dataset's items: ``starts[key] + offset`` of ``locate_many``."""
    indices = np.arange(len(dataset)) if indices is None else indices
    keys, offs = dataset.locate_many(indices)
    return np.asarray([starts[k] for k in keys], np.int64) + offs


def twin_batches(dataset, batch_size, obs, acts, starts, obs_map, act_maps):
    """What the loader of ``dataset`` yields, from the twin: a list of (states [B, L, 1, No], actions [B, L, 1, Na])."""
    first = firsts(dataset, starts)
    act_in, F, act_out = act_maps
    maps = (act_in, None if F is None else np.asarray(F), act_out)
    out = []
    for i0 in range(0, len(first), batch_size):
        s, a = gather_twin(obs, acts, first[i0:i0 + batch_size], dataset.length, obs_map, maps)
        out.append((s[:, :, None, :], a[:, :, None, :]))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# sur_val_loss in fp64
# ----------------------------------------------------------------------------------------------------------------------
def val_loss_fp64(states, out_all, d_all, delta, mean, stdv, inv_coef):
    """The formula of ``sur_val_loss`` in fp64 over fp32 inputs: states [B,T,1,N], out_all / d_all [T,B,1,N] time-major,
    inv_coef [4,N] or None.  Returns a dict of the three losses, ``hsteploss`` [T], and the fp64 error sums
    (unscaled, scaled, delta, then per step) the accumulator holds."""
    s = np.asarray(states, np.float64)
    out, d = np.asarray(out_all, np.float64).transpose(1, 0, 2, 3), np.asarray(d_all, np.float64).transpose(1, 0, 2, 3)
    decoded = np.concatenate((s[:, :1], out[:, :-1]), axis=1)
    deltas = ((s[:, 1:] - s[:, :-1]) / np.float64(np.float32(delta)) - np.float64(np.float32(mean))) / np.float64(np.float32(stdv))
    if inv_coef is None:
        affine = lambda v: v
    else:
        a, ba, dc, c = (np.asarray(inv_coef[i], np.float64) for i in range(4))
        affine = lambda v: (v - a) / ba * dc + c
    e_delta, e_scaled, e_un = (d[:, :-1] - deltas) ** 2, (decoded - s) ** 2, (affine(decoded) - affine(s)) ** 2
    per_step = e_un.sum(axis=(0, 2, 3))
    return {"loss": e_un.mean(), "scaled": e_scaled.mean(), "delta": e_delta.mean(), "hsteploss": e_un.mean(axis=(0, 2, 3)),
            "sums": np.concatenate(([e_un.sum(), e_scaled.sum(), e_delta.sum()], per_step)), "deltas": deltas,
            "decoded": affine(decoded)}


# ----------------------------------------------------------------------------------------------------------------------
# the phase against a hand-written loop
# ----------------------------------------------------------------------------------------------------------------------
def training_module(M, env, tf, device, seed=0, scaled=True, N=None):
    """The controller's training module over the N = 64 factory (the any-N factory otherwise): tau 5, tbtt 10, the
    connector ``tf.replay_to_world``, and -- ``scaled`` -- delta statistics in a ``Normalize`` the surrogate's
    ``dscaling`` and the module's ``undscaling`` share."""
    N = env.N if N is None else N
    torch.manual_seed(seed)
    und = None
    if scaled:
        norm = M.T.Normalize(aggregate=True, batched=True)
        norm.mean, norm.var, norm.count = torch.full((1, 1, 1), 0.01), torch.full((1, 1, 1), 0.5), 100
        und = M.T.BatchTransform(norm)
    f = M.factory_cls() if N == 64 else M.factory_n_cls()
    tstep = env.cfg_steps * env.dt
    sur = f.surrogate(delta=tstep, dscaling=None if und is None else und.Inverse, tau=5, **f.model(N=N))
    return M.TrainingModule(surrogate=sur, loss=torch.nn.MSELoss(reduction="none"), tstep=tstep, delta=tstep, undscaling=und,
                            stransf=tf.replay_to_world, tau=5, tbtt=10).to(device)


def split_replay(M, episodes, cut=3):
    """Two host replays holding the first ``cut`` and the remaining episodes: extending with one after the other gives
    the same keys on a host and on a device replay, and slabs whose rows are not in packed order."""
    return host_replay(M, episodes[:cut]), host_replay(M, episodes[cut:])


def curriculum():
    from pdecontrol.surrogates.common.schedulers import StepScheduler
    return StepScheduler(steptype="epoch", steps=[0], values=[3, 6])       # T = 8 in epoch 0, 11 afterwards


def reference_fit(module, datamodule, fit, packed_replay, maps, *, max_steps, min_steps, patience, max_epochs=None):
    """The rule of ``update_surrogate`` written out by hand: per epoch the datamodule's own (host) loaders are built --
    so numpy's generator and the curriculum are consumed as by the phase --, training feeds ``module.fused_step`` from
    numpy-twin batches uploaded to the device, validation goes through ``module.validation_step`` (the caller keeps it
    on the torch ops) and its epoch value is the sample-weighted mean over batches."""
    obs, acts, starts = packed_replay
    obs_map, act_maps = maps
    device = module.device
    up = lambda pair: tuple(torch.from_numpy(np.ascontiguousarray(x)).to(device) for x in pair)
    fit.wait_count = 0
    target, min_target = fit.global_step + max_steps, fit.global_step + min_steps
    datamodule.trainer = fit
    epochs = 0
    while True:
        loader = datamodule.train_dataloader()
        module.train()
        for pair in twin_batches(loader.dataset, datamodule.batch_size, obs, acts, starts, obs_map, act_maps):
            if fit.global_step >= target:
                break
            module.fused_step(up(pair))
            fit.global_step += 1
        loader = datamodule.val_dataloader()
        module.eval()
        sums, hstep, count = np.zeros(3), 0.0, 0
        with torch.no_grad():
            for bidx, pair in enumerate(twin_batches(loader.dataset, datamodule.batch_size, obs, acts, starts, obs_map, act_maps)):
                out = module.validation_step(up(pair), bidx)
                b = len(pair[0])
                sums += b * np.asarray([float(out["loss"]), float(module.logged["Val. Scaled Loss"]),
                                        float(module.logged["Val. Delta Loss"])])
                hstep = hstep + b * out["hsteploss"].double().cpu().numpy()
                count += b
        value = sums[0] / count
        fit.history.append({"Val. Loss": value, "Val. Scaled Loss": sums[1] / count, "Val. Delta Loss": sums[2] / count,
                            "hsteploss": hstep / count, "epoch": fit.current_epoch, "global_step": fit.global_step})
        if value < fit.best_score:
            fit.best_score, fit.wait_count = value, 0
        else:
            fit.wait_count += 1
        stop = fit.wait_count >= patience or not np.isfinite(value)
        fit.current_epoch += 1
        epochs += 1
        if fit.global_step >= target or (stop and fit.global_step >= min_target) or (max_epochs is not None and epochs >= max_epochs):
            return float(value)


def optimizer_state(module):
    """Parameters and the captured step's Adam state (moments and step counter of every pack), as numpy."""
    params = [p.detach().cpu().numpy() for p in module.surrogate.parameters()]
    packs = module.surrogate._fused_packs.packs
    assert all(p._adam_state is not None for p in packs), "the captured step keeps its Adam state on the packs"
    return params, [t.cpu().numpy() for p in packs for t in p._adam_state[:3]]
