"""What the controller's three device-resident phases (policy_phase.py, imagination_phase.py, collection_phase.py) share
when they decide whether the kernels implement a connector or a wrapper stack: transform chains reduced to a column
sensor and per-column affine coefficients, the checks both stack recognisers make, and the once-per-reason notice of a
phase that runs on its other tier."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from pdecontrol.surrogates import ops
from pdegym.common import transforms as tr
from pdegym.common import vec_wrappers as vw


class Unrecognized(Exception):
    """A connector or a stack the kernels do not implement; ``str()`` is the reason."""


@dataclass
class FieldMap:
    """What a recognised chain does to the last axis of a field: output column j reads input column
    ``start + j * stride`` and maps it through ``((v - a) / (b - a)) * (d - c) + c`` with ``coef[:, j]`` =
    (a, b - a, d - c, c); ``coef`` None is the identity."""
    start: int
    stride: int
    width: int
    coef: Optional[torch.Tensor]

    def apply_numpy(self, values):
        """The map in numpy, in the four separately rounded fp32 steps of ``ScaleTransform._affine``."""
        v = np.asarray(values, dtype=np.float32)[..., self.start::self.stride][..., :self.width]
        if self.coef is None:
            return v.copy()
        a, ba, dc, c = (self.coef[i].numpy() for i in range(4))
        with np.errstate(invalid="ignore", divide="ignore"):
            return (((v - a) / ba) * dc + c).astype(np.float32)


def _settled(norm):
    """A ``Normalize`` whose statistics can no longer move: frozen and fitted.  It is then an affine map per column."""
    return bool(norm.frozen) and norm.mean is not None and norm.var is not None


def flatten(t, normalize=False):
    """The chain as a list of ("sensor", stride) / ("scale", ScaleTransform, inverse) steps.  With ``normalize`` a
    ``Normalize`` that is frozen and fitted is a ("norm", Normalize, inverse) step as well; without it, and for every other
    ``Normalize``, the chain is refused.  Only the callers whose kernels are pinned with such a step ask for it
    (``world_connector`` and the validation loss)."""
    if t is None or isinstance(t, tr.Identity):
        return []
    if isinstance(t, tr.Operation):
        return [step for inner in t.transforms for step in flatten(inner, normalize)]
    if isinstance(t, tr._OperationInverse):
        return [step for inner in t.transfs for step in flatten(inner, normalize)]
    if isinstance(t, tr._BatchInverse):
        return flatten(t.transform, normalize)
    if isinstance(t, tr.BatchTransform):
        return flatten(t.transform, normalize)
    if isinstance(t, tr.SensorTransform):
        return [("sensor", int(t.stride))]
    if type(t) is tr.ScaleTransform:
        return [("scale", t, False)]
    if normalize and type(t) is tr.Normalize and _settled(t):
        return [("norm", t, False)]
    if type(t) is tr._InverseView:
        inner = t.transf
        if isinstance(inner, tr.Identity):
            return []
        if type(inner) is tr.ScaleTransform:
            return [("scale", inner, True)]
        if normalize and type(inner) is tr.Normalize and _settled(inner):
            return [("norm", inner, True)]
        if isinstance(inner, tr.SensorTransform) and int(inner.stride) == 1:
            return []
        raise Unrecognized(f"the inverse of a {type(inner).__name__}")
    raise Unrecognized(f"a {type(t).__name__}")


def _columns(stat, width, what):
    stat = torch.as_tensor(stat).detach().cpu()
    if stat.dtype != torch.float32:
        raise Unrecognized(f"a ScaleTransform with {what} in {str(stat.dtype).replace('torch.', '')}")
    if stat.numel() == 1:
        return stat.reshape(1).expand(width)
    if stat.shape[-1] == width and stat.numel() == width:
        return stat.reshape(width)
    raise Unrecognized(f"a ScaleTransform whose {what} of shape {tuple(stat.shape)} is not one value or one per column")


_HOST_COPIES = {}


def _host_copy(stat):
    """``stat`` on the host.  The copy of a device tensor is cached per tensor object -- a frozen ``Normalize`` never
    re-assigns its statistics --, so recognising the same chain again (every validation batch does) costs no
    device-to-host copy and no synchronisation."""
    if not (isinstance(stat, torch.Tensor) and stat.is_cuda):
        return torch.as_tensor(stat).detach().cpu()
    hit = _HOST_COPIES.get(id(stat))
    if hit is None or hit[0] is not stat:
        if len(_HOST_COPIES) > 256:
            _HOST_COPIES.clear()
        hit = _HOST_COPIES[id(stat)] = (stat, stat.detach().cpu())
    return hit[1]


def _normalize_coef(norm, inverse, width):
    """The four-step coefficients of a frozen, fitted ``Normalize``: with s = sqrt(var + epsilon) in fp32 torch, as
    ``_fwd`` / ``_inv`` take it, forward is (mean, s, 1, -0.0) and the inverse (+0.0, 1, s, mean).  Multiplying by 1 and
    subtracting +0.0 change no bit; the forward map adds MINUS zero, so that a quotient that underflows to -0.0 stays
    -0.0."""
    scale = _statistic(torch.sqrt(_host_copy(norm.var) + norm.epsilon), width, "variance")
    mean = _statistic(_host_copy(norm.mean), width, "mean")
    zero, one = torch.zeros(width), torch.ones(width)
    return torch.stack([zero, one, scale, mean] if inverse else [mean, scale, one, -zero])


def field_map(chain, width, normalize=False):
    """``FieldMap`` of a chain over a field whose rows are ``width`` columns wide; raises ``Unrecognized``.
    ``normalize``: take a frozen, fitted ``Normalize`` as the affine map it is (``flatten``)."""
    start, stride, coef = 0, 1, None
    for step in flatten(chain, normalize):
        if step[0] == "sensor":
            r = step[1]
            if r < 1:
                raise Unrecognized(f"a SensorTransform of stride {r}")
            start, stride = start + (r // 2) * stride, stride * r
            if coef is not None:
                coef = coef[:, r // 2::r]
            width = len(range(r // 2, width, r))
            if width < 1:
                raise Unrecognized("sensors that leave no column")
        else:
            if coef is not None:
                raise Unrecognized("two scalings in a row")
            _, scale, inverse = step
            if step[0] == "norm":
                coef = _normalize_coef(scale, inverse, width)
                continue
            vmin, vmax, lower, upper = (torch.as_tensor(s).detach().cpu() for s in (scale.vmin, scale.vmax, scale.lower, scale.upper))
            a, b, c, d = (lower, upper, vmin, vmax) if inverse else (vmin, vmax, lower, upper)
            coef = torch.stack([_columns(a, width, "bounds"), _columns(b - a, width, "bounds"),
                                _columns(d - c, width, "bounds"), _columns(c, width, "bounds")])
    return FieldMap(start, stride, width, None if coef is None else coef.contiguous())


# ---- inverse observation chains (the surrogate test phase) ------------------------------------------------------------
def _leaves(t):
    """The transforms of a chain in application order, ``Operation``s and ``BatchTransform``s opened up."""
    if isinstance(t, (tr.BatchTransform, tr._BatchInverse)):
        return _leaves(t.transform)
    steps = _steps(t)
    return steps if len(steps) == 1 and steps[0] is t else [leaf for step in steps for leaf in _leaves(step)]


def _statistic(stat, width, what):
    if stat is None:
        raise Unrecognized(f"a Normalize without a fitted {what}")
    stat = torch.as_tensor(stat).detach().cpu()
    if stat.dtype != torch.float32:
        raise Unrecognized(f"a Normalize with its {what} in {str(stat.dtype).replace('torch.', '')}")
    if stat.numel() == 1:
        return stat.reshape(1).expand(width)
    if stat.shape[-1] == width and stat.numel() == width:
        return stat.reshape(width)
    raise Unrecognized(f"a Normalize whose {what} of shape {tuple(stat.shape)} is not one value or one per column")


def inverse_map(chain, width):
    """``(kind, coef)`` of an inverse observation chain (``stransf.otransf.Inverse``) over rows of ``width`` columns, as
    ``ks_eval_rows_device`` takes it: identity sensors and at most one scaling.  Kind 0 is the identity (``coef`` None);
    kind 1 a ``ScaleTransform`` in either direction, ``coef`` [4, width] = (a, b - a, d - c, c) as in ``FieldMap``; kind 2
    the inverse of a ``Normalize`` with scalar or per-column statistics, ``coef`` [2, width] = (sqrt(var + epsilon), mean),
    the square root taken in fp32 torch as ``Normalize._inv`` takes it.  Raises ``Unrecognized``."""
    kind, coef = 0, None
    for leaf in _leaves(chain):
        inverse = type(leaf) is tr._InverseView
        inner = leaf.transf if inverse else leaf
        if inner is None or isinstance(inner, tr.Identity):
            continue
        if isinstance(inner, tr.SensorTransform):
            if int(inner.stride) != 1:
                raise Unrecognized(f"a SensorTransform of stride {inner.stride}")
            continue
        if kind:
            raise Unrecognized("two scalings in a row")
        if type(inner) is tr.ScaleTransform:
            kind, coef = 1, field_map(leaf, width).coef
        elif type(inner) is tr.Normalize and inverse:
            scale = None if inner.var is None else torch.sqrt(torch.as_tensor(inner.var).detach().cpu() + inner.epsilon)
            kind = 2
            coef = torch.stack([_statistic(scale, width, "variance"), _statistic(inner.mean, width, "mean")]).contiguous()
        else:
            raise Unrecognized(f"a {type(inner).__name__}" if not inverse else f"the inverse of a {type(inner).__name__}")
    return kind, coef


# ---- what both stack recognisers check -------------------------------------------------------------------------------
def is_forcing(t):
    if isinstance(t, tr.BatchTransform):
        t = t.transform
    return t if type(t) is tr.GaussianForcing else None


def split_at_forcing(transforms):
    """(transforms before the forcing, the ``GaussianForcing`` or None, transforms after it) of a list applied left to
    right; without a forcing everything is "before".  Raises ``Unrecognized`` on a second forcing."""
    before, forcing, after = [], None, []
    for t in transforms:
        f = is_forcing(t)
        if f is not None:
            if forcing is not None:
                raise Unrecognized("two forcings")
            forcing = f
        else:
            (before if forcing is None else after).append(t)
    return before, forcing, after


def forcing_matrix(forcing):
    """The fp32 [A, L] matrix of a ``GaussianForcing``, contiguous on the host."""
    matrix = forcing.forcing.detach().cpu()
    if matrix.dtype != torch.float32 or matrix.dim() != 2:
        raise Unrecognized("a forcing matrix that is not fp32 [A, N]")
    return matrix.contiguous()


def action_maps(before, forcing, after, normalize=False):
    """(``act_in`` FieldMap over the A action columns, the forcing matrix, ``act_out`` FieldMap over its L columns) of an
    action chain split by ``split_at_forcing`` around a forcing."""
    matrix = forcing_matrix(forcing)
    A, L = (int(v) for v in matrix.shape)
    act_in = field_map(tr.Operation(before), A, normalize)
    if (act_in.start, act_in.stride, act_in.width) != (0, 1, A):
        raise Unrecognized("a sensor on the agent's actions")
    return act_in, matrix, field_map(tr.Operation(after), L, normalize)


def _steps(t):
    """The transforms of a chain in application order, ``Operation``s opened up."""
    if isinstance(t, tr.Operation):
        return [leaf for inner in t.transforms for leaf in _steps(inner)]
    if isinstance(t, tr._OperationInverse):
        return [leaf for inner in t.transfs for leaf in _steps(inner)]
    return [t]


def world_connector(stransf, obs_width, act_width):
    """What a replay connector does to the ``obs`` and ``actions`` of a sample, as ``sur_gather_windows`` takes it:
    (obs ``FieldMap``, (``act_in`` FieldMap with an identity sensor, the forcing matrix or None, ``act_out`` FieldMap)).

    Recognised: a ``SampleTransform`` whose ``otransf`` flattens to sensors and at most one scaling and whose ``atransf``
    flattens to at most one scaling, at most one ``GaussianForcing``, then at most one scaling and sensors -- the
    controller's ``replay_to_world`` (mbrl.py:182-185).  Without a forcing ``act_in`` is the identity and ``act_out``
    carries the whole action chain.  Anything else raises ``Unrecognized``."""
    if type(stransf) is not tr.SampleTransform:
        raise Unrecognized(f"a {type(stransf).__name__} in place of the SampleTransform")
    obs = field_map(stransf.otransf, int(obs_width), normalize=True)
    before, forcing, after = split_at_forcing(_steps(stransf.atransf))
    A = int(act_width)
    if forcing is None:
        return obs, (FieldMap(0, 1, A, None), None, field_map(tr.Operation(before), A, normalize=True))
    act_in, matrix, act_out = action_maps(before, forcing, after, normalize=True)
    if act_in.width != A:
        raise Unrecognized(f"a forcing over {act_in.width} actuators for actions of {A} columns")
    return obs, (act_in, matrix, act_out)


def updates_statistics(wrapper):
    """A ``TransformActionWrapper`` whose step changes its transform: not frozen, over a scaling that is not frozen."""
    if wrapper.frozen or is_forcing(wrapper.transform) is not None:
        return False
    return any(step[0] == "scale" and not step[1].frozen for step in flatten(wrapper.transform, normalize=True))


def action_store(env, stack, otherwise):
    """``env`` is the one-step ``StoreNActionsVecWrapper`` that is ``stack.astore``; ``otherwise`` is the reason when it
    is not that store."""
    if type(env) is not vw.StoreNActionsVecWrapper or env is not stack.astore:
        raise Unrecognized(otherwise)
    if env.num_steps != 1:
        raise Unrecognized(f"an action store of {env.num_steps} steps")


def observation_store(env, stack):
    """``env`` is the one-step ``StoreNObsVecWrapper`` that is ``stack.ostore``; returns what it wraps."""
    if type(env) is not vw.StoreNObsVecWrapper or env is not stack.ostore:
        raise Unrecognized(f"a {type(env).__name__} in place of the observation store")
    if env.num_steps != 1:
        raise Unrecognized(f"an observation store of {env.num_steps} steps")
    return env.env


def one_channel_each(env, what):
    """(observation columns, action columns) of ``env`` (``what``: "a world", "an env"), one channel each."""
    oshape, ashape = tuple(env.single_observation_space.shape), tuple(env.single_action_space.shape)
    if len(oshape) != 2 or oshape[0] != 1 or len(ashape) != 2 or ashape[0] != 1:
        raise Unrecognized(f"{what} with observations {oshape} and actions {ashape} (one channel each)")
    return oshape[1], ashape[1]


def same_device(a, b):
    """``a``, a device with its index, is the device ``b`` names ("cuda" is the current device)."""
    return a == torch.empty(0, device=b).device


def notice(sentence, reason, expected=False):
    """Logs ``sentence % reason`` the first time ``reason`` is met: a warning, or an info line for an ``expected`` one."""
    if reason not in ops._NOTIFIED:
        ops._NOTIFIED.add(reason)
        (ops._LOG.info if expected else ops._LOG.warning)(sentence, reason)
