"""Truncated-BPTT training module of the surrogate.

API mirror of the reference's ``pdecontrol/surrogates/training.py`` (``PDETrainingModule`` :14-62,
``training_step`` :64-130, ``validation_step`` :132-174, ``test_step`` :176-271,
``configure_optimizers`` :273-278): same constructor, same returned-dict keys, same logged metric
names ("Train Loss", "Val. Loss", ...).

What is different under the hood: logged values stay tensors (no ``.item()`` host sync inside
the step), time grids are Python-side, and ``fused_step`` offers the whole
forward + backward + Adam update as ONE replayable HIP graph for fixed batch shapes.

How the reference's caller reaches the fast paths (``pl.Trainer.fit``, pdecontrol/mbrl/mbrl.py:593):
  * default (automatic optimization): Lightning calls ``training_step`` eagerly, then ``backward`` and
    ``optimizer.step``.  On a CUDA device ``training_step`` runs on the fused HIP kernels (21 launches) and
    ``configure_optimizers`` returns a single-kernel (``fused=True``) Adam.
  * ``graphed=True`` (constructor keyword, i.e. ``--training '{"initial": {"graphed": true, ...}}'`` through the
    reference's own config channel, mbrl.py:230-245; or ``PDECONTROL_GRAPHED=1``): the module switches to Lightning's
    manual optimization and ``training_step`` replays the captured graph (forward + backward + Adam in one
    ``hipGraphLaunch``).  The optimizer returned by ``configure_optimizers`` then only carries the learning rate
    (schedulers keep working: the graph reads it from a device scalar); its ``step`` is never called.
"""
import collections
import os
from typing import Callable

import numpy as np
import torch

from pdecontrol._compat.lightning import pl
from pdecontrol.mbrl.types import ModelRollout
from pdecontrol.surrogates.surrogate import AutoRegPDESurrogate, LatentAutoRegPDESurrogate, PDESurrogate
from pdegym.common.transforms import BatchTransform, Identity, SampleTransform


# what _test_kernel_plan hands to _test_metrics_device: the inverse observation map (kind, device coefficients or None),
# the family ("ks" / "burgers") and the env that launches, and the sizes and names of what its two launches write
_TestPlan = collections.namedtuple("_TestPlan", "kind coef family backend row_stats tables names")


class _GraphOwnedAdam(torch.optim.Adam):
    """What ``configure_optimizers`` hands to Lightning when the module is ``graphed``: it carries the parameter groups
    (learning rate, read by schedulers and copied into the captured step's device scalar) but its ``step`` applies
    nothing -- the Adam update already happened inside the replayed graph."""

    def step(self, closure=None):
        return None if closure is None else closure()


class PDETrainingModule(pl.LightningModule):
    def __init__(self, surrogate: PDESurrogate, loss: Callable, tstep: float, delta: float, env=None,
                 stransf: SampleTransform = None, undscaling: BatchTransform = None, tau: int = 5, tbtt: int = 10,
                 lr: float = 1e-03, lr_gamma: float = 1.0, step_size: int = 25, graphed: bool = None, **kwargs):
        super().__init__()
        self.graphed = (os.environ.get("PDECONTROL_GRAPHED", "0") == "1") if graphed is None else bool(graphed)
        # automatic optimization: forward and backward replayed as two captured graphs (PDECONTROL_SPLIT_GRAPHS=0 opts out)
        self.split_graphs = os.environ.get("PDECONTROL_SPLIT_GRAPHS", "1") != "0"

        if self.graphed:
            self.automatic_optimization = False   # Lightning: training_step owns backward + optimizer step
        self.surrogate, self.loss, self.tstep, self.delta, self.env = surrogate, loss, tstep, delta, env
        self.stransf = SampleTransform() if stransf is None else stransf
        self.undscaling = BatchTransform(Identity()) if undscaling is None else undscaling
        self.tau, self.tbtt, self.lr, self.lr_gamma, self.step_size = tau, tbtt, lr, lr_gamma, step_size
        if isinstance(surrogate, AutoRegPDESurrogate):
            self.training_mode = "delta"
        elif isinstance(surrogate, LatentAutoRegPDESurrogate):
            self.training_mode = "decoded"
        elif getattr(surrogate, "training_mode", None) in ("delta", "decoded"):
            self.training_mode = surrogate.training_mode      # e.g. the FNO surrogate of the Burgers path (f4)
        else:
            raise ValueError
        assert self.tbtt > self.tau, "Chunk size of TBTT must be larger than warm-up length."

    # -- helpers -----------------------------------------------------------------------------
    def _grid(self, n):
        """times / targets of an n-action chunk: k*tstep and (k+1)*tstep (CPU tensors)."""
        k = torch.arange(n)
        return self.tstep * k, self.tstep * (k + 1)

    def _full_rollout(self, states, actions) -> ModelRollout:
        times, targets = self._grid(actions.size(1))
        return self.surrogate.rollout(states=states[:, :self.tau], actions=actions, times=times, targets=targets,
                                      hidden=None)

    # -- training: truncated back-propagation through time ------------------------------------
    def tbptt_forward(self, states, actions):
        """Chunks of ``tbtt`` steps; chunk 0 warms up on the first ``tau`` true states, later chunks
        start from the previous chunk's last prediction with gradients cut (state and hidden)."""
        from pdecontrol.surrogates import ops
        if isinstance(self.surrogate, AutoRegPDESurrogate) and ops.use_fused_for(self.surrogate, states):
            # every chunk in a handful of launches, independent work on parallel streams (hipops._TBPTTFn); None: inputs
            # that require grad -> the generic chunk loop below (on the fused rollout)
            from pdecontrol.surrogates import hipops
            fused = hipops.fused_tbptt(self.surrogate, states, actions, self.tau, self.tbtt)
            if fused is not None:
                outputs, deltas, hidden, d_all = fused
                out = ModelRollout(outputs=outputs, deltas=deltas, hidden=tuple(h.detach() for h in hidden))
                out.time_major_deltas = d_all
                return [out]
        if states.is_cuda and ops.fused_enabled() and type(self.surrogate).__name__ == "FNOAutoRegSurrogate":
            # the FNO surrogate's whole TBPTT pass as one autograd node on the whole-network kernels (csrc/fno.hip); None:
            # a geometry they are not built for or inputs that require grad -> the generic chunk loop below
            from pdecontrol.surrogates import fno_hip
            fused = fno_hip.tbptt(self.surrogate, states, actions, self.tau, self.tbtt, self._grid)
            if fused is not None:
                outputs, deltas, d_all = fused
                out = ModelRollout(outputs=outputs, deltas=deltas, hidden=())
                out.time_major_deltas = d_all
                return [out]
        rollouts = []
        seed_states, hidden = None, None
        # inlatents are never read by the loss: skip the re-encoding unless the free-running transition reads it
        autoreg = (isinstance(self.surrogate, AutoRegPDESurrogate)
                   and not getattr(self.surrogate.transition_model, "reads_free_running_state", False))
        if autoreg:
            self.surrogate.reencode_predictions = False
        try:
            for c, achunk in enumerate(torch.split(actions, self.tbtt, dim=1)):
                if c == 0:
                    seed_states = states[:, :self.tbtt][:, :self.tau]
                times, targets = self._grid(achunk.size(1))
                out = self.surrogate.rollout(states=seed_states, actions=achunk, times=times, targets=targets,
                                             hidden=hidden)
                rollouts.append(out)
                seed_states = out.outputs[:, -1:].detach()
                out.hidden = hidden = tuple(h.detach() for h in out.hidden)
        finally:
            if autoreg:
                self.surrogate.reencode_predictions = True
        return rollouts

    def _fused_delta_loss(self, rollouts, states):
        """The loss section of training_step as one HIP launch, when the step ran on the fused kernels and the
        configuration is the controller's (delta mode, MSELoss(reduction="none"), affine undscaling)."""
        d_all = getattr(rollouts[0], "time_major_deltas", None) if len(rollouts) == 1 else None
        if d_all is None or self.training_mode != "delta":
            return None
        if not (isinstance(self.loss, torch.nn.MSELoss) and self.loss.reduction == "none"):
            return None
        from pdecontrol.surrogates import hipops
        consts = hipops.undscale_constants(self.undscaling)
        if consts is None or states.dtype != torch.float32 or states.shape[2] != 1:
            return None
        return hipops.fused_delta_loss(self.surrogate, d_all, states, self.delta, *consts)

    def _pipelined_training_step(self, batch):
        """The whole training pass -- forward, loss, backward, gradient reduction (+ Adam when the captured step lent its
        descriptors) -- in one hand-scheduled set of launches with the TBPTT chunks pipelined (``hipops.fused_tbptt_train``:
        chunk c's backward runs beside chunk c+1's forward).  No autograd and d loss = 1, so this is for the captured step
        only (``GraphedTBPTTStep``); returns None when the configuration is not the controller's (delta mode,
        MSELoss(reduction="none"), affine undscaling, fused kernels) or the sequence is a single chunk."""
        from pdecontrol.surrogates import ops
        states, actions, *_ = batch
        if not (isinstance(self.surrogate, AutoRegPDESurrogate) and ops.use_fused_for(self.surrogate, states)) or self.training_mode != "delta":
            return None
        if not (isinstance(self.loss, torch.nn.MSELoss) and self.loss.reduction == "none"):
            return None
        from pdecontrol.surrogates import hipops
        consts = hipops.undscale_constants(self.undscaling)
        if consts is None or states.dtype != torch.float32 or states.shape[2] != 1:
            return None
        with torch.no_grad():
            res = hipops.fused_tbptt_train(self.surrogate, states, actions, self.tau, self.tbtt, self.delta, *consts)
        if res is None:
            return None
        outputs, outdeltas, _hidden, loss, hsteploss, stats, deltas = res
        logged = {"Train Loss": loss, "Train Mean Delta Output": stats[0], "Train Std. Delta Output": stats[1],
                  "Train Mean Delta": stats[2], "Train Std. Delta": stats[3]}
        if torch.cuda.is_current_stream_capturing():
            self.__dict__["_graph_logged"] = logged
        else:
            for name, value in logged.items():
                self.log(name, value, on_step=False, on_epoch=True)
        return {"loss": loss, "hsteploss": hsteploss, "outputs": outputs, "actions": actions.detach(),
                "states": states.detach(), "outdeltas": outdeltas[:, :-1], "deltas": deltas}

    def _latent_constants(self):
        """(mean, std) of the decoded-mode kernels (``sur_tbptt_decoded_loss``, ``sur_latent_deltas``) when the configuration
        is the controller's for a latent surrogate: decoded mode, MSELoss(reduction="none"), and ``undscaling`` and the
        surrogate's ``dscaling.Inverse`` reducing to the SAME scalar constants (both wrap one Normalize, mbrl.py:168-171; the
        kernels apply one pair to the true and to the predicted deltas).  None otherwise."""
        if not isinstance(self.surrogate, LatentAutoRegPDESurrogate) or self.training_mode != "decoded":
            return None
        if not (isinstance(self.loss, torch.nn.MSELoss) and self.loss.reduction == "none"):
            return None
        from pdecontrol.surrogates import hipops
        consts = hipops.undscale_constants(self.undscaling)
        if consts is None or consts != hipops.latent_scale_constants(self.surrogate):
            return None
        return consts

    def _latent_training_step(self, batch):
        """``_pipelined_training_step`` for a latent surrogate on the fused kernels (``hipops.fused_latent_tbptt_train``): the
        whole decoded-mode pass -- forward, ``sur_tbptt_decoded_loss``, backward, gradient reduction (+ clip and Adam when the
        captured step lent its descriptors) -- without autograd and with d loss = 1, so for the captured step only
        (``GraphedTBPTTStep``).  None when ``_latent_constants`` is, the surrogate does not run on the latent kernels or the
        batch is not fp32 [B, T >= 2, 1, N]: then today's route runs."""
        from pdecontrol.surrogates import ops
        states, actions, *_ = batch
        consts = self._latent_constants()
        if consts is None or not (states.is_cuda and ops.use_fused_latent_for(self.surrogate, states)):
            return None
        if states.dtype != torch.float32 or states.shape[2] != 1 or actions.shape[1] < 2 or states.shape[1] != actions.shape[1]:
            return None
        from pdecontrol.surrogates import hipops
        with torch.no_grad():
            outputs, outdeltas, _hidden, loss, hsteploss, stats, deltas = hipops.fused_latent_tbptt_train(
                self.surrogate, states, actions, self.tau, self.tbtt, self.delta, *consts)
        logged = {"Train Loss": loss, "Train Mean Delta Output": stats[0], "Train Std. Delta Output": stats[1],
                  "Train Mean Delta": stats[2], "Train Std. Delta": stats[3]}
        if torch.cuda.is_current_stream_capturing():
            self.__dict__["_graph_logged"] = logged
        else:
            for name, value in logged.items():
                self.log(name, value, on_step=False, on_epoch=True)
        return {"loss": loss, "hsteploss": hsteploss, "outputs": outputs, "actions": actions.detach(),
                "states": states.detach(), "outdeltas": outdeltas, "deltas": deltas}

    def training_step(self, batch, bidx):
        states = batch[0]
        if self.graphed and states.is_cuda:
            return self._graphed_training_step(batch)
        if self.split_graphs and states.is_cuda and torch.is_grad_enabled():
            out = self._split_graph_training_step(batch)
            if out is not None:
                return out
        return self._eager_training_step(batch, bidx)

    def _frozen_parameters(self):
        """Names of the surrogate's parameters with requires_grad=False, apart from the initial hidden state (H0 / C0 are
        non-trainable by construction, transition.py)."""
        return [n for n, p in self.surrogate.named_parameters() if not p.requires_grad and not n.endswith((".H0", ".C0"))]

    def _split_graph_training_step(self, batch):
        """training_step under Lightning's automatic optimization as two replayed hipGraphs behind one autograd node
        (``graph_step.GraphedAutogradStep``): forward + loss now, backward + gradient reduction when the caller runs
        ``loss.backward()``.  None when the configuration is not the controller's (then the launch-by-launch path runs)."""
        from pdecontrol.surrogates import ops
        states, actions, *_ = batch
        if not (isinstance(self.surrogate, AutoRegPDESurrogate) and ops.use_fused_for(self.surrogate, states)) or self.training_mode != "delta":
            return None
        if not (isinstance(self.loss, torch.nn.MSELoss) and self.loss.reduction == "none"):
            return None
        from pdecontrol.surrogates import hipops
        if hipops.undscale_constants(self.undscaling) is None or states.dtype != torch.float32 or states.shape[2] != 1:
            return None
        if torch.cuda.is_current_stream_capturing():
            return None
        from pdecontrol.surrogates.graph_step import GraphedAutogradStep
        if states.requires_grad or actions.requires_grad:
            return None         # the captured step copies the batch into static buffers: no gradient reaches the inputs
        key = (tuple(states.shape), tuple(actions.shape))
        cache = self.__dict__.setdefault("_split_steps", {})
        step = cache.get(key)
        if step is None or not step.valid():
            if self._frozen_parameters():
                return None     # a frozen sub-module: the captured backward would still write its gradients
            step = cache[key] = GraphedAutogradStep(self, key[0], key[1])
        elif not step.all_trainable():
            return None
        out = step.forward(states, actions)
        for name, value in step.logged.items():
            self.log(name, value, on_step=False, on_epoch=True)
        return out

    def _eager_training_step(self, batch, bidx):
        states, actions, *_ = batch
        rollouts = self.tbptt_forward(states, actions)

        fused = self._fused_delta_loss(rollouts, states)
        if fused is not None:
            # loss, per-step loss, the four logged statistics and d loss / d deltas: one launch
            loss, hsteploss, stats, deltas = fused
            outputs, outdeltas = rollouts[0].outputs, rollouts[0].deltas[:, :-1]
            m_out, s_out, m_true, s_true = stats[0], stats[1], stats[2], stats[3]
        else:
            outputs = torch.cat([r.outputs for r in rollouts], dim=1)
            outdeltas = torch.cat([r.deltas for r in rollouts], dim=1)[:, :-1]
            deltas = self.undscaling(torch.diff(states, dim=1) / self.delta)
            if self.training_mode == "delta":
                loss = self.loss(outdeltas, deltas)
            else:
                decoded = torch.cat((states[:, :1], outputs[:, :-1]), dim=1)
                loss = self.loss(decoded, states)
            hsteploss = loss.mean(dim=(0, 2, 3))
            loss = loss.mean()
            m_out, s_out = outdeltas.detach().mean(), outdeltas.detach().std()
            m_true, s_true = deltas.detach().mean(), deltas.detach().std()

        logged = {"Train Loss": loss.detach(), "Train Mean Delta Output": m_out.detach(), "Train Std. Delta Output": s_out.detach(),
                  "Train Mean Delta": m_true.detach(), "Train Std. Delta": s_true.detach()}
        if torch.cuda.is_available() and states.is_cuda and torch.cuda.is_current_stream_capturing():
            self.__dict__["_graph_logged"] = logged     # static tensors of the captured step, logged at every replay
        else:
            for name, value in logged.items():
                self.log(name, value, on_step=False, on_epoch=True)

        return {"loss": loss, "hsteploss": hsteploss.detach(), "outputs": outputs.detach(),
                "actions": actions.detach(), "states": states.detach(), "outdeltas": outdeltas.detach(),
                "deltas": deltas.detach()}

    def fused_step(self, batch, lr=None, clip=None):
        """One optimizer step -- training_step + backward + Adam(lr) -- as ONE replayed HIP graph on static
        buffers (pdecontrol.surrogates.graph_step.GraphedTBPTTStep; a graph per batch shape, captured on first
        use; ONE Adam state and learning rate for all of them).  Returns training_step's dict; its tensors are
        overwritten by the next call.  CUDA only.  ``clip``: pl.Trainer's ``gradient_clip_val`` (``clip_grad_norm_`` between
        backward and Adam, inside the graph); None or <= 0 is no clipping and exactly the unclipped graph."""
        states, actions, *_ = batch
        return self.graphed_step_for(states.shape, actions.shape, lr=lr, clip=clip).step(states, actions, lr=lr)

    def graphed_step_for(self, states_shape, actions_shape, lr=None, clip=None):
        """The captured step of ``fused_step`` for one batch shape and one clip value (captured on first use, re-captured once
        it is no longer ``valid()``).  A caller that fills its static ``states`` / ``actions`` itself -- the surrogate-update
        phase's window gather -- replays it with ``step()``."""
        from pdecontrol.surrogates.graph_step import GraphedTBPTTStep, clip_value
        clip = clip_value(clip)
        key = (tuple(states_shape), tuple(actions_shape))
        if clip is not None:
            key += (clip,)
        cache = self.__dict__.setdefault("_graphed_steps", {})
        trained = self.__dict__.get("_graphed_trained")
        stale = key not in cache or not cache[key].valid()
        if stale or trained is None or not all(p.requires_grad for p in trained):
            # the captured step reduces and applies Adam over whole parameter sets: it would train frozen weights
            frozen = self._frozen_parameters()
            if frozen:
                raise RuntimeError(f"fused_step trains every parameter, but {len(frozen)} have requires_grad=False "
                                   f"({', '.join(frozen[:3])}{', ...' if len(frozen) > 3 else ''}): use training_step + "
                                   f"backward + the optimizer of configure_optimizers for a partly frozen surrogate")
            self.__dict__["_graphed_trained"] = [p for n, p in self.surrogate.named_parameters()
                                                 if not n.endswith((".H0", ".C0"))]
        if stale:
            # one process per GPU with an initialised process group: the captured step must exchange gradients
            # (forward/backward graph -> one flat-bucket all-reduce -> Adam graph), never train the ranks apart silently
            dist = torch.distributed
            distributed = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
            cache[key] = GraphedTBPTTStep(self, key[0], key[1], lr=lr, distributed=distributed, clip=clip)
        self.__dict__["_last_graphed_step"] = cache[key]
        return cache[key]

    def _graphed_training_step(self, batch):
        """training_step under Lightning's manual optimization: replay the graph with the learning rate of the
        optimizer Lightning holds (so StepLR and friends act on the captured Adam), log what training_step logs."""
        lr = None
        try:
            opts = self.optimizers()
            opt = opts[0] if isinstance(opts, (list, tuple)) else opts
            lr = float(opt.param_groups[0]["lr"])
        except Exception:   # no trainer attached (direct call): the module's own lr
            lr = None
        # manual optimization: Lightning's own clip never runs, so the shim Trainer leaves its gradient_clip_val here
        out = self.fused_step(batch, lr=lr, clip=self.__dict__.get("_trainer_gradient_clip_val"))
        if lr is not None:
            opt.step()      # bookkeeping only (_GraphOwnedAdam): keeps scheduler / Lightning step counters consistent
        # the five "Train ..." metrics of the step that was just replayed (static tensors of that captured step)
        for name, value in self.__dict__["_last_graphed_step"].logged.items():
            self.log(name, value, on_step=False, on_epoch=True)
        return out

    def on_train_epoch_end(self):
        # manual optimization: Lightning does not step the schedulers for us
        if self.graphed:
            try:
                scheds = self.lr_schedulers()
            except Exception:
                return
            if scheds is None:
                return
            for sch in (scheds if isinstance(scheds, (list, tuple)) else [scheds]):
                sch.step()

    # -- validation / test: one un-truncated rollout ------------------------------------------
    def _inverse_scaling(self, n, device):
        """[4, n] device coefficients of ``stransf.otransf.Inverse`` when it is an identity sensor and at most one
        ``ScaleTransform`` or one frozen, fitted ``Normalize`` (``False`` for the identity; None for anything else, e.g.
        a ``Normalize`` that is not frozen).  The host coefficients are worked out on every call (a few tiny CPU ops);
        they go up again only when their values change."""
        from pdecontrol.mbrl.recognition import Unrecognized, field_map
        try:
            fmap = field_map(self.stransf.otransf.Inverse, n, normalize=True)
        except (Unrecognized, NotImplementedError):
            return None
        if (fmap.start, fmap.stride, fmap.width) != (0, 1, n):
            return None
        if fmap.coef is None:
            return False
        cached = self.__dict__.get("_inv_coef")
        if cached is None or cached[0] != device or not torch.equal(cached[1], fmap.coef):
            cached = self.__dict__["_inv_coef"] = (device, fmap.coef, fmap.coef.to(device))
        return cached[2]

    def _fused_validation_loss(self, out, states, accum=None, outputs=True, fno=False):
        """The loss section of validation_step as one HIP launch (``sur_val_loss``), on the conditions of
        ``_fused_delta_loss`` plus a recognised ``stransf.otransf.Inverse``; None otherwise (then the torch ops run).
        ``accum`` / ``outputs``: the epoch accumulator and the switch of ``hipops.fused_val_loss`` (the surrogate-update
        phase keeps an epoch's sums on the device and needs neither ``deltas`` nor the decoded outputs).  ``fno``: the
        launch is also taken over the rollout of an ``FNOAutoRegSurrogate`` on the whole-network kernels, on the same
        conditions; only the surrogate-update phase asks for it, ``validation_step`` on such a module keeps the torch ops."""
        from pdecontrol.surrogates import hipops, ops
        if fno and type(self.surrogate).__name__ == "FNOAutoRegSurrogate":
            from pdecontrol.surrogates import fno_hip
            if not (states.is_cuda and ops.fused_enabled() and states.dim() == 4
                    and fno_hip.world_supported(self.surrogate, states.shape[3])):
                return None
            if self.training_mode != "delta" or not (isinstance(self.loss, torch.nn.MSELoss) and self.loss.reduction == "none"):
                return None
            consts = hipops.undscale_constants(self.undscaling)
        elif isinstance(self.surrogate, LatentAutoRegPDESurrogate):
            # the latent rollout under no_grad hands out its deltas as a view of time-major storage (sur_latent_deltas)
            consts = self._latent_constants()
            if consts is None or not (states.is_cuda and ops.use_fused_latent_for(self.surrogate, states)):
                return None
        else:
            if not (isinstance(self.surrogate, AutoRegPDESurrogate) and states.is_cuda and ops.use_fused_for(self.surrogate, states)):
                return None
            if self.training_mode != "delta" or not (isinstance(self.loss, torch.nn.MSELoss) and self.loss.reduction == "none"):
                return None
            consts = hipops.undscale_constants(self.undscaling)
        if consts is None or states.dtype != torch.float32 or states.shape[2] != 1 or states.shape[1] < 2:
            return None
        if tuple(out.outputs.shape) != tuple(states.shape) or tuple(out.deltas.shape) != tuple(states.shape):
            return None
        out_all, d_all = out.outputs.transpose(0, 1), out.deltas.transpose(0, 1)
        if not (out_all.is_contiguous() and d_all.is_contiguous()):
            return None             # not the time-major storage sur_chunk_forward wrote
        inv = self._inverse_scaling(states.shape[3], states.device)
        if inv is None:
            return None
        return hipops.fused_val_loss(self.surrogate, states, out_all, d_all, self.delta, *consts,
                                     inv if inv is not False else None, accum=accum, outputs=outputs)

    def validation_step(self, batch, bidx):
        states, actions, *_ = batch
        out = self._full_rollout(states, actions)
        fused = self._fused_validation_loss(out, states)
        if fused is not None:
            loss, hsteploss, scalars, deltas, decoded = fused
            self.log("Val. Delta Loss", scalars[1], on_step=False, on_epoch=True)
            self.log("Val. Scaled Loss", scalars[0], on_step=False, on_epoch=True)
            self.log("Val. Loss", loss, on_step=False, on_epoch=True)
            return {"loss": loss, "hsteploss": hsteploss, "outputs": decoded, "actions": actions.detach(),
                    "states": self.stransf.otransf.Inverse(states).detach(), "outdeltas": out.deltas[:, :-1].detach(),
                    "deltas": deltas}
        decoded = torch.cat((states[:, :1], out.outputs[:, :-1]), dim=1)  # IC-augmented prediction
        outdeltas = out.deltas[:, :-1]
        deltas = self.undscaling(torch.diff(states, dim=1) / self.delta)
        self.log("Val. Delta Loss", self.loss(outdeltas, deltas).detach().mean(), on_step=False, on_epoch=True)
        self.log("Val. Scaled Loss", self.loss(decoded, states).mean(), on_step=False, on_epoch=True)

        states = self.stransf.otransf.Inverse(states)
        decoded = self.stransf.otransf.Inverse(decoded)
        loss = self.loss(decoded, states)
        hsteploss = loss.detach().mean(dim=(0, 2, 3))
        loss = loss.mean()
        self.log("Val. Loss", loss, on_step=False, on_epoch=True)
        return {"loss": loss.detach(), "hsteploss": hsteploss.detach(), "outputs": decoded.detach(),
                "actions": actions.detach(), "states": states.detach(), "outdeltas": outdeltas.detach(),
                "deltas": deltas.detach()}

    # -- test: the metric section on the device (ks_eval_rows_device / ks_eval_fold_device for a KS env, bg_eval_rows /
    # bg_eval_fold for a Burgers env) ---------------------------------------------------------------------------------
    def _burgers_backend(self, states):
        """The ``BurgersBatchedVecEnv`` whose ``eval_rows_device`` / ``eval_fold_device`` take this batch: ``env`` itself
        or the vector env behind a ``BurgersEnv``, on the states' grid and device; None for any other env."""
        from pdegym.burgers import BurgersBatchedVecEnv, BurgersEnv
        if not isinstance(self.env, (BurgersEnv, BurgersBatchedVecEnv)) or self.env.N != states.shape[3]:
            return None
        vec = self.env.vec if isinstance(self.env, BurgersEnv) else self.env
        return vec if vec.device == states.device else None

    def _burgers_objective(self):
        """The objective of a Burgers env (either class), None for any other env."""
        from pdegym.burgers import BurgersBatchedVecEnv, BurgersEnv
        return self.env.objective if isinstance(self.env, (BurgersEnv, BurgersBatchedVecEnv)) else None

    def _test_kernel_plan(self, states, out):
        """A ``_TestPlan`` -- (kind, device coefficients or None) of ``stransf.otransf.Inverse``, the backend that launches
        (the KS env, whose reward handle does, or the Burgers vector env), its row-stat and table counts and its table
        names -- when the metric section of ``test_step`` runs as the two HIP launches; otherwise None, with a one-time
        notice that says why."""
        from pdecontrol.mbrl.recognition import Unrecognized, inverse_map, notice
        from pdecontrol.surrogates import ops
        from pdegym.kuramoto import KuramotoSivashinskyEnv
        sentence = "test_step computes its metrics with torch on the host: %s"
        objective = self._burgers_objective()
        if objective not in (None, "l2control"):
            # bg_eval_rows writes the l2control reward of both rows; the host lines call the env's own reward_func
            notice(sentence, f"the Burgers env's {objective} objective (the reward columns of bg_eval_rows are l2control's)",
                   expected=True)
            return None
        if not states.is_cuda:
            notice(sentence, "the batch is in host memory", expected=True)
            return None
        if not ops.fused_enabled():
            notice(sentence, "the fused kernels are switched off", expected=True)
            return None
        if states.dtype != torch.float32 or states.dim() != 4 or states.shape[2] != 1:
            notice(sentence, f"states of shape {tuple(states.shape)} in {states.dtype} are not fp32 [B, T, 1, N]")
            return None
        burgers = self._burgers_backend(states)
        if burgers is None and (not isinstance(self.env, KuramotoSivashinskyEnv) or self.env.N != states.shape[3]):
            if type(self.env).__name__ in ("BurgersEnv", "BurgersBatchedVecEnv"):
                notice(sentence, f"the Burgers env is not on the states' grid of {states.shape[3]} points and on {states.device}")
            else:
                notice(sentence, f"the env is no KuramotoSivashinskyEnv on the states' grid of {states.shape[3]} points")
            return None
        pred = out.outputs
        if pred.dtype != torch.float32 or not pred.is_cuda or tuple(pred.shape) != tuple(states.shape):
            notice(sentence, f"the rollout returned {tuple(pred.shape)} in {pred.dtype} for states {tuple(states.shape)}")
            return None
        try:
            kind, coef = inverse_map(self.stransf.otransf.Inverse, states.shape[3])
        except (Unrecognized, NotImplementedError) as reason:
            notice(sentence, f"the inverse observation transform is {reason}")
            return None
        if burgers is not None:
            from pdegym.burgers import _hip as bg
            backend = ("burgers", burgers, bg.EVAL_ROW_STATS, bg.EVAL_TABLES, bg.EVAL_TABLE_NAMES)
        else:
            import kspde
            backend = ("ks", self.env, kspde.EVAL_ROW_STATS, kspde.EVAL_TABLES, kspde.EVAL_TABLE_NAMES)
        if coef is None:
            return _TestPlan(kind, None, *backend)
        cached = self.__dict__.get("_test_inv_coef")
        if cached is None or cached[0] != states.device or cached[1].shape != coef.shape or not torch.equal(cached[1], coef):
            cached = self.__dict__["_test_inv_coef"] = (states.device, coef, coef.to(states.device))
        return _TestPlan(kind, cached[2], *backend)

    @staticmethod
    def _rows(field):
        """``field`` [B, T, 1, N] as ks_eval_batch names it: (tensor, batch stride, time stride) with unit-stride rows
        that do not overlap -- the tensor itself, batch- or time-major, or a contiguous copy."""
        n = field.shape[3]
        if field.stride(3) != 1 or field.stride(0) < n or field.stride(1) < n:
            field = field.contiguous()
        return field, field.stride(0), field.stride(1)

    def _test_metrics_device(self, states, actions, out, plan, accum=None, keep=True):
        """The metric section of ``test_step`` for one batch on the device: two launches of the plan's backend (the KS
        env's reward handle, or the Burgers vector env) on torch's current stream.  Returns (tables fp64
        [1 + plan.tables T], inverse-scaled states, IC-augmented inverse-scaled outputs), the last two None without
        ``keep``; ``accum`` is the epoch accumulator of the fold launch: fp64, at least ``1 + plan.tables T`` long
        (``test_surrogate`` sizes it for the KS backend's 25 tables; a backend with fewer writes the front of it and
        ``_named_tables`` reads no further)."""
        kind, coef = plan.kind, plan.coef
        b, t, _, n = states.shape
        dev = states.device
        if accum is not None and (accum.dtype != torch.float64 or accum.numel() < 1 + plan.tables * t):
            raise ValueError(f"the epoch accumulator holds {accum.numel()} {accum.dtype} values, the fold launch writes "
                             f"{1 + plan.tables * t} doubles")
        self.__dict__["_test_table_names"] = plan.names      # what _named_tables names an epoch's accumulator by
        truth, truth_bs, truth_ts = self._rows(states.detach())
        pred, pred_bs, pred_ts = self._rows(out.outputs.detach())
        truth_out = torch.empty((b, t, 1, n), dtype=torch.float32, device=dev) if keep else None
        pred_out = torch.empty((b, t, 1, n), dtype=torch.float32, device=dev) if keep else None
        rowstats = torch.empty((b, t, plan.row_stats), dtype=torch.float64, device=dev)
        tables = torch.empty(1 + plan.tables * t, dtype=torch.float64, device=dev)
        ptr = lambda v: None if v is None else v.data_ptr()
        d_accum = 0 if accum is None else accum.data_ptr()
        # pred_shift: the prediction of step 0 is the initial condition, of step t >= 1 the rollout's output t - 1
        if plan.family == "burgers":
            from pdegym.burgers import _hip as bg
            desc = bg.EvalBatch(ptr(truth), truth_bs, truth_ts, ptr(pred), pred_bs, pred_ts, 1, kind, ptr(coef),
                                ptr(truth_out), ptr(pred_out))
            plan.backend.eval_rows_device(desc, b, t, rowstats.data_ptr())
            plan.backend.eval_fold_device(rowstats.data_ptr(), b, t, tables.data_ptr(), d_accum)
            return tables, truth_out, pred_out
        import kspde
        objective = self.env.step_objective
        phi = None
        if objective == "dissipation":
            flat = actions.reshape(b * t, *actions.shape[2:])
            phi = BatchTransform(self.env.forcing)(self.stransf.atransf.Inverse(flat))
            phi = phi.to(torch.float32).reshape(b * t, n).contiguous()
        desc = kspde.ks_eval_batch(ptr(truth), truth_bs, truth_ts, ptr(pred), pred_bs, pred_ts, 1, ptr(phi), kind, ptr(coef),
                                   ptr(truth_out), ptr(pred_out))
        handle = plan.backend._reward_handle(dev)
        handle.eval_rows_device(objective, desc, b, t, rowstats.data_ptr())
        handle.eval_fold_device(rowstats.data_ptr(), b, t, tables.data_ptr(), d_accum)
        return tables, truth_out, pred_out

    def _named_tables(self, values, steps, names=None):
        """fp64 host values of the fold launch (the MSE, then ``[T]`` per table; anything behind the last table is not
        read) as the reference's keys.  ``names``: the plan's; None: those of the plan ``_test_metrics_device`` last ran,
        which is how ``test_surrogate`` names its accumulator at the end of an epoch."""
        if names is None:
            names = self.__dict__.get("_test_table_names")
            if names is None:
                import kspde
                names = kspde.EVAL_TABLE_NAMES
        assert len(values) >= 1 + len(names) * steps, (len(values), len(names), steps)
        named = {"MSE": values[0]}
        for k, name in enumerate(names):
            named[name] = values[1 + k * steps:1 + (k + 1) * steps]
        return named

    def test_step(self, batch, bidx):
        states, actions, *_ = batch
        out = self._full_rollout(states, actions)
        plan = self._test_kernel_plan(states, out)
        if plan is None:
            self.last_test_tier = "torch"
            return self._test_step_host(states, actions, out)
        self.last_test_tier = "kernel"
        tables, truth, pred = self._test_metrics_device(states, actions, out, plan)
        named = self._named_tables(tables.cpu().numpy(), states.shape[1], plan.names)
        data = {name: np.asarray(value, dtype=np.float32) for name, value in named.items()}
        data.update({"states": truth.cpu().numpy(), "outputs": pred.cpu().numpy(), "actions": actions.detach().cpu().numpy()})
        return data

    def _test_step_host(self, states, actions, out):
        """The metric section of ``test_step`` in torch on the host, line for line the reference's."""
        outputs = torch.cat((states[:, :1], out.outputs[:, :-1]), dim=1)
        states = self.stransf.otransf.Inverse(states).detach().cpu()
        outputs = self.stransf.otransf.Inverse(outputs).detach().cpu()
        actions = actions.detach().cpu()

        def norms(a, b, dims, p):
            return torch.norm(a - b, p=p, dim=dims[0]), torch.norm(b, p=p, dim=dims[0])

        err1, ref1 = norms(outputs, states, (3,), 1)
        err2, ref2 = norms(outputs, states, (3,), 2)
        tm = lambda v: v.mean(dim=(0, 2)).numpy()
        data = {"MSE": self.loss(outputs, states).mean().numpy(), "l1_loss": tm(err1), "l2_loss": tm(err2),
                "l1_loss_scaled": tm(err1 / ref1), "l2_loss_scaled": tm(err2 / ref2),
                "nrmse": tm(err2 ** 2 / ref2 ** 2)}

        # reward estimates on true vs predicted states (env.forcing / env.reward_func, per sample)
        b, t, ac, ah = actions.shape
        _, _, sc, sh = states.shape
        flat = lambda v, c, h: v.reshape(b * t, c, h)
        phi = BatchTransform(self.env.forcing)(self.stransf.atransf.Inverse(flat(actions, ac, ah)))
        rew = lambda vals: torch.stack([torch.as_tensor(self.env.reward_func(v, p)) for v, p in zip(vals, phi)],
                                       dim=0).reshape(b, t)
        rews, pred_rews = rew(flat(states, sc, sh)), rew(flat(outputs, sc, sh))
        e1, r1 = torch.norm(rews - pred_rews, p=1, dim=0), torch.norm(rews, p=1, dim=0)
        e2, r2 = torch.norm(rews - pred_rews, p=2, dim=0), torch.norm(rews, p=2, dim=0)
        data.update({"l1_loss_rews": e1.numpy(), "l2_loss_rews": e2.numpy(), "l1_loss_scaled_rews": (e1 / r1).numpy(),
                     "l2_loss_scaled_rews": (e2 / r2).numpy(), "nrmse_rews": (e2 ** 2 / r2 ** 2).numpy()})

        # spatial derivatives (env.rhs) of true vs predicted states.  The reference calls env.rhs once per sample
        # (training.py:237-245); the HIP rhs hook is row-parallel, so all B*T samples go in ONE call (same values)
        def derivatives(vals):
            _, each = self.env.rhs(vals.numpy(), phi.numpy())                  # (ux, uxx, uxxxx); (ux, uxx) on Burgers
            d = torch.as_tensor(np.stack(list(each), axis=1))                  # [B*T, 3, C, H]
            return d.reshape(b, t, *d.shape[1:])
        dv, pdv = derivatives(flat(states, sc, sh)), derivatives(flat(outputs, sc, sh))
        d1, n1 = torch.norm(dv - pdv, p=1, dim=4), torch.norm(dv, p=1, dim=4)
        d2, n2 = torch.norm(dv - pdv, p=2, dim=4), torch.norm(dv, p=2, dim=4)
        dm = lambda v: v.mean(dim=(0, 3))
        named = {"l1_loss_derivs": dm(d1), "l2_loss_derivs": dm(d2), "l1_loss_scaled_derivs": dm(d1 / n1),
                 "l2_loss_scaled_derivs": dm(d2 / n2), "nrms_derivs": dm(d2 ** 2 / n2 ** 2)}
        for name, table in named.items():
            for idx, column in enumerate(table.T):
                data[f"{name}-derivative-{idx}"] = column
        data.update({"states": states.numpy(), "outputs": outputs.numpy(), "actions": actions.numpy()})
        return data

    def _fused_eager(self):
        from pdecontrol.surrogates import hipops, ops
        return ops.fused_enabled() and hipops.fused_supported(self.surrogate)

    def configure_optimizers(self):
        params = list(self.surrogate.parameters())
        # same update rule as the reference's Adam; on a GPU as one multi-tensor kernel instead of ~6 per parameter
        on_gpu = bool(params) and params[0].is_cuda
        if self.graphed and on_gpu:
            optimizer = _GraphOwnedAdam(params, lr=self.lr)
        elif on_gpu and self._fused_eager() and not self._frozen_parameters():
            # the whole Adam update as ONE launch over the fused packs' flat state (same rule as torch.optim.Adam)
            from pdecontrol.surrogates import hipops
            optimizer = hipops.PackAdam(self.surrogate, lr=self.lr)
        else:
            # (a partly frozen surrogate lands here: PackAdam's single launch would move the frozen weights of a pack)
            extra = {"fused": True} if on_gpu else {}
            optimizer = torch.optim.Adam(params, lr=self.lr, **extra)
        scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=self.step_size, gamma=self.lr_gamma)
        return [optimizer], [{"scheduler": scheduler, "interval": "epoch"}]
