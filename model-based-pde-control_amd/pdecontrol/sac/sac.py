"""``SAC(observation_space, action_space, config)``: the reference's soft actor-critic agent (pdecontrol/sac/sac.py) with
its names, signatures and, on the CPU, its arithmetic and order of random draws bit for bit.

Construction order is the reference's (critic, critic target, optional ``log_alpha``, policy), so a torch seed gives its
initial weights.  Reference quirks kept as they are:

* ``select_action(state, deterministic=False)`` accepts ``deterministic`` and ignores it: it always samples.
* ``update(batch)`` takes the 7-tuple ``(obs, actions, nxtobs, rewards, terminated, truncated, steps)`` and squeezes
  ``obs``, ``actions`` and ``nxtobs`` on axis 1.
* A ``terminated`` sample anywhere in the batch is an ``AssertionError``: the time-limit ``truncated`` flag is ignored and
  real terminations are not expected from the PDE envs.

One deliberate difference: the reference's ``update`` never moves the batch and so cannot run with ``config.cuda``; here
the batch is moved to ``self.device`` (``cuda`` when ``config.cuda`` is set, overridden by an optional ``config.device``).

Logging: ``logger`` is an optional callable with ``wandb.log``'s signature; the default is ``wandb.log`` when ``wandb``
imports, else none.  An attached logger receives the reference's calls (``{"Pol. Rew. Mean": ...}`` with ``commit=False``,
then the four ``SAC/...`` scalars); without one no statistic is fetched to the host.

On a CUDA device ``act`` and ``update`` run on the kernels of csrc/sac.hip (pdecontrol/sac/sac_hip.py says when, and
what happens otherwise); ``critic_optim``, ``policy_optim`` and ``alpha_optim`` stay ``torch.optim.Adam`` objects on every
path and hold the moments the kernels update.
"""
from argparse import Namespace

import torch
import torch.nn.functional as F
from torch.optim import Adam

from pdecontrol.sac.policies import GaussianPolicy, QNetwork, draw_noise
from pdecontrol.sac.utils import hard_update, soft_update

_UNSET = object()


def _default_logger():
    try:
        import wandb
    except ImportError:
        return None
    return wandb.log


class SAC(object):
    def __init__(self, observation_space, action_space, config: Namespace, logger=_UNSET):
        self.gamma = config.gamma
        self.tau = config.tau
        self.alpha = config.alpha
        self.policy_type = config.policy
        self.target_update_interval = config.target_update_interval
        self.automatic_entropy_tuning = config.automatic_entropy_tuning
        self.logger = _default_logger() if logger is _UNSET else logger

        self.device = torch.device("cuda" if config.cuda else "cpu")
        if getattr(config, "device", None) is not None:
            self.device = torch.device(config.device)

        ochannels, oheight = observation_space.shape
        achannels, aheight = action_space.shape
        sizes = (ochannels, oheight, achannels, aheight, config.hidden_size)

        self.critic = QNetwork(*sizes).to(device=self.device)
        self.critic_optim = Adam(self.critic.parameters(), lr=config.lr)
        self.critic_target = QNetwork(*sizes).to(self.device)
        hard_update(self.critic_target, self.critic)
        self.updates = 0

        if self.automatic_entropy_tuning is True:
            # target entropy = -dim(A)
            self.target_entropy = -torch.prod(torch.Tensor(action_space.shape).to(self.device)).item()
            self.log_alpha = torch.zeros(1, requires_grad=True, device=self.device)
            self.alpha_optim = Adam([self.log_alpha], lr=config.lr)

        self.policy = GaussianPolicy(*sizes, action_space).to(self.device)
        self.policy_optim = Adam(self.policy.parameters(), lr=config.lr)

        self._fused = None               # sac_hip.FusedSAC, created at the first fused call
        self._terminated_seen = None     # device count of terminated samples in device-resident batches (torch spelling)

    # ------------------------------------------------------------------------------------------------------------------
    # acting
    # ------------------------------------------------------------------------------------------------------------------
    def select_action(self, state, deterministic=False):
        """numpy in, numpy out.  ``deterministic`` is accepted and ignored, as in the reference: the action is sampled."""
        state = torch.FloatTensor(state).to(self.device)
        return self.act(state).detach().cpu().numpy()

    def act(self, obs, deterministic=False):
        """Device tensor [B, channels, height] in, action [B, achannels, aheight] out, no host copy.  Here ``deterministic``
        does select the mean action ``tanh(mean) * scale + bias``.  On the kernels this is one launch."""
        fused = self._fused_for(obs)
        if fused is None:
            with torch.no_grad():
                action, _, mean = self.policy.sample(obs)
            return mean if deterministic else action
        B = obs.shape[0]
        shape = (B, self.policy.achannels, self.policy.aheight)
        noise = None if deterministic else draw_noise(torch.empty(shape, dtype=torch.float32, device=obs.device))
        action, _, _ = fused.forward(obs.reshape(B, -1).contiguous(), None if noise is None else noise.reshape(B, -1))
        return action.reshape(shape)

    def _fused_for(self, obs=None, batch=None):
        if self.device.type != "cuda":
            return None
        from pdecontrol.sac import sac_hip
        if not sac_hip.use_kernels(self, obs, batch):
            return None
        if self._fused is None:
            self._fused = sac_hip.FusedSAC(self)
        return self._fused

    # ------------------------------------------------------------------------------------------------------------------
    # training
    # ------------------------------------------------------------------------------------------------------------------
    def _prepare(self, batch):
        """The 7-tuple on ``self.device``: squeezed obs / actions / nxtobs, rewards, float terminated.  A batch that
        arrives on the CPU has its ``terminated`` flags checked here, on the host."""
        obs, actions, nxtobs, rewards, terminated, truncated, steps = batch
        obs, actions, nxtobs = (t.squeeze(1) for t in (obs, actions, nxtobs))
        on_host = terminated.device.type == "cpu"
        if on_host:
            assert not bool(terminated.any()), "terminated samples are not expected (the reference asserts the same)"
        dev = self.device
        obs, actions, nxtobs, rewards = (t.to(dev) for t in (obs, actions, nxtobs, rewards))
        terminated = terminated.to(device=dev, dtype=torch.float32)
        return obs, actions, nxtobs, rewards, terminated, on_host

    def update(self, batch, noise=None):
        """One reference update: critic step, policy step against the updated critic, optional entropy-coefficient step,
        Polyak average of the target every ``target_update_interval`` updates.  ``noise`` (not in the reference) is an
        optional pair of standard-normal tensors shaped like the squeezed actions, for the next-state and the current-state
        sample; None draws them as ``Normal.rsample`` does."""
        obs, actions, nxtobs, rewards, terminated, on_host = self._prepare(batch)
        fused = self._fused_for(obs, (actions, rewards, terminated))
        if noise is not None:
            noise = tuple(n.to(device=obs.device, dtype=obs.dtype).reshape(actions.shape) for n in noise)
        if fused is None:
            return self._update_torch(obs, actions, nxtobs, rewards, terminated, on_host, noise or (None, None))
        B = obs.shape[0]
        # the two draws of the torch spelling's rsample calls: same call, shape and order
        noise_next, noise_cur = noise if noise is not None else (draw_noise(actions), draw_noise(actions))
        flat = lambda t: t.reshape(B, -1).contiguous()
        fused.update(flat(obs), flat(actions), flat(nxtobs), rewards.reshape(B).contiguous(), terminated.reshape(B).contiguous(),
                     flat(noise_next), flat(noise_cur))
        if self.logger is not None:
            self._log_stats(fused.stats.tolist())

    def _log_stats(self, stats, check=True):
        if check:
            self._check_terminated(stats[5])
        self.logger({"Pol. Rew. Mean": stats[4]}, commit=False)
        self.logger({"SAC/Qloss": stats[0], "SAC/PolicyLoss": stats[1], "SAC/entropy_loss": stats[2], "SAC/alpha_loss": stats[3]})

    @staticmethod
    def _check_terminated(count):
        assert count == 0, "terminated samples are not expected (the reference asserts the same)"

    def _update_torch(self, obs, actions, nxtobs, rewards, terminated, on_host, noise=(None, None)):
        """The torch spelling: the reference's operations in the reference's order."""
        log = self.logger
        if log is not None:
            log({"Pol. Rew. Mean": torch.mean(rewards)}, commit=False)
        if not on_host:      # a device-resident batch: count on the device, raise at the next fetch of the statistics
            count = (terminated != 0).sum()
            self._terminated_seen = count if self._terminated_seen is None else self._terminated_seen + count
        mask_batch = 1.0 - terminated

        with torch.no_grad():
            next_action, next_log_pi, _ = self.policy.sample(nxtobs, noise[0])
            q1_next, q2_next = self.critic_target(nxtobs, next_action)
            min_q_next = torch.min(q1_next, q2_next) - self.alpha * next_log_pi
            next_q_value = rewards + mask_batch * self.gamma * (min_q_next)

        qf1, qf2 = self.critic(obs, actions)
        qf1_loss = F.mse_loss(qf1, next_q_value)
        qf2_loss = F.mse_loss(qf2, next_q_value)
        qf_loss = qf1_loss + qf2_loss
        self.critic_optim.zero_grad()
        qf_loss.backward()
        self.critic_optim.step()

        pi, log_pi, _ = self.policy.sample(obs, noise[1])
        qf1_pi, qf2_pi = self.critic(obs, pi)
        min_qf_pi = torch.min(qf1_pi, qf2_pi)
        policy_loss = ((self.alpha * log_pi) - min_qf_pi).mean()
        self.policy_optim.zero_grad()
        policy_loss.backward()
        self.policy_optim.step()

        if self.automatic_entropy_tuning:
            alpha_loss = -(self.log_alpha * (log_pi + self.target_entropy).detach()).mean()
            self.alpha_optim.zero_grad()
            alpha_loss.backward()
            self.alpha_optim.step()
            self.alpha = self.log_alpha.exp()
            alpha_tlogs = self.alpha.clone()
        else:
            alpha_loss = torch.tensor(0.0).to(self.device)
            alpha_tlogs = torch.tensor(self.alpha)

        if self.updates % self.target_update_interval == 0:
            soft_update(self.critic_target, self.critic, self.tau)
        self.updates += 1

        if log is not None:
            if self._terminated_seen is not None:
                seen, self._terminated_seen = self._terminated_seen, None
                self._check_terminated(int(seen))
            log({"SAC/Qloss": qf_loss.item(), "SAC/PolicyLoss": policy_loss.item(), "SAC/entropy_loss": alpha_loss.item(),
                 "SAC/alpha_loss": alpha_tlogs.item()})

    def update_many(self, batches):
        """``update`` for every batch of a sequence of same-shaped batches, or of a 7-tuple of stacked tensors with a
        leading update axis.  The torch spelling is the plain loop.  On the kernels one update is captured as a hipGraph at
        first use and replayed per batch from static input buffers; the noise is drawn outside the graph with the calls of
        ``update``, and the statistics are fetched once at the end (only if a logger is attached).  The results are those
        of calling ``update`` per batch."""
        if isinstance(batches, tuple) and len(batches) == 7 and isinstance(batches[0], torch.Tensor):
            batches = [tuple(t[i] for t in batches) for i in range(batches[0].shape[0])]
        batches = list(batches)
        if not batches:
            return
        first = self._prepare(batches[0])
        fused = self._fused_for(first[0], (first[1], first[3], first[4]))
        if fused is None:
            for batch in batches:
                self.update(batch)
            return
        B = first[0].shape[0]
        graph = fused.graph_for((B, tuple(first[1].shape[1:])))
        history = self._stats_history(len(batches))
        for i, batch in enumerate(batches):
            obs, actions, nxtobs, rewards, terminated, _ = first if i == 0 else self._prepare(batch)
            assert obs.shape[0] == B and tuple(actions.shape[1:]) == tuple(graph.noise_cur.shape[1:]), "batches must share a shape"
            srcs = (obs, actions, nxtobs, rewards, terminated)
            fill = lambda: [dst.copy_(src.reshape(dst.shape), non_blocking=True) for dst, src in zip(graph.inputs[:5], srcs)]
            self._replay_update(fused, graph, fill, None if history is None else history[i])
        self._log_history(history)

    def _stats_history(self, n):
        """Device rows for the statistics of ``n`` captured updates, or None without a logger (nothing is fetched then)."""
        return torch.zeros((n, 8), dtype=torch.float32, device=self.device) if self.logger is not None else None

    @staticmethod
    def _replay_update(fused, graph, fill, stats_row=None):
        """One update on the captured graph.  ``fill()`` enqueues whatever writes the graph's five static batch buffers
        (``update_many``: five copies; the policy-update phase: one ``rp_gather`` launch); the noise is drawn outside the
        graph with the calls of ``update``, and the statistics are kept in ``stats_row`` on the device."""
        fused.sync_in()
        fill()
        graph.noise_next.normal_()
        graph.noise_cur.normal_()
        graph.graph.replay()
        fused.sync_out()
        if stats_row is not None:
            stats_row.copy_(fused.stats)

    def _log_history(self, history):
        """The one fetch at the end of a run of captured updates: the terminated check, then the reference's log calls."""
        if history is not None:
            rows = history.tolist()
            self._check_terminated(sum(r[5] for r in rows))
            for row in rows:
                self._log_stats(row, check=False)
