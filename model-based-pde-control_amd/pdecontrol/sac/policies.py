"""Networks of the SAC agent under the reference's names (pdecontrol/sac/policies.py).  Module trees, attribute names and
construction order are the reference's, so a torch seed gives its initial weights and ``state_dict`` keys are
``linear1 ... linear6``, ``mean_linear`` and ``log_std_linear``.  Observations are [B, channels, height] and are flattened;
actions likewise."""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.distributions import Normal

LOG_SIG_MAX = 2
LOG_SIG_MIN = -20
epsilon = 1e-6


def weights_init_(m):
    """Xavier-uniform weights (gain 1) and zero biases on every Linear."""
    if isinstance(m, nn.Linear):
        torch.nn.init.xavier_uniform_(m.weight, gain=1)
        torch.nn.init.constant_(m.bias, 0)


def _flat(x):
    return x.reshape(x.shape[0], x.shape[1] * x.shape[2])


class ValueNetwork(nn.Module):
    """State value V(s): obs -> hidden -> hidden -> 1."""

    def __init__(self, ochannels, oheight, hidden_dim):
        super().__init__()
        self.linear1 = nn.Linear(ochannels * oheight, hidden_dim)
        self.linear2 = nn.Linear(hidden_dim, hidden_dim)
        self.linear3 = nn.Linear(hidden_dim, 1)
        self.apply(weights_init_)

    def forward(self, state):
        x = F.relu(self.linear1(_flat(state)))
        x = F.relu(self.linear2(x))
        return self.linear3(x)


class QNetwork(nn.Module):
    """Twin action values Q1, Q2 of (obs | action): linear1-3 are Q1, linear4-6 are Q2."""

    def __init__(self, ochannels, oheight, achannels, aheight, hidden_dim):
        super().__init__()
        self.achannels, self.aheight = achannels, aheight
        width = ochannels * oheight + achannels * aheight
        self.linear1 = nn.Linear(width, hidden_dim)
        self.linear2 = nn.Linear(hidden_dim, hidden_dim)
        self.linear3 = nn.Linear(hidden_dim, 1)
        self.linear4 = nn.Linear(width, hidden_dim)
        self.linear5 = nn.Linear(hidden_dim, hidden_dim)
        self.linear6 = nn.Linear(hidden_dim, 1)
        self.apply(weights_init_)

    def forward(self, state, action):
        xu = torch.cat([_flat(state), _flat(action)], 1)
        q1 = self.linear3(F.relu(self.linear2(F.relu(self.linear1(xu)))))
        q2 = self.linear6(F.relu(self.linear5(F.relu(self.linear4(xu)))))
        return q1, q2


class GaussianPolicy(nn.Module):
    """Tanh-squashed diagonal Gaussian policy.  ``action_scale`` / ``action_bias`` are plain tensors (not buffers, as in
    the reference: they are not part of ``state_dict``) that ``to`` moves along."""

    def __init__(self, ochannels, oheight, achannels, aheight, hidden_dim, action_space=None):
        super().__init__()
        self.achannels, self.aheight = achannels, aheight
        self.linear1 = nn.Linear(ochannels * oheight, hidden_dim)
        self.linear2 = nn.Linear(hidden_dim, hidden_dim)
        self.mean_linear = nn.Linear(hidden_dim, achannels * aheight)
        self.log_std_linear = nn.Linear(hidden_dim, achannels * aheight)
        self.apply(weights_init_)
        if action_space is None:
            self.action_scale = torch.tensor(1.0)
            self.action_bias = torch.tensor(0.0)
        else:
            self.action_scale = torch.FloatTensor((action_space.high - action_space.low) / 2.0)
            self.action_bias = torch.FloatTensor((action_space.high + action_space.low) / 2.0)

    def forward(self, state):
        bsize = state.shape[0]
        x = F.relu(self.linear1(_flat(state)))
        x = F.relu(self.linear2(x))
        mean = self.mean_linear(x).reshape(bsize, self.achannels, self.aheight)
        log_std = self.log_std_linear(x).reshape(bsize, self.achannels, self.aheight)
        return mean, torch.clamp(log_std, min=LOG_SIG_MIN, max=LOG_SIG_MAX)

    def sample(self, state, noise=None):
        """(action, log-probability [B, 1] summed over channel and height, tanh(mean) rescaled).  ``noise`` is the
        standard-normal draw of the reparameterisation; None draws it exactly as ``Normal.rsample`` does."""
        mean, log_std = self.forward(state)
        normal = Normal(mean, log_std.exp())
        if noise is None:
            noise = draw_noise(mean)
        x_t = normal.loc + noise * normal.scale
        y_t = torch.tanh(x_t)
        action = y_t * self.action_scale + self.action_bias
        log_prob = normal.log_prob(x_t)
        log_prob -= torch.log(self.action_scale * (1 - y_t.pow(2)) + epsilon)
        log_prob = log_prob.sum((1, 2)).reshape(-1, 1)
        mean = torch.tanh(mean) * self.action_scale + self.action_bias
        return action, log_prob, mean

    def to(self, device):
        self.action_scale = self.action_scale.to(device)
        self.action_bias = self.action_bias.to(device)
        return super().to(device)


def draw_noise(like):
    """The standard-normal tensor ``Normal(like, .).rsample()`` draws: same call, shape, dtype and device, hence the same
    values at a given generator state."""
    return torch.empty(like.shape, dtype=like.dtype, device=like.device).normal_()
