"""Host helpers of the controller (reference ``pdecontrol/mbrl/utils.py``): array conversions and the two scripted agents,
whose actions do not depend on the observation.  ``collect`` runs exactly these two classes (not subclasses, not
same-named classes) on its scripted kernel tier (pdecontrol/mbrl/collection_phase.py)."""
import numpy as np
import torch


def totorch(array):
    if not isinstance(array, torch.Tensor):
        return torch.FloatTensor(array)
    return array


def tonumpy(tensor):
    if not isinstance(tensor, np.ndarray):
        return tensor.cpu().numpy()
    return tensor


class RandomAgent:
    """Uniform draws from ``action_space`` (the controller's warm-up agent)."""

    def __init__(self, action_space):
        self.action_space = action_space

    def select_action(self, *args, **kwargs):
        return self.action_space.sample()


class ActionRepeatAgent:
    """Replays a table ``[E, steps, 1, A]`` column by column (the controller's surrogate evaluation)."""

    def __init__(self, actions):
        self.actions = actions
        assert self.actions.ndim == 4
        self.nstep = 0

    def select_action(self, *args, **kwargs):
        action = self.actions[:, self.nstep, :, :]
        self.nstep += 1
        return action
