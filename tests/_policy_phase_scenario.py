"""Shared pieces of the policy-phase tests (tests/test_policy_phase_host.py, tests/test_policy_phase_gpu.py) and of
tools/policy_phase_bench.py: two scripted ``ExperienceReplay``s of different size with ragged episodes (the scripted
stepping of tests/_dataset_scenario.py), the controller's two connectors, and the reference's loader construction."""
import numpy as np
import torch
from torch.utils.data import ConcatDataset, DataLoader, RandomSampler

from pdecontrol.mbrl.replay import ExperienceReplay
from pdecontrol.mbrl.types import Sample
from pdecontrol.surrogates.common.dataset import PDEDataLoader, SubSeqDataset
from pdegym.common.transforms import BatchTransform, ScaleTransform, SensorTransform, SampleTransform

FIELDS = ("obs", "actions", "nxtobs", "rewards", "terminated", "truncated", "steps")


def scripted_replay(width, act_dim, seed, steps, ends, low=-2.0, high=1.0, terminated_at=None):
    """``steps`` vector steps of ``len(ends)`` sub-environments; sub-environment e ends an episode after each of its step
    counts in ``ends[e]``.  Observations are seeded normals, actions uniform in [low, high], rewards in (-1, 0)."""
    rp = ExperienceReplay()
    rs = np.random.RandomState(seed)
    nenv = len(ends)
    t, count, n = np.zeros(nenv, dtype=np.int64), np.zeros(nenv, dtype=np.int64), 0
    for _ in range(steps):
        samples = []
        for e in range(nenv):
            count[e] += 1
            t[e] += 1
            done = int(count[e]) in ends[e]
            samples.append(Sample(rs.randn(1, width).astype(np.float32),
                                  rs.uniform(low, high, (1, act_dim)).astype(np.float32),
                                  rs.randn(1, width).astype(np.float32), np.float32(-rs.uniform(0.01, 0.99)),
                                  n == terminated_at, bool(done), np.int32(t[e])))
            n += 1
            if done:
                t[e] = 0
        rp.add(samples)
    return rp


def controller_connectors(act_dim, stride=1, per_column=False, width=None, low=-2.0, high=1.0, seed=0):
    """``(world_replay_to_agent, replay_to_agent)`` as the controller's ``setup_transforms`` builds them: observations
    scaled by running extrema and read through the agent's sensor, actions mapped from their bounds to [-1, 1].
    ``per_column`` gives both scalings one bound per column instead of the controller's aggregated scalars."""
    rs = np.random.RandomState(seed + 500)
    if per_column:
        lo = -3.0 - rs.uniform(0, 1, (1, 1, width)).astype(np.float32)
        hi = 3.0 + rs.uniform(0, 1, (1, 1, width)).astype(np.float32)
        oscaling = ScaleTransform(bounds=(lo, hi), aggregate=False, batched=True, frozen=True)
        alow = (low - rs.uniform(0, 1, (1, 1, act_dim))).astype(np.float32)
        ahigh = (high + rs.uniform(0, 1, (1, 1, act_dim))).astype(np.float32)
    else:
        oscaling = ScaleTransform(batched=True, aggregate=True, frozen=False)
        oscaling.update(rs.randn(16, 1, 8).astype(np.float32) * 1.7)
        alow = np.full((1, 1, act_dim), low, dtype=np.float32)
        ahigh = np.full((1, 1, act_dim), high, dtype=np.float32)
    ascaling = ScaleTransform(bounds=(alow, ahigh), aggregate=not per_column, frozen=True, batched=True).Inverse
    agent_sensor = BatchTransform(SensorTransform(stride=stride))
    replay_to_agent = SampleTransform(otransf=[oscaling, agent_sensor], atransf=ascaling.Inverse)
    world_replay_to_agent = SampleTransform(atransf=ascaling.Inverse)
    return world_replay_to_agent, replay_to_agent


def replay_pair(obs_dim=8, act_dim=4, stride=1, seed=0, per_column=False, terminated_at=None, scale=1):
    """``[imagined, real]`` datasets as the controller's ``update_policy`` builds them.  The agent sees ``obs_dim``
    columns: the real replay stores ``obs_dim * stride`` and is read through the sensor, the imagined one stores them."""
    world = scripted_replay(obs_dim, act_dim, seed + 1, 21 * scale, {0: (4, 11, 30), 1: (9,), 2: (15, 16)},
                            terminated_at=terminated_at)
    real = scripted_replay(obs_dim * stride, act_dim, seed + 2, 14 * scale, {0: (5, 12), 1: (8,)})
    to_agent_world, to_agent = controller_connectors(act_dim, stride, per_column, obs_dim * stride, seed=seed)
    make = lambda rp, stransf: SubSeqDataset(data=rp.data, length=1, stride=1, bootstrapping=False, stransf=stransf)
    return [make(world, to_agent_world), make(real, to_agent)]


def reference_loader(datasets, batch_size, num_updates):
    """The loader of the reference's ``update_policy`` (pdecontrol/mbrl/mbrl.py:545-560)."""
    data = ConcatDataset(tuple(datasets))
    sampler = RandomSampler(data, replacement=True, num_samples=batch_size * num_updates)
    return DataLoader(dataset=data, batch_size=batch_size, shuffle=False, sampler=sampler,
                      collate_fn=PDEDataLoader.sample_collate)


def collate_items(datasets, indices):
    """The collated batch of the given items of ``ConcatDataset(datasets)``."""
    data = ConcatDataset(tuple(datasets))
    return PDEDataLoader.sample_collate([data[int(i)] for i in indices])


def same_batch(got, want, what=""):
    assert len(got) == len(want) == 7
    for name, g, w in zip(FIELDS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        assert torch.equal(g.cpu(), w.cpu()), (what, name)
