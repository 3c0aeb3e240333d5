"""What the collection segment path shares, without a GPU: the one slab struct behind its three C and three Python names,
and the reward expression each env owns (``rewards_of``), which the segment's host epilogue calls in place of a branch
on the env's kind."""
import ctypes
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _collect_scenario as sc  # noqa: E402
import _real_replay_scenario as rr  # noqa: E402
from test_burgers_collect_host import _bare_env  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_three_slab_names_are_one_struct():
    import hipbind
    import kspde
    from pdecontrol.mbrl import replay_hip
    from pdegym.burgers import _hip
    assert replay_hip.Slab is kspde.ks_record is _hip.Slabs is hipbind.Slabs
    assert ctypes.sizeof(hipbind.Slabs) == 64
    assert [n for n, _ in hipbind.Slabs._fields_] == list(rr.FIELDS) + ["rows"]
    for header, alias in (("replay_hip.h", "rp_slab"), ("kspde.h", "ks_record"), ("burgers_hip.h", "bg_slabs")):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
        assert '#include "replay/slabs.h"' in text, header
        assert re.search(r"^typedef replay_slabs %s;" % alias, text, re.M), header
        assert not re.search(r"struct %s\b" % alias, text), header
    text = open(os.path.join(ROOT, "include", "replay", "slabs.h")).read()
    assert len(re.findall(r"typedef struct (\w+)", text)) == 1 and "typedef struct replay_slabs {" in text


def _same_bits(a, b):
    assert a.dtype == b.dtype == np.float64 and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_ks_env_forms_the_rewards_of_finish_step():
    """``rewards_of`` on sums that hit the roundings (zero, a subnormal, 1e300, inf, NaN, sums whose reward lies halfway
    between two fp32 numbers) equals ``(-1.0) * (1 / N) * ssq / cfg_steps`` bit for bit, at any shape, and it is what
    ``_finish_step`` returns."""
    env = sc.build(E=5, N=64, device=-1).env
    N, n = env.N, env.cfg_steps
    assert len(rr.halfway_sums(N, n)) + 6 <= 4 * 5
    sums = rr.reward_sums(np.random.RandomState(3), 4, 5, N, n)
    assert np.isnan(sums).any() and np.isinf(sums).any() and (sums == 0).any()
    with np.errstate(all="ignore"):
        want = (-1.0) * (1 / N) * sums / n
        _same_bits(env.rewards_of(sums), want)
        _same_bits(env.rewards_of(sums[2]), want[2])
        env.reset(seed=1)
        obs = np.zeros((5, N), dtype=np.float32)
        _same_bits(env._finish_step(obs, sums[1], np.zeros(5, dtype=np.int32))[1], want[1])


def test_the_burgers_env_forms_the_rewards_of_its_reward_scale():
    env = _bare_env()
    sums = rr.reward_sums(np.random.RandomState(4), 4, 5, env.N, env.cfg_steps)
    with np.errstate(all="ignore"):
        _same_bits(env.rewards_of(sums), sums * env.reward_scale())
        _same_bits(env.rewards_of(sums), sums * (-(1.0 / env.N) / env.cfg_steps))
    assert env.bind_stream(None) is None
