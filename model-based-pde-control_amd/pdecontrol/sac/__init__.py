"""Soft actor-critic agent under the reference's import path (``from pdecontrol.sac.sac import SAC``).  On the CPU it is
the reference's arithmetic bit for bit; on an MI355X ``act`` and ``update`` run on the kernels of csrc/sac.hip."""
