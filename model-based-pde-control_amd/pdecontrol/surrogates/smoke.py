"""Tiny surrogate TBPTT step on cuda:0 for __graft_entry__.smoke(): the fused HIP kernels (libsurrogate_hip.so, the
default CUDA path) against the same module on the CPU, eagerly and through the captured hipGraph; then one SAC update on
libsac_hip.so against the same agent on the CPU (``run_sac``)."""
import torch


def run():
    from pdecontrol.surrogates import ops
    from pdecontrol.surrogates.bench_tbptt import build_module, synthetic_batch
    dev = torch.device("cuda", 0)
    cpu_module, gpu_module = build_module("cpu"), build_module(dev)
    s, a = synthetic_batch(B=4)
    ref = cpu_module.training_step((s, a), 0)
    ref["loss"].backward()
    batch = (s.to(dev), a.to(dev))
    assert ops.use_fused(batch[0]), "the fused HIP kernels must be the CUDA path"
    out = gpu_module.training_step(batch, 0)
    out["loss"].backward()
    torch.cuda.synchronize(dev)
    assert getattr(gpu_module.surrogate, "_fused_packs", None) is not None, "fused kernels did not run"
    rel = abs(float(out["loss"].detach()) - float(ref["loss"].detach())) / abs(float(ref["loss"].detach()))
    assert rel < 1e-5, rel
    gmax = max(float((pg.grad.cpu() - pc.grad).abs().max()) for pg, pc in
               zip(gpu_module.surrogate.parameters(), cpu_module.surrogate.parameters()) if pc.grad is not None)
    assert gmax < 1e-3, gmax
    # the same step as one replayed hipGraph (forward + backward + Adam inside the gradient-reduction launch)
    first = float(gpu_module.fused_step(batch)["loss"])
    for _ in range(3):
        last = float(gpu_module.fused_step(batch)["loss"])
    assert abs(first - float(ref["loss"].detach())) / abs(first) < 1e-5 and last < first
    print(f"smoke ok: fused surrogate TBPTT loss rel diff GPU vs CPU {rel:.2e}, max grad diff {gmax:.2e}; "
          f"graphed step trains ({first:.5f} -> {last:.5f})")
    run_sac(dev)


def run_sac(dev):
    """One SAC update at B = 8 on the kernels of libsac_hip.so against the same agent on the CPU (same seed, same noise)."""
    from argparse import Namespace
    from types import SimpleNamespace

    import numpy as np

    from pdecontrol.sac.sac import SAC
    B, N, A = 8, 64, 4
    box = lambda low, high, n: SimpleNamespace(low=np.full((1, n), low, np.float32), high=np.full((1, n), high, np.float32),
                                               shape=(1, n))
    logged = {}
    agents = {}
    for name, device in (("cpu", "cpu"), ("gpu", dev)):
        cfg = Namespace(gamma=0.99, tau=0.005, alpha=0.2, policy="Gaussian", target_update_interval=1,
                        automatic_entropy_tuning=True, cuda=False, device=device, hidden_size=256, lr=3e-4)
        torch.manual_seed(0)
        log = logged.setdefault(name, {})
        agents[name] = SAC(box(-np.inf, np.inf, N), box(-1.0, 1.0, A), cfg, logger=lambda e, commit=True, log=log: log.update(e))
    g = torch.Generator().manual_seed(1)
    x = torch.linspace(0, 6.2831853, N)
    field = lambda: (torch.sin(x + 6 * torch.rand(B, 1, 1, 1, generator=g)) * torch.rand(B, 1, 1, 1, generator=g))
    flags = torch.zeros(B, 1, dtype=torch.bool)
    batch = (field(), 2 * torch.rand(B, 1, 1, A, generator=g) - 1, field(), -torch.rand(B, 1, generator=g), flags, flags, flags.long())
    noise = (torch.randn(B, 1, A, generator=g), torch.randn(B, 1, A, generator=g))
    for agent in agents.values():
        agent.update(batch, noise=noise)
    torch.cuda.synchronize(dev)
    assert agents["gpu"]._fused is not None and agents["gpu"].updates == 1, "the SAC kernels did not run"
    # (log_alpha starts at zero, so the first entropy loss is exactly zero on both: compared through the others' scale)
    rel = {k: abs(float(logged["gpu"][k]) - float(v)) / max(abs(float(v)), 1e-3) for k, v in logged["cpu"].items()}
    assert set(rel) == {"Pol. Rew. Mean", "SAC/Qloss", "SAC/PolicyLoss", "SAC/entropy_loss", "SAC/alpha_loss"}
    assert all(r < 1e-4 for r in rel.values()), rel
    tgt = max(float((p.detach().cpu() - q.detach()).abs().max()) for p, q in zip(agents["gpu"].critic_target.parameters(),
                                                                 agents["cpu"].critic_target.parameters()))
    assert tgt < 1e-5, tgt          # tau * (one Adam step of 3e-4) = 1.5e-6 per element
    assert abs(float(agents["gpu"].log_alpha.detach()) - float(agents["cpu"].log_alpha.detach())) < 1e-8
    print(f"smoke ok: fused SAC update, losses rel diff GPU vs CPU {max(rel.values()):.2e}, target max diff {tgt:.2e}")
