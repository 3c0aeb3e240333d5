"""Physics-informed training losses (API mirror of the reference's ``pdecontrol/surrogates/phyloss/phyloss.py``:
``PhyPDELoss`` :13-33, ``BurgersPhyPDELoss`` :36-89; ``MSELoss`` is re-exported so that the controller's
``getattr(phyloss, config.loss)`` resolves it too).

The loss compares every state of a trajectory with the state the PDE's own time stepper makes of its predecessor:
for ``augmented`` [B, T, 1, N]

    target[:, 0] = augmented[:, -1]               (the LAST slice -- what the reference computes for slot 0; kept)
    target[:, t] = phyevolve^substeps(augmented[:, t-1])            t >= 1
    loss         = MSELoss(reduction)(augmented, target)

``substeps`` (default 1 = the reference) is the one extension: ``pdegym.burgers`` advances ``cfg_steps`` sub-steps of
``dt`` per ``env.step``, so only ``substeps = cfg_steps`` makes the loss of a solver trajectory vanish.  It is
deliberately not called ``cfg_steps``: the controller passes ``**scenario`` through ``ignore_extra_keywords``, and its
own call line must keep computing what the reference's does.

On fp32 CUDA tensors of a grid width the Burgers kernels handle, the element-wise loss and its gradient are one launch
each (``phyloss_hip``, csrc/burgers.hip); CPU tensors, fp64 and the explicit opt-out (``ops.fused(False)``) run the torch
spelling below, whose operation order is the reference's (the CPU result is bit-equal, tests/test_phyloss_host.py).
"""
from typing import Dict

import torch
from torch.nn import MSELoss  # noqa: F401  resolved by name from this module

from pdecontrol.surrogates.utils import Conv1dDerivative


class PhyPDELoss:
    """Base class: ``__call__`` builds the physics targets with ``phyevolve`` and applies the criterion."""

    def __init__(self, reduction: str = "none", substeps: int = 1):
        if int(substeps) < 1:
            raise ValueError(f"substeps must be at least 1, got {substeps}")
        self.criterion = torch.nn.MSELoss(reduction=reduction)
        self.substeps = int(substeps)

    def __call__(self, augmented, *args, **kwargs):
        """``augmented`` [B, T, C, N]; anything else (``loss(decoded, states)`` passes the true states) is ignored."""
        evolved = augmented
        for _ in range(self.substeps):
            evolved = self.phyevolve(evolved)
        # slot 0 has no predecessor: the reference compares it with the last slice
        targets = torch.cat((augmented[:, -1, None, :, :], evolved[:, :-1, :, :]), dim=1)
        return self.criterion(augmented, targets)

    def residual(self, augmented):
        raise NotImplementedError

    def phyevolve(self, augmented):
        raise NotImplementedError


class BurgersPhyPDELoss(PhyPDELoss):
    """Viscous Burgers, ``u_t = nu u_xx - u u_x``, periodic: 2nd-order central gradient, 4th-order central Laplacian,
    one explicit-midpoint step of ``dt`` per ``phyevolve``."""
    # cross-correlation taps, in the order nn.Conv1d applies them
    FIRST_DERIVATIVE_SECOND_ORDER_CENTRAL = [-1 / 2, 0, 1 / 2]
    SECOND_DERIVATIVE_FOURTH_ORDER_CENTRAL = [-1 / 12, 4 / 3, -5 / 2, 4 / 3, -1 / 12]

    def __init__(self, dx, dt, nu, reduction: str = "none", substeps: int = 1):
        super().__init__(reduction=reduction, substeps=substeps)
        self.dx, self.dt, self.nu = dx, dt, nu
        self.grad, self.laplace = self._stencils(torch.device("cpu"), torch.float32)
        self._by_kind = {}

    def _stencils(self, device, dtype):
        grad = Conv1dDerivative(filter=[[self.FIRST_DERIVATIVE_SECOND_ORDER_CENTRAL]], resolution=self.dx, kernel_size=3,
                                padding=1, padding_mode="circular")
        laplace = Conv1dDerivative(filter=[[self.SECOND_DERIVATIVE_FOURTH_ORDER_CENTRAL]], resolution=self.dx ** 2,
                                   kernel_size=5, padding=2, padding_mode="circular")
        if dtype != torch.float32:     # the taps at the tensor's own precision, not fp32 taps widened
            for mod, taps in ((grad, self.FIRST_DERIVATIVE_SECOND_ORDER_CENTRAL),
                              (laplace, self.SECOND_DERIVATIVE_FOURTH_ORDER_CENTRAL)):
                mod.filter.weight = torch.nn.Parameter(torch.as_tensor([[taps]], dtype=dtype), requires_grad=False)
        return grad.to(device), laplace.to(device)

    def _stencils_for(self, tensor):
        if tensor.device.type == "cpu" and tensor.dtype == torch.float32:
            return self.grad, self.laplace
        key = (tensor.device, tensor.dtype)
        if key not in self._by_kind:
            self._by_kind[key] = self._stencils(*key)
        return self._by_kind[key]

    def residual(self, augmented):
        b, t, c, h = augmented.shape
        grad, laplace = self._stencils_for(augmented)
        rows = augmented.reshape(b * t, c, h)
        ux = grad(rows).reshape(b, t, c, h)
        uxx = laplace(rows).reshape(b, t, c, h)
        return self.nu * uxx - rows.reshape(b, t, c, h) * ux

    def phyevolve(self, augmented):
        """One explicit-midpoint ("improved Euler") step of ``dt``."""
        utilde = augmented + 0.5 * self.dt * self.residual(augmented)
        return augmented + self.dt * self.residual(utilde)

    def __call__(self, augmented, *args, **kwargs):
        from pdecontrol.surrogates.phyloss import phyloss_hip
        if phyloss_hip.use_kernels(augmented):
            elementwise = phyloss_hip.burgers_phyloss(augmented, self.dx, self.dt, self.nu, self.substeps)
            reduction = self.criterion.reduction
            return elementwise if reduction == "none" else (elementwise.mean() if reduction == "mean" else elementwise.sum())
        return super().__call__(augmented)

    def check(self, scenario: Dict, module):
        assert scenario["cfg_steps"] == module.surrogate.psteps
