"""Latent-space surrogate ablations (mirror of the reference's ``pdecontrol/architectures/latent.py``:
``KSLatentConvolutionalLSTM`` :10-67, ``KSLatentLSTM`` :70-102), plus ``KSLatentConvolutionalLSTMN`` -- the same network
with its LayerNorm widths derived from the grid size N, as ``KSAutoRegConvolutionalLSTMN`` is for the autoregressive model.

All three build a ``LatentAutoRegPDESurrogate``: the transition's output is integrated in latent space and the running
latent is decoded.  The convolutional ones have exactly the module tree (and state_dict keys) of the autoregressive
ConvLSTM, so on a GPU they run on the same fused kernels (``hipops.fused_latent_rollout``)."""
from torch import nn

from pdecontrol.architectures.autoreg import _conv_lstm_model
from pdecontrol.surrogates.factory import PDESurrogateFactory
from pdecontrol.surrogates.models.fcnn import LinearBlock
from pdecontrol.surrogates.surrogate import LatentAutoRegPDESurrogate
from pdecontrol.surrogates.transition import LSTMTransitionModel


class KSLatentConvolutionalLSTM(PDESurrogateFactory):
    """Hard-encoding initial conditions ablation; sizes fixed for N = 64."""

    def surrogate(self, **kwargs):
        return LatentAutoRegPDESurrogate(**kwargs)

    def model(self, **kwargs):
        return _conv_lstm_model(64)


class KSLatentConvolutionalLSTMN(PDESurrogateFactory):
    """Same architecture for any grid size N divisible by 4 (taken from the scenario's ``N``)."""

    def surrogate(self, **kwargs):
        return LatentAutoRegPDESurrogate(**kwargs)

    def model(self, N=64, **kwargs):
        assert N % 4 == 0
        return _conv_lstm_model(int(N))


class KSLatentLSTM(PDESurrogateFactory):
    """Fully-connected LSTM baseline: dense ELU encoder / decoder around a flat LSTM, raw 4 actuator values as actions."""

    def surrogate(self, **kwargs):
        return LatentAutoRegPDESurrogate(**kwargs)

    def model(self, **kwargs):
        state_encoder = nn.Sequential(LinearBlock(1, 64, 1, 32, activation=nn.ELU),
                                      LinearBlock(1, 32, 1, 16, activation=nn.ELU))
        state_decoder = nn.Sequential(LinearBlock(1, 16, 1, 32, activation=nn.ELU),
                                      LinearBlock(1, 32, 1, 64, activation=nn.Identity))
        action_encoder = nn.Identity()
        transition_model = LSTMTransitionModel(schannels=1, ssize=16, achannels=1, asize=4)
        return {"state_encoder": state_encoder, "state_decoder": state_decoder, "action_encoder": action_encoder,
                "transition_model": transition_model}
