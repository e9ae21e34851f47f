"""The network of the denoising autoencoder (reference: atomai/models/denoiser.py:83-130, `_build_autoencoder`):

    Sequential(encoder, decoder)
      encoder = Sequential([ConvBlock -> MaxPool2d(2, 2)]* -> ConvBlock)
      decoder = Sequential(ConvBlock, [UpsampleBlock(C -> C) -> ConvBlock]*, Conv2d(C, 1, 1))

Same module tree, hence the same ``state_dict()`` keys (``0.<i>.block.<j>.weight``, ``1.<i>.conv.weight``,
``1.<last>.weight`` ...), shapes and RNG-order initialisation as the reference.  The children are parameter containers
only: ``forward`` runs the whole net as ONE tape (engine.Tape), and the trainers' fused step ends it in the one-pass
head + MSE node (engine.PxLossNode, kind 'mse') when that node takes the head."""
from typing import List

import torch
import torch.nn as nn

from .blocks import ConvBlock, UpsampleBlock
from .fcnn import _HipNet, _hip_pool, _hip_px
from ._function import run_tape


def _call_as(module: nn.Module, fn, x):
    """``module(x)`` with ``fn`` as its forward for this one call: hooks attached to the module still fire around it."""
    module.forward = fn                                # instance attribute, for one call (as fcnn._hip_px)
    try:
        return module(x)
    finally:
        del module.forward


class DenoiserNet(_HipNet, nn.Sequential):
    """``DenoiserNet(encoder_filters, decoder_filters, encoder_layers, decoder_layers, use_batch_norm, upsampling_mode)``:
    any list lengths and positive filter counts, 'nearest' or 'bilinear'.  The input is (N, 1, H, W) with H and W
    divisible by ``2 ** (len(encoder_filters) - 1)`` (one 2x2 pooling between encoder blocks)."""

    def __init__(self, encoder_filters: List[int], decoder_filters: List[int], encoder_layers: List[int],
                 decoder_layers: List[int], use_batch_norm: bool = False, upsampling_mode: str = "nearest") -> None:
        enc, dec = [], []
        cin = 1
        for i, (nf, nl) in enumerate(zip(encoder_filters, encoder_layers)):
            enc.append(ConvBlock(2, nl, cin, nf, batch_norm=use_batch_norm))
            if i < len(encoder_filters) - 1:
                enc.append(nn.MaxPool2d(2, 2))
            cin = nf
        for i, (nf, nl) in enumerate(zip(decoder_filters, decoder_layers)):
            if i > 0:
                dec.append(UpsampleBlock(2, cin, cin, mode=upsampling_mode))
            dec.append(ConvBlock(2, nl, cin, nf, batch_norm=use_batch_norm))
            cin = nf
        dec.append(nn.Conv2d(cin, 1, 1))
        nn.Sequential.__init__(self, nn.Sequential(*enc), nn.Sequential(*dec))

    # ---- geometry
    def _npool(self) -> int:
        return sum(isinstance(m, nn.MaxPool2d) for m in self[0])

    def _check_input(self, x: torch.Tensor) -> None:
        if x.ndim != 4 or x.shape[1] != 1:
            raise AssertionError("the denoiser takes a (N, 1, H, W) tensor")
        f = 2 ** self._npool()
        if x.shape[2] % f or x.shape[3] % f:
            raise AssertionError(f"the denoiser needs H and W divisible by {f} ({self._npool()} 2x2 poolings between "
                                 f"its encoder blocks); got {tuple(x.shape[2:])}")

    # ---- the single-tape path
    def _build(self, tape, x, px_mode: int = 0):
        self._check_input(x)
        enc, dec = list(self[0]), list(self[1])
        pool_next = len(enc) > 1 and isinstance(enc[1], nn.MaxPool2d)
        node, act = enc[0]._emit_input(tape, x, pool_next=pool_next)
        for m in enc[1:] + dec[:-1]:
            act = tape.pool(act) if isinstance(m, nn.MaxPool2d) else m._emit(tape, [act])
        return node, self._px(tape, act, dec[-1], px_mode)

    # ---- block by block, for hooks: every block, pooling and the final 1x1 convolution still on the HIP kernels
    def _modular(self, x):
        self._check_input(x)

        def run(seq):
            def fwd(h):
                for m in seq:
                    if isinstance(m, nn.MaxPool2d):
                        h = _call_as(m, lambda t: _hip_pool(t, self.training), h)
                    elif isinstance(m, nn.Conv2d):
                        h = _hip_px(h, m, self.training)
                    else:
                        h = m(h)
                return h
            return fwd
        return _call_as(self[1], run(self[1]), _call_as(self[0], run(self[0]), x))

    def _hooked(self) -> bool:
        return any(len(m._forward_hooks) or len(m._forward_pre_hooks) for m in self.modules() if m is not self)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if self._hooked():
            return self._modular(x)
        return run_tape(self._build, x, list(self.parameters()), self.training)

    def forward_loss(self, x: torch.Tensor, target: torch.Tensor, criterion=None):
        """('loss', mean squared error of net(x) against the float target [N][1][H][W]) when the head and the loss ran as
        the fused node (engine.PxLossNode, kind 'mse'), else ('logits', net(x)) — the caller then applies its criterion.
        Training mode only; `criterion`: None or a mean-reduction losses_metrics.MSELoss."""
        from ..losses_metrics.losses import MSELoss
        ok = (isinstance(target, torch.Tensor) and x.ndim == 4 and target.dtype == torch.float32
              and tuple(target.shape) == tuple(x.shape) and x.shape[1] == 1
              and (criterion is None or (type(criterion) is MSELoss and criterion.reduction == "mean")))
        if not ok or not self.training or self._hooked():
            return "logits", self.forward(x)
        self._loss_target, self._loss_fused, self._loss_spec = target, False, ("mse", criterion)
        try:
            out = run_tape(self._build, x, list(self.parameters()), True)
        finally:
            self._loss_target, self._loss_spec = None, ("ce", None)
        return ("loss" if self._loss_fused else "logits"), out
