"""Segmentation losses on the HIP path (reference: atomai/losses_metrics/losses.py:139-174).

``select_loss('ce', nb_classes)`` returns a module with the same call signature as
``torch.nn.CrossEntropyLoss()`` / ``torch.nn.BCEWithLogitsLoss()`` (mean reduction), whose forward is ONE
kernel that also produces d loss / d logits, so ``loss.backward()`` costs nothing extra on this op.
``select_loss('dice')`` / ``select_loss('focal')`` return ``dice_loss`` / ``focal_loss`` (reference: losses.py:13-89) over the
kernels of csrc/dice.hip, the gradient produced in the forward pass as well.
"""
import torch
import torch.nn as nn

import os

from .. import _lib as L

# workgroups of the fused loss kernels (each walks its pixels with a grid stride, one dependent load chain per thread):
# 1024 blocks left 4 waves per SIMD to hide a ~2 us load round trip (2.2 TB/s on the 267 MB of a bs-32 512^2 CE pass)
LOSS_BLOCKS = [int(os.environ.get("AMX_LOSS_BLOCKS", "4096"))]


def _times_upstream(dl, g):
    """dlogits * (upstream gradient of the scalar loss) without a pass over dlogits when the upstream gradient is 1
    (``loss.backward()``): the factor is read on the device, nothing synchronises."""
    if g.numel() == 1 and g.dtype == torch.float32 and g.device == dl.device:
        L.call("amx_scale_unless_one", L.ptr(dl), L.ptr(g.contiguous()), dl.numel(), L.stream_ptr(dl))
        return dl
    return dl * g


class _CEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        N, K = logits.shape[0], logits.shape[1]
        HW = logits[0, 0].numel()
        x = logits.detach().contiguous()
        t = target.contiguous()
        need = logits.requires_grad
        dl = torch.empty_like(x) if need else None
        rows = max(1, min(LOSS_BLOCKS[0], (N * HW + 255) // 256))
        part = torch.empty(rows, dtype=torch.float32, device=x.device)
        L.call("amx_ce_fwd_bwd", L.ptr(x), L.ptr(t), L.ptr(dl), L.ptr(part), rows, N, K, HW,
               L.stream_ptr(x))
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        L.call("amx_reduce_rows", L.ptr(part), rows, 1, 1, 1.0 / (N * HW), L.ptr(loss), L.stream_ptr(x))
        ctx.dl = dl
        return loss

    @staticmethod
    def backward(ctx, g):
        dl, ctx.dl = ctx.dl, None
        return _times_upstream(dl, g), None


class _BCEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        x = logits.detach().contiguous()
        t = target.detach().contiguous().to(torch.float32)
        n = x.numel()
        need = logits.requires_grad
        dl = torch.empty_like(x) if need else None
        rows = max(1, min(LOSS_BLOCKS[0], (n + 255) // 256))
        part = torch.empty(rows, dtype=torch.float32, device=x.device)
        L.call("amx_bce_fwd_bwd", L.ptr(x), L.ptr(t), L.ptr(dl), L.ptr(part), rows, n, L.stream_ptr(x))
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        L.call("amx_reduce_rows", L.ptr(part), rows, 1, 1, 1.0 / n, L.ptr(loss), L.stream_ptr(x))
        ctx.dl = dl
        return loss

    @staticmethod
    def backward(ctx, g):
        dl, ctx.dl = ctx.dl, None
        return _times_upstream(dl, g), None


class CrossEntropyLoss(nn.Module):
    """torch.nn.CrossEntropyLoss() semantics: logits (N,K,H,W), int64 targets (N,H,W), mean."""

    def forward(self, logits, target):
        if target.dtype != torch.int64 or logits.ndim < 3 or target.shape != logits.shape[:1] + logits.shape[2:]:
            raise ValueError("expected logits (N,K,...) and int64 targets (N,...)")
        return _CEFn.apply(logits, target)

    def __repr__(self):
        return "CrossEntropyLoss()"


class BCEWithLogitsLoss(nn.Module):
    """torch.nn.BCEWithLogitsLoss() semantics (mean over all elements)."""

    def forward(self, logits, target):
        if target.shape != logits.shape:
            raise ValueError(f"Target size ({target.shape}) must be the same as input size ({logits.shape})")
        return _BCEFn.apply(logits, target)

    def __repr__(self):
        return "BCEWithLogitsLoss()"


class _MSEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        p, t = pred.detach(), target.detach()
        n = p.numel()
        need = pred.requires_grad
        dl = torch.empty_like(p) if need else None
        rows = L.load().amx_mse_rows(n)
        part = torch.empty(rows, dtype=torch.float32, device=p.device)
        sp = L.stream_ptr(p)
        L.call("amx_mse_fwd_bwd", L.ptr(p), L.ptr(t), L.ptr(dl), L.ptr(part), n, rows, sp)
        loss = torch.empty((), dtype=torch.float32, device=p.device)
        L.call("amx_reduce_rows", L.ptr(part), rows, 1, 1, 1.0 / n, L.ptr(loss), sp)
        ctx.dl = dl
        return loss

    @staticmethod
    def backward(ctx, g):
        dl, ctx.dl = ctx.dl, None
        return _times_upstream(dl, g), None


class MSELoss(nn.MSELoss):
    """torch.nn.MSELoss whose mean reduction over same-shape contiguous fp32 device tensors is ONE pass that also
    produces d loss / d prediction (csrc/signal.hip: amx_mse_fwd_bwd, deterministic two-stage sum) — the criterion of the
    im2spec / spec2im trainers.  Every other call (another reduction, broadcasting shapes, other dtypes, a target that
    requires a gradient, host tensors) is the parent class's, warnings included."""

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        on_device = input.is_cuda or L.is_test_backend()
        if (self.reduction == "mean" and on_device and input.device == target.device and input.shape == target.shape
                and input.dtype == torch.float32 and target.dtype == torch.float32 and input.numel() > 0
                and input.is_contiguous() and target.is_contiguous() and not target.requires_grad):
            return _MSEFn.apply(input, target)
        return super().forward(input, target)

    def __repr__(self):
        return "MSELoss()"


def dice_launch_plan(N: int, K: int, H: int, W: int):
    """(B, rows, nch): bins of the reference's dice loss (2 for one class, else K * W: one per class and image COLUMN,
    losses.py:85), rows of the partial tensor of amx_dice_sums / amx_px_dice_sums, chunk rows handed to amx_dice_finalize."""
    lib = L.load()
    rows = lib.amx_dice_rows(N, H, W, K)
    return lib.amx_dice_bins(K, W), rows, min(rows, 16)


def dice_table_and_loss(part, B: int, rows: int, nch: int, eps: float, sp):
    """Partial rows [rows][2][B] -> (table [B][2] of gradient coefficients, scalar loss): two small launches."""
    sums = torch.empty((nch, 2 * B), dtype=torch.float32, device=part.device)
    L.call("amx_reduce_rows_chunked", L.ptr(part), rows, 2 * B, nch, L.ptr(sums), sp)
    chunk = (rows + nch - 1) // nch
    nch = (rows + chunk - 1) // chunk                     # chunk rows the launch above has written
    table = torch.empty((B, 2), dtype=torch.float32, device=part.device)
    loss = torch.empty((), dtype=torch.float32, device=part.device)
    L.call("amx_dice_finalize", L.ptr(sums), nch, B, float(eps), L.ptr(table), L.ptr(loss), sp)
    return table, loss


def dice_target(logits, labels):
    """The target layouts of the reference's dice_loss.forward (losses.py:65-85) as kernel arguments (int64, float32):
    (N,H,W) labels of any integer type for K >= 2 classes, (N,1,H,W) labels for K == 1 (a float mask is truncated as
    ``.long()`` does).  Anything else raises ValueError."""
    if logits.ndim != 4:
        raise ValueError(f"dice_loss expects logits (N,K,H,W); got {tuple(logits.shape)}")
    N, K, H, W = logits.shape
    want = (N, 1, H, W) if K == 1 else (N, H, W)
    if not isinstance(labels, torch.Tensor) or tuple(labels.shape) != want or labels.dtype == torch.bool \
            or labels.is_complex():
        raise ValueError(f"dice_loss expects labels {want} for logits {tuple(logits.shape)}; got "
                         f"{tuple(labels.shape) if isinstance(labels, torch.Tensor) else type(labels)}")
    t = labels.detach()
    if K == 1 and t.dtype == torch.float32:
        return None, t.contiguous()
    return t.long().contiguous(), None


class _DiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, eps):
        N, K, H, W = logits.shape
        ti, tf = dice_target(logits, labels)
        x = logits.detach().contiguous()
        sp = L.stream_ptr(x)
        B, rows, nch = dice_launch_plan(N, K, H, W)
        part = torch.empty((rows, 2 * B), dtype=torch.float32, device=x.device)
        L.call("amx_dice_sums", L.ptr(x), L.ptr(ti), L.ptr(tf), L.ptr(part), rows, N, K, H, W, sp)
        table, loss = dice_table_and_loss(part, B, rows, nch, eps, sp)
        ctx.dl = None
        if logits.requires_grad:
            ctx.dl = torch.empty_like(x)
            L.call("amx_dice_bwd", L.ptr(x), L.ptr(ti), L.ptr(tf), L.ptr(table), L.ptr(ctx.dl), N, K, H, W, sp)
        return loss

    @staticmethod
    def backward(ctx, g):
        dl, ctx.dl = ctx.dl, None
        return _times_upstream(dl, g), None, None


class dice_loss(nn.Module):
    """The reference's Sorensen-Dice loss (losses.py:53-89) on the HIP path: the bin sums, a small coefficient table and
    the gradient as three kernels (csrc/dice.hip), the gradient produced in the forward pass like the 'ce' losses.
    As in the reference the sums of a multi-class loss run over N and H only (``dims = (0,) + range(2, labels.ndim)`` with
    (N,H,W) labels): one Dice ratio per class AND image column; a one-class loss has the two bins foreground / background."""

    def __init__(self, eps: float = 1e-7):
        super().__init__()
        self.eps = eps

    def forward(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        dice_target(logits, labels)               # (shapes are validated before autograd sees the call)
        return _DiceFn.apply(logits, labels, self.eps)


def focal_scalars(c, alpha: float, gamma: float):
    """(F, dF/dc) of the reference's focal loss as device scalars from the mean BCE `c` (one tiny launch, no sync)."""
    out = torch.empty((2,), dtype=torch.float32, device=c.device)
    L.call("amx_focal_from_bce", L.ptr(c), float(alpha), float(gamma), L.ptr(out[0:1]), L.ptr(out[1:2]), L.stream_ptr(c))
    return out[0], out[1:2]


def times_dfdc(g, dfdc):
    """upstream gradient * dF/dc on the device (the factor amx_scale_unless_one then applies)."""
    if not (g.numel() == 1 and g.dtype == torch.float32 and g.device == dfdc.device):
        return g.to(dfdc.dtype).to(dfdc.device).reshape(1) * dfdc
    out = torch.empty((1,), dtype=torch.float32, device=dfdc.device)
    L.call("amx_mul_scalars", L.ptr(g.contiguous()), L.ptr(dfdc), L.ptr(out), L.stream_ptr(dfdc))
    return out


class _FocalFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, alpha, gamma):
        x = logits.detach().contiguous()
        t = target.detach().contiguous().to(torch.float32)
        n = x.numel()
        dl = torch.empty_like(x) if logits.requires_grad else None
        rows = max(1, min(LOSS_BLOCKS[0], (n + 255) // 256))
        part = torch.empty(rows, dtype=torch.float32, device=x.device)
        L.call("amx_bce_fwd_bwd", L.ptr(x), L.ptr(t), L.ptr(dl), L.ptr(part), rows, n, L.stream_ptr(x))
        c = torch.empty((1,), dtype=torch.float32, device=x.device)
        L.call("amx_reduce_rows", L.ptr(part), rows, 1, 1, 1.0 / n, L.ptr(c), L.stream_ptr(x))
        loss, ctx.dfdc = focal_scalars(c, alpha, gamma)
        ctx.dl = dl
        return loss

    @staticmethod
    def backward(ctx, g):
        dl, ctx.dl = ctx.dl, None
        return _times_upstream(dl, times_dfdc(g, ctx.dfdc)), None, None, None


class focal_loss(nn.Module):
    """The reference's focal loss (losses.py:13-50): ``alpha * (1 - exp(-c))**gamma * c`` with c the MEAN
    BCE-with-logits — a scalar function of the mean, not a per-pixel focal term.  One-class nets only: logits and float
    labels of the same shape (anything else raises ValueError, as F.binary_cross_entropy_with_logits does)."""

    def __init__(self, alpha: float = 0.5, gamma: float = 2, with_logits: bool = True):
        super().__init__()
        if not with_logits:
            raise NotImplementedError("focal_loss(with_logits=False) (probabilities in) is outside this build: the "
                                      "segmentation nets end in logits and select_loss('focal') never builds it")
        self.alpha, self.gamma, self.logits = alpha, gamma, with_logits

    def forward(self, prediction: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        if not isinstance(labels, torch.Tensor) or labels.shape != prediction.shape:
            raise ValueError(f"Target size ({getattr(labels, 'shape', None)}) must be the same as input size "
                             f"({prediction.shape})")
        return _FocalFn.apply(prediction, labels, self.alpha, self.gamma)


def select_loss(loss: str, nb_classes: int = None, **kwargs):
    """Same selection logic and error behaviour as the reference (losses.py:139-174) for the losses on
    the hot path ('ce', 'dice', 'focal', callables); the others are outside this build's scope."""
    if loss in ['ce', 'multitask'] and nb_classes is None:
        raise ValueError("For cross-entropy loss function, you must specify the number of classes")
    if loss == 'dice':
        return dice_loss()
    if loss == 'focal':
        return focal_loss()
    if loss == 'ce' and nb_classes == 1:
        return BCEWithLogitsLoss()
    if loss == 'ce' and nb_classes > 2:
        return CrossEntropyLoss()
    if loss == 'mse':
        return MSELoss()
    if hasattr(loss, "__call__"):
        return loss
    if loss in ('nll', 'multitask_nll', 'multitask_ce'):
        raise NotImplementedError(f"loss '{loss}' is outside the MI355X hot path of this build")
    raise NotImplementedError(
        "Select Dice loss ('dice'), focal loss ('focal') "
        " cross-entropy loss ('ce'), means-squared error ('mse'),"
        " multitask loss (multitask_nll and multitask_ce)"
        " or pass your custom loss function")
