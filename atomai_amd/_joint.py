"""The discrete (Gumbel-Softmax) channel of the joint VAEs on csrc/joint.hip: segmented softmax heads, the joint latent
kernel (reparameterisation of the continuous latents, Gumbel-Softmax sample of every head, per-sample KL to the uniform
categorical) and their gradients.  Every public function below is one launch of the same two kernel pairs with parts
switched off; there is no second copy of the math and no torch fallback (fp32 tensors on the device or an error).
"""
import ctypes as C
from typing import List, Optional, Sequence

import torch

from . import _lib as L

MAX_HEADS = 16       # AMX_JOINT_MAX_HEADS of include/atomai_amd.h
MAX_D = 4096         # AMX_JOINT_MAX_D


def check_discrete_dim(discrete_dim) -> List[int]:
    """Validates a list of head sizes against the kernel limits; returns it as a list of ints."""
    if not isinstance(discrete_dim, (list, tuple)) or len(discrete_dim) == 0:
        raise ValueError("discrete_dim must be a non-empty list of the sizes of the discrete latent variables")
    sizes = [int(k) for k in discrete_dim]
    if any(k < 1 for k in sizes):
        raise ValueError(f"every discrete dimension must be >= 1, got {list(discrete_dim)}")
    if len(sizes) > MAX_HEADS:
        raise ValueError(f"at most {MAX_HEADS} discrete latent variables are supported, got {len(sizes)}")
    if sum(sizes) > MAX_D:
        raise ValueError(f"the discrete dimensions may sum to at most {MAX_D}, got {sum(sizes)}")
    return sizes


def _segs(sizes: Sequence[int]):
    return (C.c_int * len(sizes))(*sizes)


def _f32(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: the joint-VAE kernels are fp32 only, got {t.dtype}")
    return t.detach().contiguous()


class _SegSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, sizes):
        x = _f32(logits, "seg_softmax")
        B, D = x.shape
        assert D == sum(sizes)
        alpha = torch.empty_like(x)
        L.call("amx_segsoftmax_fwd", L.ptr(x), _segs(sizes), len(sizes), B, L.ptr(alpha), L.stream_ptr(x))
        ctx.save_for_backward(alpha)
        ctx.sizes = tuple(sizes)
        return alpha

    @staticmethod
    def backward(ctx, dalpha):
        alpha, = ctx.saved_tensors
        d = _f32(dalpha, "seg_softmax backward")
        dlogits = torch.empty_like(alpha)
        L.call("amx_segsoftmax_bwd", L.ptr(alpha), L.ptr(d), _segs(ctx.sizes), len(ctx.sizes), alpha.shape[0],
               L.ptr(dlogits), L.stream_ptr(alpha))
        return dlogits, None


def seg_softmax(logits: torch.Tensor, sizes: Sequence[int]) -> torch.Tensor:
    """Softmax over every head of a packed (B, sum(sizes)) row of logits."""
    return _SegSoftmaxFn.apply(logits, tuple(int(k) for k in sizes))


class _JointLatentFn(torch.autograd.Function):
    """(z_mean, z_logsd, eps, alpha, u) -> (theta, z_dec, kl_disc) in one launch each way (amx_joint_latent_fwd / _bwd).
    ``z_mean is None``: no continuous part; ``u is None``: no sample; ``want_kl`` False: no KL."""

    @staticmethod
    def forward(ctx, z_mean, z_logsd, eps, alpha, u, sizes, tau, coord, dx_prior, want_kl):
        al = _f32(alpha, "alpha")
        B, D = al.shape
        assert D == sum(sizes)
        dev = al.device
        if z_mean is not None:
            zm, zl, ep = _f32(z_mean, "z_mean"), _f32(z_logsd, "z_logsd"), _f32(eps, "eps")
            Z = zm.shape[1]
        else:
            zm = zl = ep = None
            Z = 0
        uu = None if u is None else _f32(u, "u")
        W = Z - coord + (D if uu is not None else 0)
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        theta = e(B, 3) if coord else None
        zdec = e(B, W) if W > 0 else None
        kl = e(B) if want_kl else None
        L.call("amx_joint_latent_fwd", L.ptr(zm), L.ptr(zl), L.ptr(ep), L.ptr(al), L.ptr(uu), _segs(sizes), len(sizes), B,
               Z, int(coord), float(dx_prior), float(tau), L.ptr(theta), L.ptr(zdec), L.ptr(kl), L.stream_ptr(al))
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(zl, ep, al, zdec)
        ctx.meta = (tuple(sizes), float(tau), int(coord), float(dx_prior), Z, uu is not None)
        return theta, zdec, kl

    @staticmethod
    def backward(ctx, dtheta, dzdec, gkl):
        zl, ep, al, zdec = ctx.saved_tensors
        sizes, tau, coord, dx_prior, Z, sampled = ctx.meta
        B = al.shape[0]
        c = lambda g: None if g is None else _f32(g, "upstream gradient")
        dtheta, dzdec, gkl = c(dtheta), c(dzdec), c(gkl)
        dm = torch.empty_like(zl) if Z else None
        dl = torch.empty_like(zl) if Z else None
        dalpha = torch.empty_like(al)
        L.call("amx_joint_latent_bwd", L.ptr(zl), L.ptr(ep), L.ptr(al), L.ptr(zdec), L.ptr(dtheta), L.ptr(dzdec),
               L.ptr(gkl), _segs(sizes), len(sizes), B, Z, coord, dx_prior, tau, int(sampled), L.ptr(dm), L.ptr(dl),
               L.ptr(dalpha), L.stream_ptr(al))
        return dm, dl, None, dalpha, None, None, None, None, None, None


def joint_latent(z_mean, z_logsd, eps, alpha, u, sizes, tau: float, coord: int, dx_prior: float):
    """The whole latent step of a joint model: returns (theta (B, 3) or None, z_dec (B, Z - coord + D), kl_disc (B))."""
    return _JointLatentFn.apply(z_mean, z_logsd, eps, alpha, u, tuple(int(k) for k in sizes), tau, coord, dx_prior, True)


def gumbel_softmax(alpha: torch.Tensor, u: torch.Tensor, tau: float) -> torch.Tensor:
    """Gumbel-Softmax sample of ONE head from its uniform noise ``u``: softmax((log(alpha + 1e-12) + g(u)) / tau)."""
    sizes = check_discrete_dim([alpha.shape[1]])
    return _JointLatentFn.apply(None, None, None, alpha, u, tuple(sizes), tau, 0, 0.0, False)[1]


def kl_discrete_rows(alpha: torch.Tensor, sizes: Optional[Sequence[int]] = None) -> torch.Tensor:
    """Per-sample KL (B,) of the packed heads ``alpha`` (default: one head) to the uniform categorical."""
    sizes = check_discrete_dim([alpha.shape[1]] if sizes is None else list(sizes))
    return _JointLatentFn.apply(None, None, None, alpha, None, tuple(sizes), 1.0, 0, 0.0, True)[2]
