"""Fused projection head op: out = W4 @ gelu(W3 @ x + b3) + b4.

GPU path runs the single-pass HIP kernels (see csrc/proj_head.hip for the
traffic analysis — avoids the reference's ~25 GB/step of intermediate HBM
round trips at the flagship config); CPU path is the plain composition.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import _ext

__all__ = ["proj_head", "proj_head_supported", "proj_head_range",
           "proj_head_fused_bwd"]

# caps of the kernels (register tiles are sized by them; the extension
# re-checks every one, and the LDS bound, before launching)
MAX_IN, MAX_MID, MAX_OUT = 32, 512, 8
# the shape with compile-time M / I kernels, a bf16 forward and the fused
# backward: in, mid, largest out
PINNED_IN, PINNED_MID, PINNED_MAX_OUT = 20, 128, 2
# dynamic LDS ProjDims::bwd_lds (csrc/proj_head.hip) may ask for
BWD_LDS_LIMIT = 160 * 1024


def _pinned(i: int, m: int, o2: int) -> bool:
    return i == PINNED_IN and m == PINNED_MID and o2 <= PINNED_MAX_OUT


def proj_head_bwd_lds(itemsize: int, i: int, m: int, o2: int) -> int:
    """LDS bytes of proj_head_bwd_kernel: W3, b3, W4 and the four per-wave
    gb3 / gW4 partials (the same formula as ProjDims::bwd_lds)."""
    return itemsize * (m * i + m + o2 * m + 4 * m + 4 * o2 * m)


def proj_head_fused_bwd(dtype, i: int, m: int, o2: int) -> bool:
    """Whether backward is the one-kernel proj_head_bwd_fused (no [B,M,S]
    hidden-grad tensor); otherwise proj_head_bwd plus the channel-mix ops."""
    return dtype in (torch.float32, torch.bfloat16) and _pinned(i, m, o2)


def proj_head_range(dtype, i: int, m: int, o2: int) -> bool:
    """Shapes and dtypes the fused head takes, forward and backward."""
    if dtype == torch.bfloat16:
        return _pinned(i, m, o2)
    if dtype not in (torch.float32, torch.float64):
        return False
    itemsize = 4 if dtype == torch.float32 else 8
    return (i <= MAX_IN and m <= MAX_MID and o2 <= MAX_OUT
            and proj_head_bwd_lds(itemsize, i, m, o2) <= BWD_LDS_LIMIT)


def proj_head_supported(x: torch.Tensor, i: int, m: int, o2: int) -> bool:
    return x.is_cuda and proj_head_range(x.dtype, i, m, o2)


class _ProjHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W3, b3, W4, b4):
        B, I = x.shape[0], x.shape[1]
        S = x.numel() // max(B * I, 1)
        x3 = x.reshape(B, I, S).contiguous()
        ext = _ext.get(required=True)
        out = ext.proj_head_fwd(x3, W3.contiguous(), b3.contiguous(),
                                W4.contiguous(), b4.contiguous())
        ctx.save_for_backward(x3, W3, b3, W4)
        ctx.x_shape = tuple(x.shape)
        return out

    @staticmethod
    def backward(ctx, gy):
        x3, W3, b3, W4 = ctx.saved_tensors
        ext = _ext.get(required=True)
        if proj_head_fused_bwd(x3.dtype, x3.shape[1], W3.shape[0], W4.shape[0]):
            # flagship: one kernel, no [B,128,S] gz3 intermediate in HBM
            gx, gW3, gb3, gW4g, gb4 = ext.proj_head_bwd_fused(
                gy.contiguous(), x3, W3.contiguous(), b3.contiguous(),
                W4.contiguous())
            return (gx.reshape(ctx.x_shape), gW3.to(W3.dtype),
                    gb3.to(W3.dtype), gW4g.to(W3.dtype), gb4.to(W3.dtype))
        gz3, gb3, gW4g, gb4 = ext.proj_head_bwd(
            gy.contiguous(), x3, W3.contiguous(), b3.contiguous(), W4.contiguous())
        gx = ext.channel_mix_fwd_t(gz3, W3.contiguous())   # W3^T @ gz3
        gW3, _ = ext.channel_mix_bwd_w(gz3, x3, False)     # gz3 @ x^T
        return gx.reshape(ctx.x_shape), gW3, gb3, gW4g, gb4


def proj_head(x: torch.Tensor, W3, b3, W4, b4) -> torch.Tensor:
    """x: [B, I, *sp]; returns [B, O2, *sp] with the head fully fused.

    b3/b4 may be broadcast-shaped; flattened internally.  A GPU tensor
    outside proj_head_supported raises: the caller composes the head itself
    (nn/fno.py does, and records it).
    """
    b3f = b3.reshape(-1)
    b4f = b4.reshape(-1)
    i, m, o2 = W3.shape[1], W3.shape[0], W4.shape[0]
    if proj_head_supported(x, i, m, o2):
        out3 = _ProjHeadFn.apply(x, W3, b3f, W4, b4f)
        out_shape = list(x.shape)
        out_shape[1] = o2
        return out3.reshape(out_shape)
    if x.is_cuda:
        raise RuntimeError(
            f"proj_head: no fused kernel for in={i}, mid={m}, out={o2}, "
            f"{x.dtype} (see proj_head_supported)")
    # CPU reference composition
    h = F.gelu(torch.einsum("mi,bi...->bm...", W3, x)
               + b3f.view(1, -1, *([1] * (x.dim() - 2))))
    return torch.einsum("om,bm...->bo...", W4, h) + b4f.view(1, -1, *([1] * (x.dim() - 2)))
