"""Fused FNO lift head op (see csrc/lift_head.hip).

Applies linear1 (time lift T_in -> T_out) + GELU + linear2 (channel lift) +
GELU in one kernel, for 1 <= T_in <= 16, T_out <= 64, C_in <= 4 and
width <= 64: ``lift_head_supported`` is the predicate of the narrow kernel
rows (width <= 24), ``lift_head_wide_range`` that of the wide ones (width
25..64; the model routes fp32 and fp64 there, bf16 stays composed by
measurement).  CPU / unsupported shapes use the composed path in the model
instead.
"""

from __future__ import annotations

import torch

from .. import _ext

__all__ = ["lift_head", "lift_head_supported", "lift_head_wide_range"]

# caps of the kernels (LDS tiles / register arrays are sized by them; the
# extension re-checks every one before launching)
MAX_T_IN, MAX_T_OUT, MAX_C_IN, MAX_WIDTH = 16, 64, 4, 24
# the wide rows of csrc/lift_head.hip (WCAP 64): widths past MAX_WIDTH up to
WIDE_MAX_WIDTH = 64
# T_in == 1 with T_out up to this goes in as [B, C, S] (kLaneKMaxTo in
# csrc/lift_head.hip, which refuses a longer T_out in that form)
LANE_K_MAX_T_OUT = 32


def lift_head_supported(x, t_in, t_out, c_in, width) -> bool:
    """The narrow kernel rows: a GPU tensor, width <= 24."""
    return (x.is_cuda
            and x.dtype in (torch.float32, torch.float64, torch.bfloat16)
            and 1 <= t_in <= MAX_T_IN and 1 <= t_out <= MAX_T_OUT
            and 1 <= c_in <= MAX_C_IN and 1 <= width <= MAX_WIDTH)


def lift_head_wide_range(dtype, t_in, t_out, c_in, width) -> bool:
    """The wide kernel rows (widths 25..64), as a pure host predicate: the
    caller checks that the tensor is on the GPU.  bf16 is left out although
    the kernels take it: at width 64 the fused bf16 forward + backward wins
    on the flagship lift (2.9 against 11.4 ms) but loses on the Navier-Stokes
    one (0.81 against 0.65 ms; profiles/optimization_log.md, "Lift head for
    widths 25-64"), so bf16 models keep the composed lift there."""
    return (dtype in (torch.float32, torch.float64)
            and 1 <= t_in <= MAX_T_IN and 1 <= t_out <= MAX_T_OUT
            and 1 <= c_in <= MAX_C_IN
            and MAX_WIDTH < width <= WIDE_MAX_WIDTH)


class _LiftHeadFn(torch.autograd.Function):
    """xs is [B, C, S] (T_in == 1 kernels) or [B, C, S, T_in] (general)."""

    @staticmethod
    def forward(ctx, xs, W1, b1, W2, b2):
        ext = _ext.get(required=True)
        out = ext.lift_head_fwd(xs, W1.contiguous(), b1.contiguous(),
                                W2.contiguous(), b2.contiguous())
        ctx.save_for_backward(xs, W1, b1, W2, b2)
        return out

    @staticmethod
    def backward(ctx, gy):
        xs, W1, b1, W2, b2 = ctx.saved_tensors
        ext = _ext.get(required=True)
        gx, gW1, gb1, gW2, gb2 = ext.lift_head_bwd(
            gy.contiguous(), xs, W1.contiguous(), b1.contiguous(),
            W2.contiguous(), b2.contiguous())
        # bf16 activations: weight grads come back fp32-accumulated
        return (gx, gW1.to(W1.dtype), gb1.to(b1.dtype), gW2.to(W2.dtype),
                gb2.to(b2.dtype))


def lift_head(x, W1, b1, W2, b2):
    """x: [B, C, *sp, T_in] -> [B, width, *sp, T_out], fully fused, for
    every shape either predicate above accepts (the extension raises
    "unsupported dims" outside them)."""
    B, C = x.shape[0], x.shape[1]
    sp = x.shape[2:-1]
    t_in = x.shape[-1]
    S = 1
    for d in sp:
        S *= d
    if t_in == 1 and W1.shape[0] <= LANE_K_MAX_T_OUT:
        # the T_in == 1 kernels take x with the unit time axis folded away
        xs = x.reshape(B, C, S).contiguous()
    else:
        xs = x.reshape(B, C, S, t_in).contiguous()
    # the extension takes the weights in x's dtype (no-op casts for a model
    # built in one dtype)
    W1, b1, W2, b2 = (t.to(x.dtype) for t in (W1, b1, W2, b2))
    out = _LiftHeadFn.apply(xs, W1, b1.reshape(-1), W2, b2.reshape(-1))
    return out.reshape(B, W2.shape[0], *sp, W1.shape[0])
