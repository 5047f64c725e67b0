"""Pointwise linear (channel/time mixing) and fused GELU ops.

MI355X-native implementation of the reference's einsum-based pointwise linear
(`torch.einsum(self.eqn, W, x)` at /root/reference/dfno/dfno.py:62) and the
separate `F.gelu` passes (/root/reference/dfno/dfno.py:291,335,338,350).

These ops are HBM-bandwidth-bound on MI355X (arithmetic intensity 2*I*O /
(4*(I+O)) flop/byte is ~5-9 for this model's widths, below the 25 flop/byte
fp32 ridge at 6.3 TB/s), so the native kernels win by FUSING: one kernel does
contraction + bias + GELU, touching the activation once instead of the
reference's three passes (einsum, +=bias, gelu).

Dispatch: CUDA tensors require the HIP extension (fail loudly — no silent
eager fallback on a GPU box); CPU uses pure-torch reference math.  The
channel-contraction kernel covers the shapes this model uses; exotic shapes
raise on GPU only if the extension is missing, otherwise fall back to a
library GEMM (rocBLAS einsum), which is an allowed library path.
"""

from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn.functional as F

from .. import _ext
from ..dispatch import note_fallback


def _native_dt(t: torch.Tensor, op: str = "channel_mix") -> bool:
    """fp32/fp64 native-kernel gate; bf16 is handled by the dedicated bf16
    branch at each call site BEFORE this check.  Anything else takes the
    composed-torch path (still on GPU via rocBLAS/eager) with a warn-once."""
    ok = t.dtype in (torch.float32, torch.float64)
    if not ok and t.is_cuda and t.dtype != torch.bfloat16:
        note_fallback(op, f"dtype {t.dtype} has no native kernel")
    return ok


_EMPTY_BF16 = {}


def _ebf(device):
    t = _EMPTY_BF16.get(device)
    if t is None:
        t = torch.empty(0, dtype=torch.bfloat16, device=device)
        _EMPTY_BF16[device] = t
    return t


def _bf16_mix_ok(x3: torch.Tensor, I: int, O: int, op: str) -> bool:
    """bf16-storage channel-mix kernel coverage (csrc/pointwise.hip); shapes the
    wide kernel takes instead are not a fallback."""
    if not (x3.is_cuda and x3.dtype == torch.bfloat16):
        return False
    S = x3.shape[2] if x3.dim() == 3 else 0
    ok = S % 8 == 0 and (I <= 32 or O <= 24)
    if not ok and not wide_mix_range(x3.dtype, I, O, S):
        note_fallback(op, f"bf16 shape I={I} O={O} S={S} outside kernel range")
    return ok


def wide_mix_range(dtype, I: int, O: int, S: int) -> bool:
    """Range of the wide channel-mix kernel (csrc/mix_wide.hip) as a pure
    function of dtype and shape: fp32 or bf16 storage, 33 <= max(I, O) <= 128
    (either side may be narrower), bf16 rows in whole 16-byte vectors.  The
    call sites ask it only where the <= 32 kernels do not already apply, so
    every narrower dispatch stays what it was."""
    if dtype not in (torch.float32, torch.bfloat16):
        return False
    if min(I, O) < 1 or not 33 <= max(I, O) <= 128:
        return False
    return dtype == torch.float32 or S % 8 == 0


def grad_w_caps_ok(dtype, I: int, O: int, S: int) -> bool:
    """The caps of the grad-W entry points (csrc/grad_w.hip), stated once, for
    ``I`` x rows against ``O`` gz rows of length ``S``: the fp32 / fp64
    reduction takes at most 64 x rows; the bf16 one also at most 128 gz rows,
    in whole 128-element tiles."""
    if dtype == torch.bfloat16:
        return I <= 64 and O <= 128 and S % 128 == 0
    return I <= 64


def _wide_mix_ok(x3: torch.Tensor, I: int, O: int) -> bool:
    """``wide_mix_range`` for a GPU tensor ``[B, I, S]``."""
    return bool(x3.is_cuda and x3.dim() == 3
                and wide_mix_range(x3.dtype, I, O, x3.shape[2]))


def _wide_mix(x3, W, b, res, act: bool, wt: bool, need_z: bool):
    e = torch.empty(0, dtype=x3.dtype, device=x3.device)
    return _ext.get(required=True).wide_channel_mix(
        x3.contiguous(), W.contiguous(),
        b.contiguous() if b is not None else e,
        res.contiguous() if res is not None else e, act, wt, need_z)

__all__ = ["linear_nd", "add_gelu", "gelu", "linear_res_gelu"]

_SQRT_2 = math.sqrt(2.0)
_INV_SQRT_2PI = 1.0 / math.sqrt(2.0 * math.pi)


def _gelu_grad(z: torch.Tensor) -> torch.Tensor:
    """d/dz gelu(z) for the exact (erf) gelu, matching F.gelu default."""
    return 0.5 * (1.0 + torch.erf(z / _SQRT_2)) + z * torch.exp(-0.5 * z * z) * _INV_SQRT_2PI


# ---------------------------------------------------------------------------
# channel-mix backward: y = act(W x + ...) with pre-activation z.  Each step
# owns its dispatch (fp32/fp64 native kernel, bf16 kernel within its caps,
# torch composition); mix_backward is the one entry the autograd Functions
# here and in ops/epilogue.py share.
# ---------------------------------------------------------------------------

def _gelu_bwd(gy: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """gz = gy * gelu'(z)."""
    if gy.is_cuda and _native_dt(gy):
        return _ext.get(required=True).gelu_bwd(gy, z)
    if gy.is_cuda and gy.dtype == torch.bfloat16 and gy.numel() % 8 == 0:
        return _ext.get(required=True).bf16_gelu_bwd(gy, z.contiguous())
    return gy * _gelu_grad(z)


def mix_t_slab(dtype, O: int, I: int) -> int:
    """Output rows per channel_mix_fwd_t call for gx = W^T gz with ``O`` gz
    rows and ``I`` gx rows, or 0 for one call.  csrc/pointwise.hip streams
    more than 32 input rows into register accumulators for up to 16 outputs
    (32 in fp32) and otherwise stages a [rows x 32] tile plus W in at most
    160 KiB of LDS; where that does not fit (fp64 512 -> 32 needs 262,400 B)
    the outputs go in slabs of 16 through the accumulator kernel, which
    streams at most 512 input rows."""
    if dtype not in (torch.float32, torch.float64):
        return 0
    itemsize = 4 if dtype == torch.float32 else 8
    acc_rows = 32 if dtype == torch.float32 else 16
    if O <= 32 or I <= acc_rows or O > 512:
        return 0
    fits = itemsize * (O * 32 + I * O + I) <= 160 * 1024
    return 0 if fits else 16


def _mix_bwd_x(gz: torch.Tensor, W: torch.Tensor, op: str) -> torch.Tensor:
    """gx[b,i,s] = sum_o W[o,i] gz[b,o,s]."""
    O, I = W.shape
    if gz.is_cuda and _native_dt(gz):
        if min(I, O) > 32 and _wide_mix_ok(gz, O, I):
            return _wide_mix(gz, W, None, None, False, True, False)[0]
        ext = _ext.get(required=True)
        slab = mix_t_slab(gz.dtype, O, I)
        if slab:
            return torch.cat([ext.channel_mix_fwd_t(gz, W[:, i:i + slab].contiguous())
                              for i in range(0, I, slab)], dim=1)
        return ext.channel_mix_fwd_t(gz, W)
    if _bf16_mix_ok(gz, O, I, op):
        gx, _ = _ext.get(required=True).bf16_channel_mix(
            gz.contiguous(), W.contiguous(), _ebf(gz.device), False, True,
            False, _ebf(gz.device))
        return gx
    if _wide_mix_ok(gz, O, I):
        return _wide_mix(gz, W, None, None, False, True, False)[0]
    return torch.einsum("oi,bos->bis", W, gz)


def _mix_bwd_w(gz: torch.Tensor, x3: torch.Tensor, W: torch.Tensor,
               want_bias: bool):
    """gW[o,i] = sum_bs gz[b,o,s] x[b,i,s], gb[o] = sum_bs gz[b,o,s]."""
    I, O, S = x3.shape[1], W.shape[0], x3.shape[2]
    bf16 = gz.is_cuda and gz.dtype == torch.bfloat16
    if gz.is_cuda and _native_dt(gz) and grad_w_caps_ok(gz.dtype, I, O, S):
        gW, gb = _ext.get(required=True).channel_mix_bwd_w(
            gz.contiguous(), x3.contiguous(), want_bias)
    elif gz.is_cuda and _native_dt(gz) and grad_w_caps_ok(gz.dtype, O, I, S):
        # more than 64 x rows against few gz rows (linear4, 128 -> 1): the
        # same reduction with the roles swapped, gW^T[i,o] = sum x[i] gz[o]
        gWt, _ = _ext.get(required=True).channel_mix_bwd_w(
            x3.contiguous(), gz.contiguous(), False)
        gW = gWt.t().contiguous()
        gb = gz.sum(dim=(0, 2)) if want_bias else None
    elif bf16 and grad_w_caps_ok(gz.dtype, I, O, S):
        gW, gb = _ext.get(required=True).bf16_channel_mix_bwd_w(
            gz.contiguous(), x3.contiguous(), want_bias)
        gW, gb = gW.to(W.dtype), gb.to(W.dtype)
    else:
        # includes bf16 with more than 64 x rows (linear4 of a composed bf16
        # head at any width): the pinned bf16 dispatch trace has no grad-W
        # call there, so that one reduction stays with torch

        gW = torch.einsum("bos,bis->oi", gz, x3)
        gb = gz.sum(dim=(0, 2)) if want_bias else None
    return gW, gb if want_bias else None


def mix_backward(gy, z3, x3, W, *, act: bool, want_bias: bool = False,
                 want_gz: bool = False, want_gx: bool = True,
                 op: str = "channel_mix_bwd"):
    """Backward of ``y = act(W x + ...)`` with ``gy, z3, x3`` as ``[B,*,S]``
    and contiguous ``gy``: returns ``(gx, gW, gb, gz)``, with ``None`` for
    whatever was not asked for.  ``op`` names the caller in fallback notes."""
    if (act and gy.is_cuda and gy.dtype in (torch.float32, torch.bfloat16)
            and x3.shape[1] == 20 and W.shape[0] == 20
            and gy.dtype == x3.dtype):
        # trunk 20x20: one kernel (mix_bwd.hip); gz exists only if wanted,
        # and without want_gx the grad-x MFMA phase and store are skipped
        gx, gW, gb, gz = _ext.get(required=True).channel_mix_bwd_fused(
            gy, z3.contiguous(), x3.contiguous(), W.contiguous().float(),
            want_bias, want_gz, *(() if want_gx else (False,)))
        return (gx if want_gx else None, gW.to(W.dtype),
                gb.to(W.dtype) if want_bias else None,
                gz if want_gz else None)
    gz = _gelu_bwd(gy, z3) if act else gy
    gx = _mix_bwd_x(gz, W, op) if want_gx else None
    gW, gb = _mix_bwd_w(gz, x3, W, want_bias)
    return gx, gW, gb, gz if want_gz else None


# ---------------------------------------------------------------------------
# channel-contraction (dim=1) fused linear+bias+gelu
# ---------------------------------------------------------------------------

class _ChannelMixFn(torch.autograd.Function):
    """y[b,o,s] = act( sum_i W[o,i] x[b,i,s] + bias[o] ) with x [B,I,S]."""

    @staticmethod
    def forward(ctx, x, W, b, act: bool):
        B, I = x.shape[0], x.shape[1]
        S = x.numel() // max(B * I, 1)
        x3 = x.reshape(B, I, S)
        O = W.shape[0]
        # the wide kernel skips the pre-activation store in a no-grad forward
        need_z = act and any(ctx.needs_input_grad[:3])
        if x.is_cuda and _native_dt(x):
            ext = _ext.get(required=True)
            if min(I, O) > 32 and _wide_mix_ok(x3, I, O):
                y3, z3 = _wide_mix(x3, W, b, None, act, False, need_z)
            else:
                y3, z3 = ext.channel_mix_fwd(x3, W, b if b is not None else torch.empty(0, dtype=x.dtype, device=x.device), act)
        elif _bf16_mix_ok(x3, I, O, "channel_mix"):
            ext = _ext.get(required=True)
            y3, z3 = ext.bf16_channel_mix(
                x3.contiguous(), W.contiguous(),
                b.contiguous() if b is not None else _ebf(x.device),
                act, False, act, _ebf(x.device))
        elif _wide_mix_ok(x3, I, O):
            y3, z3 = _wide_mix(x3, W, b, None, act, False, need_z)
        else:
            z3 = torch.einsum("oi,bis->bos", W, x3)
            if b is not None:
                z3 = z3 + b.view(1, -1, 1)
            y3 = F.gelu(z3) if act else z3
        ctx.save_for_backward(x3, W, z3 if act else torch.empty(0))
        ctx.act = act
        ctx.has_bias = b is not None
        ctx.x_shape = tuple(x.shape)
        return y3

    @staticmethod
    def backward(ctx, gy):
        x3, W, z3 = ctx.saved_tensors
        gx, gW, gb, _ = mix_backward(gy.contiguous(), z3, x3, W, act=ctx.act,
                                     want_bias=ctx.has_bias)
        return gx.reshape(ctx.x_shape), gW, gb, None


def _linear_lastdim(x: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor],
                    act: bool) -> torch.Tensor:
    """Contraction over the trailing (time) dim via a library GEMM:
    y[..., o] = sum_t x[..., t] W[o, t] (+ b[o]), optionally gelu."""
    y = torch.matmul(x, W.t())
    if b is not None:
        y = y + b.reshape(*([1] * (y.dim() - 1)), -1)
    if act:
        y = F.gelu(y)
    return y


def linear_nd(x: torch.Tensor, W: torch.Tensor, b: Optional[torch.Tensor],
              dim: int, activation: Optional[str] = None) -> torch.Tensor:
    """Linear layer along tensor dim ``dim``: out_dim = W.shape[0],
    contraction over W.shape[1].  Optionally fused exact GELU.

    Bias ``b`` may be shaped [O] or broadcastable [1,..,O,..,1] (the
    reference stores it broadcast-shaped, dfno.py:29-35).
    """
    nd = x.dim()
    d = dim % nd
    act = activation == "gelu"
    b_flat = b.reshape(-1) if b is not None else None

    if d == nd - 1:
        return _linear_lastdim(x, W, b_flat, act)

    if d == 1:
        y3 = _ChannelMixFn.apply(x, W, b_flat, act)
        out_shape = list(x.shape)
        out_shape[1] = W.shape[0]
        return y3.reshape(out_shape)

    # general dim: move to 1, recurse
    xm = x.movedim(d, 1).contiguous()
    ym = _ChannelMixFn.apply(xm, W, b_flat, act)
    out_shape = list(xm.shape)
    out_shape[1] = W.shape[0]
    return ym.reshape(out_shape).movedim(1, d).contiguous()


# ---------------------------------------------------------------------------
# fused residual-linear epilogue: gelu(W @ x + res)  (block epilogue with the
# pass-through linear folded in — the reference computes y0 = linear(x) at
# block start and gelu(y0 + y) at the end, dfno.py:244,291; fusing removes
# the y0 materialization entirely)
# ---------------------------------------------------------------------------

class _LinearResGeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, res):
        B, I = x.shape[0], x.shape[1]
        S = x.numel() // max(B * I, 1)
        x3 = x.reshape(B, I, S)
        r3 = res.reshape(B, W.shape[0], S)
        need_z = any(ctx.needs_input_grad)   # wide kernel only: z is optional
        if x.is_cuda and _native_dt(x) and I > 32:
            # past the x-resident kernels' 32 input channels
            if _wide_mix_ok(x3, I, W.shape[0]):
                y3, z3 = _wide_mix(x3, W, None, r3, True, False, need_z)
            else:
                # fp64 (or I > 128): the LDS-path mix, then the fused add+gelu
                ext = _ext.get(required=True)
                m3, _ = ext.channel_mix_fwd(
                    x3.contiguous(), W,
                    torch.empty(0, dtype=x.dtype, device=x.device), False)
                y3, z3 = ext.add_gelu_fwd(m3, r3.contiguous())
        elif x.is_cuda and _native_dt(x):
            ext = _ext.get(required=True)
            y3, z3 = ext.linear_res_gelu_fwd(x3.contiguous(), W, r3.contiguous())
        elif _bf16_mix_ok(x3, x3.shape[1], W.shape[0], "linear_res_gelu"):
            ext = _ext.get(required=True)
            y3, z3 = ext.bf16_channel_mix(x3.contiguous(), W.contiguous(),
                                          _ebf(x.device), True, False, True,
                                          r3.contiguous())
        elif _wide_mix_ok(x3, I, W.shape[0]):
            y3, z3 = _wide_mix(x3, W, None, r3, True, False, need_z)
        else:
            z3 = torch.einsum("oi,bis->bos", W, x3) + r3
            y3 = F.gelu(z3)
        ctx.save_for_backward(x3, W, z3)
        ctx.x_shape = tuple(x.shape)
        ctx.res_shape = tuple(res.shape)
        return y3

    @staticmethod
    def backward(ctx, gy):
        x3, W, z3 = ctx.saved_tensors
        # gz is the residual grad as well
        gx, gW, _, gz = mix_backward(gy.contiguous(), z3, x3, W, act=True,
                                     want_gz=True, op="linear_res_gelu_bwd")
        return gx.reshape(ctx.x_shape), gW, gz.reshape(ctx.res_shape)


def linear_res_gelu(x: torch.Tensor, W: torch.Tensor, res: torch.Tensor) -> torch.Tensor:
    """gelu(W @_channel x + res): the block's residual path in one pass."""
    out = _LinearResGeluFn.apply(x, W, res)
    shape = list(x.shape)
    shape[1] = W.shape[0]
    return out.reshape(shape)


# ---------------------------------------------------------------------------
# fused residual-add + gelu (block epilogue, reference dfno.py:291)
# ---------------------------------------------------------------------------

class _AddGeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, bt):
        if a.is_cuda and _native_dt(a):
            ext = _ext.get(required=True)
            y, z = ext.add_gelu_fwd(a.contiguous(), bt.contiguous())
        elif a.is_cuda and a.dtype == torch.bfloat16 and a.numel() % 8 == 0:
            ext = _ext.get(required=True)
            y, z = ext.bf16_add_gelu(a.contiguous(), bt.contiguous())
        else:
            z = a + bt
            y = F.gelu(z)
        ctx.save_for_backward(z)
        return y

    @staticmethod
    def backward(ctx, gy):
        (z,) = ctx.saved_tensors
        gz = _gelu_bwd(gy.contiguous(), z)
        return gz, gz


def add_gelu(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """gelu(a + b), one fused pass on GPU."""
    return _AddGeluFn.apply(a, b)


class _GeluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        if x.is_cuda and _native_dt(x):
            ext = _ext.get(required=True)
            y = ext.gelu_fwd(x.contiguous())
        elif x.is_cuda and x.dtype == torch.bfloat16 and x.numel() % 8 == 0:
            ext = _ext.get(required=True)
            y = ext.bf16_gelu_fwd(x.contiguous())
        else:
            y = F.gelu(x)
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, gy):
        (x,) = ctx.saved_tensors
        return _gelu_bwd(gy.contiguous(), x)


def gelu(x: torch.Tensor) -> torch.Tensor:
    return _GeluFn.apply(x)
