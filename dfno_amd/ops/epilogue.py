"""Block epilogue with the time-axis irfft fused in.

``irfft_linear_res_gelu(x, W, Yt, n_half, n_out, m)`` computes

    gelu(W @_channel x + pad_irfft(Yt, -1, n_half, n_out, m))

The two-op form (``pad_irfft`` then ``linear_res_gelu``) writes the full real
activation to HBM only for the epilogue to read it straight back; the fused
kernel (csrc/epilogue.hip) reads the kept-mode spectrum instead (2m floats
per line where the real line is n_out) and synthesizes each output on the
fly.  ``need_z`` follows autograd: a no-grad forward skips the
pre-activation store as well.

Backward reuses the existing native kernels: the fused trunk mix backward
(or its three-kernel composition off the 20x20 shape) for ``gx, gW, gz`` and
``dft_pad_irfft_adj(gz)`` for the spectrum gradient.

With a stash entry (the block's arrangement: ``x`` also feeds the chain's
``rfft_trunc_stash``) the residual grad-x is not computed here at all: the
backward hands ``(gz, W)`` to the rfft adjoint's stash and the adjoint mode
of the same kernel (``rfft_adj_mix``) applies ``W^T`` to the register-resident
``gz`` column while it synthesizes the spectrum gradient — ``W^T gz`` never
reaches HBM and the mix backward drops its grad-x MFMA phase and store.
``DFNO_FUSED_RFFT_ADJ=0`` restores the stashed-``gx`` backward.

Shapes outside the kernel's range (and CPU tensors) compose the two existing
ops, which are native on GPU as well — no eager fallback is introduced.
"""

from __future__ import annotations

import os

import torch

from .. import _ext
from .fft import _GRAD_STASH, StashGradFn, pad_irfft
from .pointwise import linear_res_gelu

__all__ = ["irfft_linear_res_gelu", "fused_epilogue_enabled",
           "fused_epilogue_ok", "fused_rfft_adj_enabled", "rfft_adj_mix_ok"]


def fused_epilogue_enabled() -> bool:
    """Model-path gate (env DFNO_FUSED_EPILOGUE, default on; 0 restores the
    pad_irfft + linear_res_gelu pair for A/B runs in one build)."""
    return os.environ.get("DFNO_FUSED_EPILOGUE", "1") != "0"


def fused_epilogue_ok(dtype, I: int, O: int, n_out: int, m: int) -> bool:
    """Kernel range in terms of global configuration only."""
    return (dtype == torch.float32 and 1 <= I <= 32 and 1 <= O <= 64
            and 1 <= n_out <= 64 and 1 <= m <= min(32, n_out // 2 + 1))


def fused_rfft_adj_enabled() -> bool:
    """Backward-path gate (env DFNO_FUSED_RFFT_ADJ, default on; 0 restores
    the stashed-gx backward for A/B runs in one build)."""
    return os.environ.get("DFNO_FUSED_RFFT_ADJ", "1") != "0"


def rfft_adj_mix_ok(dtype, I: int, O: int, n: int, m: int) -> bool:
    """Range of the kernel's adjoint mode: the roles swap against the
    forward, the mix's O channels are the register-resident ones."""
    return (dtype == torch.float32 and 1 <= O <= 32 and 1 <= I <= 64
            and 1 <= n <= 64 and 1 <= m <= min(32, n // 2 + 1))


class _IrfftLinearResGeluFn(torch.autograd.Function):
    """``key``/``tok`` select the deferred grad-x backward.

    Mechanism: the epilogue itself receives the stash key, the rfft's
    ordering token and a DETACHED ``x``, and its backward fills
    ``_GRAD_STASH[key]`` with ``(gz, W)``.  No gradient flows to ``x`` from
    this node, so the engine has nothing to materialise or add for it (a
    ``None`` returned through a StashGradFn alias would be turned into a
    full zero tensor by the next custom Function, and its backward would
    overwrite the stash).  Ordering is what the alias gave: ``tok`` is an
    output of ``_RfftTruncStashFn`` and an input here, and this backward
    returns an (empty) gradient for it, so the rfft adjoint cannot run
    before this backward has filled the stash — the same hard graph edge,
    next to the data dependency through ``Yt``.  ``tok`` requires grad
    whenever ``x`` does, so this backward runs even with frozen ``W``."""

    @staticmethod
    def forward(ctx, x, W, Yt, n_out, key=None, tok=None):
        ext = _ext.get(required=True)
        B, I = x.shape[0], x.shape[1]
        O, m = W.shape[0], Yt.shape[-1]
        S = x.numel() // max(B * I, 1)
        x3 = x.reshape(B, I, S).contiguous()
        Y4 = Yt.reshape(B, O, S // n_out, m).contiguous()
        need_z = any(ctx.needs_input_grad[:3]) or key is not None
        Wc = W.contiguous()
        y3, z3 = ext.irfft_linear_res_gelu_fwd(x3, Wc, Y4, n_out, need_z)
        if need_z:
            ctx.save_for_backward(x3, Wc, z3)
        ctx.x_shape = tuple(x.shape)
        ctx.y_shape = tuple(Yt.shape)
        ctx.n_out = n_out
        ctx.key = key
        return y3

    @staticmethod
    def backward(ctx, gy):
        ext = _ext.get(required=True)
        x3, W, z3 = ctx.saved_tensors
        gy = gy.contiguous()
        B, I, S = x3.shape
        O = W.shape[0]
        m = ctx.y_shape[-1]
        if ctx.key is not None:
            # grad-x deferred to the rfft adjoint (rfft_adj_mix): gz, gW only
            if I == 20 and O == 20:
                _, gW, _, gz = ext.channel_mix_bwd_fused(gy, z3, x3, W,
                                                         False, True, False)
            else:
                gz = ext.gelu_bwd(gy, z3)
                gW, _ = ext.channel_mix_bwd_w(gz, x3, False)
            _GRAD_STASH[ctx.key] = (gz, W)
            gY = ext.dft_pad_irfft_adj(
                gz.reshape(B, O, S // ctx.n_out, ctx.n_out), 3, m)
            return (None, gW.to(W.dtype), gY.reshape(ctx.y_shape), None,
                    None, torch.empty(0, device=gy.device))
        if I == 20 and O == 20:
            # trunk 20x20: one kernel; gz comes back as the residual grad
            gx, gW, _, gz = ext.channel_mix_bwd_fused(gy, z3, x3, W,
                                                      False, True)
        else:
            gz = ext.gelu_bwd(gy, z3)
            gx = ext.channel_mix_fwd_t(gz, W)
            gW, _ = ext.channel_mix_bwd_w(gz, x3, False)
        gY = ext.dft_pad_irfft_adj(gz.reshape(B, O, S // ctx.n_out, ctx.n_out),
                                   3, m)
        return (gx.reshape(ctx.x_shape), gW.to(W.dtype),
                gY.reshape(ctx.y_shape), None, None, None)


def irfft_linear_res_gelu(x: torch.Tensor, W: torch.Tensor, Yt: torch.Tensor,
                          n_half: int, n_out: int, m: int,
                          stash=None) -> torch.Tensor:
    """gelu(W @_channel x + pad_irfft(Yt)) over the trailing (time) dim.

    ``Yt`` holds the kept low modes ``[..., min(m, n_half)]`` of the
    half-spectrum, as ``pad_irfft`` takes them.

    ``stash = (key, tok)`` from ``rfft_trunc_stash(x, -1, m, key)``: the
    gradient for ``x`` is not returned but folded into that rfft's adjoint —
    as ``(gz, W)`` for ``rfft_adj_mix`` where the kernel covers the shape,
    through a ``StashGradFn`` alias (today's stashed ``gx``) otherwise."""
    m = min(m, n_half)
    fused = (x.is_cuda and x.numel() > 0 and Yt.dtype == torch.complex64
             and Yt.shape[-1] == m and x.shape[-1] == n_out
             and fused_epilogue_ok(x.dtype, x.shape[1], W.shape[0], n_out, m))
    if stash is not None:
        key, tok = stash
        if (fused and fused_rfft_adj_enabled()
                and rfft_adj_mix_ok(x.dtype, x.shape[1], W.shape[0], n_out, m)):
            out = _IrfftLinearResGeluFn.apply(x.detach(), W, Yt, n_out,
                                              key, tok)
            shape = list(x.shape)
            shape[1] = W.shape[0]
            return out.reshape(shape)
        x = StashGradFn.apply(x, tok, key)
    if fused:
        out = _IrfftLinearResGeluFn.apply(x, W, Yt, n_out)
        shape = list(x.shape)
        shape[1] = W.shape[0]
        return out.reshape(shape)
    res = pad_irfft(Yt, -1, n_half, n_out, m, out_dtype=x.dtype)
    if res.dtype != x.dtype:
        res = res.to(x.dtype)
    return linear_res_gelu(x, W, res)
