"""Block epilogue, with the time-axis irfft fused in where it applies.

``block_epilogue(x, W, y, stash=, irfft=)`` is the single entry for the FNO
block's ``gelu(W @_channel x + y)``, and the single place that decides how a
stashed input gradient is routed: it alone creates the ``StashGradFn`` alias.
Given ``irfft`` (``irfft_linear_res_gelu(x, W, Yt, n_half, n_out, m)`` is
that spelling) it computes

    gelu(W @_channel x + pad_irfft(Yt, -1, n_half, n_out, m))

The two-op form (``pad_irfft`` then ``linear_res_gelu``) writes the full real
activation to HBM only for the epilogue to read it straight back; the fused
kernel (csrc/epilogue.hip) reads the kept-mode spectrum instead (2m floats
per line where the real line is n_out) and synthesizes each output on the
fly.  ``need_z`` follows autograd: a no-grad forward skips the
pre-activation store as well.

Backward reuses the existing native kernels through the shared
``pointwise.mix_backward`` (the fused trunk mix backward, or its three-kernel
composition off the 20x20 shape) for ``gx, gW, gz``, and
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
from .pointwise import linear_res_gelu, mix_backward

__all__ = ["block_epilogue", "irfft_linear_res_gelu", "fused_epilogue_enabled",
           "fused_epilogue_ok", "fused_rfft_adj_enabled", "rfft_adj_mix_ok"]


def fused_epilogue_enabled() -> bool:
    """Model-path gate (env DFNO_FUSED_EPILOGUE, default on; 0 restores the
    pad_irfft + linear_res_gelu pair for A/B runs in one build)."""
    return os.environ.get("DFNO_FUSED_EPILOGUE", "1") != "0"


def fused_epilogue_ok(dtype, I: int, O: int, n_out: int, m: int) -> bool:
    """Routed range in terms of global configuration only.  The entry point
    also takes 33 to 64 input channels (the MFMA wide mix with the synthesis
    as its addend, csrc/mix_wide.hip), but at the width-64 flagship shape
    that kernel lost to ``pad_irfft`` + the wide mix, so wide blocks are not
    routed to it (profiles/optimization_log.md, "Time-axis irfft in the wide
    epilogue")."""
    return (dtype == torch.float32 and 1 <= I <= 32 and 1 <= O <= 64
            and 1 <= n_out <= 64 and 1 <= m <= min(32, n_out // 2 + 1))


def fused_rfft_adj_enabled() -> bool:
    """Backward-path gate (env DFNO_FUSED_RFFT_ADJ, default on; 0 restores
    the stashed-gx backward for A/B runs in one build)."""
    return os.environ.get("DFNO_FUSED_RFFT_ADJ", "1") != "0"


def rfft_adj_mix_ok(dtype, I: int, O: int, n: int, m: int) -> bool:
    """Routed range of the adjoint mode: the roles swap against the
    forward, the mix's O channels are the register-resident ones.  As in
    the forward, the entry point takes up to 64 of them and, for the same
    reason (same log entry), is not routed there."""
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
        x3, W, z3 = ctx.saved_tensors
        B, I, S = x3.shape
        deferred = ctx.key is not None
        gx, gW, _, gz = mix_backward(gy.contiguous(), z3, x3, W, act=True,
                                     want_gz=True, want_gx=not deferred)
        gtok = None
        if deferred:
            # grad-x is left to the rfft adjoint (rfft_adj_mix)
            _GRAD_STASH[ctx.key] = (gz, W)
            gtok = torch.empty(0, device=gy.device)
        else:
            gx = gx.reshape(ctx.x_shape)
        gY = _ext.get(required=True).dft_pad_irfft_adj(
            gz.reshape(B, W.shape[0], S // ctx.n_out, ctx.n_out), 3,
            ctx.y_shape[-1])
        return gx, gW, gY.reshape(ctx.y_shape), None, None, gtok


def block_epilogue(x: torch.Tensor, W: torch.Tensor, y: torch.Tensor,
                   stash=None, irfft=None) -> torch.Tensor:
    """The FNO block's epilogue ``gelu(W @_channel x + y)``.

    ``irfft = (n_half, n_out, m)``: ``y`` is still the kept-mode time
    spectrum ``[..., min(m, n_half)]`` as ``pad_irfft`` takes it, and the
    synthesis runs inside the fused kernel where it covers the shape.

    ``stash = (key, tok)`` from the transform that consumed ``x`` at the head
    of the chain (``rfft_trunc_stash`` / ``zt_fwd(stash_key=)``): the gradient
    for ``x`` is not returned to the engine but folded into that transform's
    adjoint.  This is the one place that chooses how — as ``(gz, W)`` for
    ``rfft_adj_mix`` where the fused kernel and its adjoint mode cover the
    shape (detached ``x``, no alias), through a ``StashGradFn`` alias (the
    stashed ``gx``) otherwise.  A ``zt_fwd`` stash takes a tensor only, so
    it never comes with ``irfft`` (the (z,t) synthesis owns the inverse
    wherever the (z,t) analysis ran)."""
    fused = False
    if irfft is not None:
        n_half, n_out, m = irfft
        m = min(m, n_half)
        fused = (x.is_cuda and x.numel() > 0 and y.dtype == torch.complex64
                 and y.shape[-1] == m and x.shape[-1] == n_out
                 and fused_epilogue_ok(x.dtype, x.shape[1], W.shape[0],
                                       n_out, m))
    key = tok = None
    if stash is not None:
        if (fused and fused_rfft_adj_enabled()
                and rfft_adj_mix_ok(x.dtype, x.shape[1], W.shape[0], n_out, m)):
            x = x.detach()
            key, tok = stash
        else:
            x = StashGradFn.apply(x, stash[1], stash[0])
    if fused:
        out = _IrfftLinearResGeluFn.apply(x, W, y, n_out, key, tok)
        shape = list(x.shape)
        shape[1] = W.shape[0]
        return out.reshape(shape)
    if irfft is not None:
        y = pad_irfft(y, -1, n_half, n_out, m, out_dtype=x.dtype)
        if y.dtype != x.dtype:
            y = y.to(x.dtype)
    return linear_res_gelu(x, W, y)


def irfft_linear_res_gelu(x: torch.Tensor, W: torch.Tensor, Yt: torch.Tensor,
                          n_half: int, n_out: int, m: int,
                          stash=None) -> torch.Tensor:
    """gelu(W @_channel x + pad_irfft(Yt)) over the trailing (time) dim:
    ``block_epilogue`` on a spectrum, ``stash`` as described there."""
    return block_epilogue(x, W, Yt, stash=stash, irfft=(n_half, n_out, m))
