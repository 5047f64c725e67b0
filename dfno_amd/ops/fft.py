"""Fused truncated-spectrum transforms for the FNO pencil chains.

Four linear ops cover every transform in DistributedFNOBlock:

  rfft_trunc(x, dim, m)            real -> kept low modes of the half-spectrum
  fft_trunc(x, dim, m_lo, m_hi)    complex -> kept low+high modes
  pad_ifft(y, dim, n, m_lo, m_hi)  kept modes -> full inverse (1/n folded in)
  pad_irfft(y, dim, n_half, n_out, m)  kept low half-spectrum modes -> real

On MI355X these run as single-pass hand-written DFT kernels (csrc/dft.hip):
for the kept-mode counts of an FNO (m ~ 8..24 of N ~ 30..64) a truncated
naive DFT costs N*m complex MACs per line — comparable FLOPs to a full FFT —
while fusing the mode truncation / zero-padding / 1/n scale into the
transform and reading the tensor ONCE along its native strides.  The
torch/hipFFT path this replaces pays a DtoD staging copy per transform,
permute copies for middle dims, separate cat/zeros passes for the
truncation, and their autograd mirrors (~25 ms/step at the flagship config).

Fallback (CPU, N > 64, or unsupported dtype) composes differentiable
torch.fft ops with identical semantics.

Two more things live here.  The residual-gradient stash: ``rfft_trunc_stash``
and ``zt_fwd(stash_key=)`` return an ordering token next to the spectrum, and
their adjoints add what the block epilogue left under the key; the second
consumer is wired up by ``ops.epilogue.block_epilogue`` alone, which is the
only caller of ``StashGradFn``.  And the fused (z,t) plane transforms of
csrc/dft2d.hip, whose caps are stated once, in ``zt_caps_ok``, as those of
the 1-D kernels of csrc/dft.hip are in ``dft_caps_ok``.
"""

from __future__ import annotations

import os

import torch

from .. import _ext
from ..dispatch import note_fallback

__all__ = ["rfft_trunc", "fft_trunc", "pad_ifft", "pad_irfft"]

# N <= 64: fully-tuned glds/radix-8x8 kernels.  64 < N <= 256: generalized
# radix-8xNB (c2c) and lines-per-tile (r2c/c2r) kernels — covers the 128^3 /
# 256^3 weak-scaling grids and nt <= 256 temporal scaling natively
# (VERDICT.md round-1 item 2).
_MAX_N = 256
_MAX_M = 32


def dft_caps_ok(n: int, m: int) -> bool:
    """The caps of csrc/dft.hip, stated once: transform length and kept-mode
    count of the 1-D kernels.  Every policy that must know whether they own
    a 1-D transform tests this."""
    return n <= _MAX_N and m <= _MAX_M


def _native_ok(x: torch.Tensor, n: int, m: int, op: str) -> bool:
    if not x.is_cuda:
        return False
    ok = (dft_caps_ok(n, m)
          and x.dtype in (torch.float32, torch.complex64,
                          torch.float64, torch.complex128))
    if not ok:
        note_fallback(op, f"N={n} (cap {_MAX_N}) / m={m} (cap {_MAX_M}) / "
                      f"dtype {x.dtype} outside the native-DFT range")
    return ok


# ---------------------------------------------------------------------------
# torch fallback compositions (differentiable; also the semantic reference)
# ---------------------------------------------------------------------------

def _t_rfft_trunc(x, dim, m):
    X = torch.fft.rfft(x, dim=dim)
    return X.narrow(dim, 0, m)


def _t_fft_trunc(x, dim, m_lo, m_hi):
    X = torch.fft.fft(x, dim=dim)
    lo = X.narrow(dim, 0, m_lo)
    if m_hi == 0:
        return lo.contiguous()
    hi = X.narrow(dim, X.shape[dim] - m_hi, m_hi)
    return torch.cat([lo, hi], dim=dim)


def _pad_modes(y, dim, n, m_lo, m_hi):
    pad = n - y.shape[dim]
    if pad < 1:
        return y
    shape = list(y.shape)
    shape[dim] = pad
    z = torch.zeros(shape, dtype=y.dtype, device=y.device, layout=y.layout)
    pieces = []
    if m_lo:
        pieces.append(y.narrow(dim, 0, m_lo))
    pieces.append(z)
    if m_hi:
        pieces.append(y.narrow(dim, y.shape[dim] - m_hi, m_hi))
    return torch.cat(pieces, dim=dim)


def _t_pad_ifft(y, dim, n, m_lo, m_hi):
    return torch.fft.ifft(_pad_modes(y, dim, n, m_lo, m_hi), dim=dim)


def _t_pad_irfft(y, dim, n_half, n_out, m):
    return torch.fft.irfft(_pad_modes(y, dim, n_half, m, 0), n=n_out, dim=dim)


# ---------------------------------------------------------------------------
# native autograd Functions
# ---------------------------------------------------------------------------

class _RfftTruncFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dim, m):
        ext = _ext.get(required=True)
        ctx.dim, ctx.m, ctx.n = dim, m, x.shape[dim]
        ctx.bf16 = x.dtype == torch.bfloat16
        return ext.dft_rfft_trunc(x.contiguous(), dim, m)

    @staticmethod
    def backward(ctx, gy):
        ext = _ext.get(required=True)
        if ctx.bf16:
            gx = ext.dft_rfft_trunc_adj_bf16(gy.contiguous(), ctx.dim,
                                             ctx.n, _zt_empty(gy.device))
        else:
            gx = ext.dft_rfft_trunc_adj(gy.contiguous(), ctx.dim, ctx.n)
        return gx, None, None


class _FftTruncFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dim, m_lo, m_hi):
        ext = _ext.get(required=True)
        ctx.dim, ctx.m_lo, ctx.m_hi, ctx.n = dim, m_lo, m_hi, x.shape[dim]
        return ext.dft_c2c(x.contiguous(), dim, ctx.n, m_lo, m_hi, True, 1.0)

    @staticmethod
    def backward(ctx, gy):
        # adjoint of (truncate . DFT) = conj-DFT of the zero-extended grad:
        # gx_j = sum_{k in kept} gY_k w^{+jk}  (inverse sign, no 1/n)
        ext = _ext.get(required=True)
        gx = ext.dft_c2c(gy.contiguous(), ctx.dim, ctx.n, ctx.m_lo, ctx.m_hi,
                         False, 1.0)
        return gx, None, None, None


class _PadIfftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, dim, n, m_lo, m_hi):
        ext = _ext.get(required=True)
        ctx.dim, ctx.n, ctx.m_lo, ctx.m_hi = dim, n, m_lo, m_hi
        return ext.dft_c2c(y.contiguous(), dim, n, m_lo, m_hi, False, 1.0 / n)

    @staticmethod
    def backward(ctx, gx):
        # adjoint: gY_k = (1/n) sum_j gx_j w^{-jk}, k in kept
        ext = _ext.get(required=True)
        gy = ext.dft_c2c(gx.contiguous(), ctx.dim, ctx.n, ctx.m_lo, ctx.m_hi,
                         True, 1.0 / ctx.n)
        return gy, None, None, None, None


class _PadIrfftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, dim, n_half, n_out, m, out_bf16):
        ext = _ext.get(required=True)
        ctx.dim, ctx.n_half, ctx.n_out, ctx.m = dim, n_half, n_out, m
        if out_bf16:
            return ext.dft_pad_irfft_bf16(y.contiguous(), dim, n_out, m)
        return ext.dft_pad_irfft(y.contiguous(), dim, n_out, m)

    @staticmethod
    def backward(ctx, gx):
        # gx may be bf16 (bf16 output config): the r2c adjoint stages and
        # converts it directly (no boundary cast)
        ext = _ext.get(required=True)
        gy = ext.dft_pad_irfft_adj(gx.contiguous(), ctx.dim, ctx.m)
        return gy, None, None, None, None, None


# ---------------------------------------------------------------------------
# fused residual-gradient accumulate (docs/ROADMAP.md item 4 tail)
# ---------------------------------------------------------------------------
#
# The block input feeds BOTH the spectral chain and the residual epilogue;
# the autograd engine would sum the two input gradients with a full-tensor
# aten add (~0.27 ms per block at the flagship).  Instead the epilogue-side
# gradient is STASHED (its fanout branch contributes None, so the engine
# never adds) and folded into the rfft adjoint's writeback, which is the
# LAST producer of the chain-side gradient.  A zero-size token from the
# rfft forward into the stash node makes the backward ordering a hard graph
# dependency: the stash backward must run before the rfft adjoint.
#
# A stash entry is either that gradient tensor or, from the fused irfft
# epilogue, the pair (gz, W): the adjoint kernel then applies W^T itself
# (rfft_adj_mix) and the gradient tensor never exists.

import itertools as _itertools

_GRAD_STASH = {}
_stash_keys = _itertools.count(1)


def new_stash_key() -> int:
    return next(_stash_keys)


class StashGradFn(torch.autograd.Function):
    """Alias ``x`` for a second consumer whose input-gradient is stashed
    (fused into the rfft adjoint) instead of engine-added."""

    @staticmethod
    def forward(ctx, x, tok, key):
        ctx.key = key
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        _GRAD_STASH[ctx.key] = g.contiguous()
        # None for x: the engine must NOT add this branch (the stashed value
        # is injected by _RfftTruncStashFn.backward); empty grad for tok
        # keeps the ordering edge alive.
        return None, torch.empty(0, device=g.device), None


class _RfftTruncStashFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dim, m, key):
        ext = _ext.get(required=True)
        ctx.dim, ctx.m, ctx.n, ctx.key = dim, m, x.shape[dim], key
        ctx.bf16 = x.dtype == torch.bfloat16
        y = ext.dft_rfft_trunc(x.contiguous(), dim, m)
        tok = torch.empty(0, device=x.device)
        return y, tok

    @staticmethod
    def backward(ctx, gy, gtok):
        ext = _ext.get(required=True)
        acc = _GRAD_STASH.pop(ctx.key, None)
        if acc is None:
            raise RuntimeError(
                "rfft stash: epilogue gradient missing (stash backward did "
                "not run before the rfft adjoint)")
        if isinstance(acc, tuple):
            # (gz, W) from the fused epilogue (ops/epilogue.py): the
            # residual grad-x W^T gz is applied inside the adjoint kernel
            gz, W = acc
            G = gy.contiguous()
            shape = list(G.shape)
            shape[-1] = ctx.n
            gx = ext.rfft_adj_mix(
                gz, W, G.reshape(gz.shape[0], W.shape[1], -1, ctx.m), ctx.n)
            gx = gx.reshape(shape)
        elif ctx.bf16:
            gx = ext.dft_rfft_trunc_adj_bf16(gy.contiguous(), ctx.dim,
                                             ctx.n, acc)
        else:
            gx = ext.dft_rfft_trunc_adj_acc(gy.contiguous(), ctx.dim,
                                            ctx.n, acc)
        return gx, None, None, None


def rfft_trunc_stash(x, dim, m, key):
    """Native rfft_trunc variant returning (y, ordering-token) whose adjoint
    adds the gradient stashed under ``key``.  Caller must route the block
    input's second use through ``block_epilogue(..., stash=(key, tok))``."""
    d = dim % x.dim()
    m = min(m, x.shape[d] // 2 + 1)
    return _RfftTruncStashFn.apply(x, d, m, key)


def stash_fusable(x, dim, m) -> bool:
    d = dim % x.dim()
    m = min(m, x.shape[d] // 2 + 1)
    if not (d == x.dim() - 1 and x.is_cuda and x.numel() > 0
            and torch.is_grad_enabled() and x.requires_grad
            and dft_caps_ok(x.shape[d], m)):
        return False
    if x.dtype == torch.bfloat16:
        # bf16 stash: bf16-IO r2c forward + bf16 adjoint with the packed
        # bf16 accumulate operand (the epilogue grad is bf16)
        return rfft_bf16_native_ok(x, d, m)
    return x.dtype in (torch.float32, torch.float64)


# ---------------------------------------------------------------------------
# fused (z,t) boundary 2-D transform (csrc/dft2d.hip)
# ---------------------------------------------------------------------------
#
# zt_fwd = fft_trunc(z) . rfft_trunc(t) and zt_inv = pad_irfft(t) .
# pad_ifft(z) in one plane-resident kernel each: the [L, Z, mt] complex
# intermediate of the two-pass chain (0.34 GB at the flagship, 16
# write+read passes per step over fwd/inv/adjoints) never exists.  The
# stash (residual-grad accumulate) folds into the adjoint's writeback like
# the 1-D c2r path.
#
# OFF BY DEFAULT (opt in with DFNO_ZT=1): measured on MI355X the fused
# kernels run ~600 us/call x 16 calls/step at the flagship while the 1-D
# chain they replace (r2c_glds 178 us + c2r_last 297 us + z-axis radix-8
# c2c, all traffic-bound) totals ~5.2 ms/step — a net loss of ~4 ms.  The
# direct z-contraction is VALU-issue-bound; the fusion only wins (~1 ms
# ceiling) with MFMA-tiled z-stages.  profiles/optimization_log.md has the
# numbers; the kernels stay correct + tested for that follow-up.

_ZT_EMPTY = {}


def _zt_empty(device):
    t = _ZT_EMPTY.get(device)
    if t is None:
        t = torch.empty(0, device=device)
        _ZT_EMPTY[device] = t
    return t


def zt_enabled() -> bool:
    """Fused (z,t) model-path gate (env DFNO_ZT=1; default off, see above)."""
    return os.environ.get("DFNO_ZT", "0") == "1"


def zt_caps_ok(dtype, Z, T, mz_lo, mz_hi, mt) -> bool:
    """The caps of csrc/dft2d.hip, stated once: real IO dtype (the spectrum
    side is complex64), plane extents and kept-mode counts.  Both kernels
    and every policy that must know whether they own the (z,t) transforms
    test this, next to ``zt_enabled()``."""
    return (dtype in (torch.float32, torch.bfloat16)
            and Z <= 64 and T <= 64 and mz_lo + mz_hi <= min(48, Z)
            and min(mt, T // 2 + 1) <= 32)


def zt_native_ok(x, mz_lo, mz_hi, mt) -> bool:
    return (x.is_cuda and x.dim() >= 2
            and zt_caps_ok(x.dtype, x.shape[-2], x.shape[-1],
                           mz_lo, mz_hi, mt))


class _ZtFwdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mz_lo, mz_hi, mt, stash_key):
        ext = _ext.get(required=True)
        ctx.dims = (x.shape[-2], x.shape[-1], mz_lo, mz_hi)
        ctx.bf16 = x.dtype == torch.bfloat16
        ctx.key = stash_key
        y = ext.dft_zt_fwd(x.contiguous(), mz_lo, mz_hi, mt, 1.0, False)
        if stash_key is not None:
            tok = torch.empty(0, device=x.device)
            return y, tok
        return y

    @staticmethod
    def backward(ctx, gy, *rest):
        ext = _ext.get(required=True)
        Z, T, mz_lo, mz_hi = ctx.dims
        acc = _zt_empty(gy.device)
        if ctx.key is not None:
            acc = _GRAD_STASH.pop(ctx.key, None)
            if acc is None:
                raise RuntimeError("zt stash: epilogue gradient missing")
        gx = ext.dft_zt_inv(gy.contiguous(), Z, T, mz_lo, mz_hi, 1.0, False,
                            ctx.bf16, acc if not ctx.bf16 else
                            _zt_empty(gy.device))
        return gx, None, None, None, None


class _ZtInvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, Z, T, mz_lo, mz_hi, out_bf16):
        ext = _ext.get(required=True)
        ctx.dims = (Z, T, mz_lo, mz_hi, y.shape[-1])
        x = ext.dft_zt_inv(y.contiguous(), Z, T, mz_lo, mz_hi,
                           1.0 / (Z * T), True, out_bf16, _zt_empty(y.device))
        return x

    @staticmethod
    def backward(ctx, gx):
        ext = _ext.get(required=True)
        Z, T, mz_lo, mz_hi, mt = ctx.dims
        gy = ext.dft_zt_fwd(gx.contiguous(), mz_lo, mz_hi, mt,
                            1.0 / (Z * T), True)
        return gy, None, None, None, None, None


def zt_fwd(x, mz_lo, mz_hi, mt, stash_key=None):
    """Fused truncated 2-D analysis over the trailing (z, t) dims."""
    mt = min(mt, x.shape[-1] // 2 + 1)
    return _ZtFwdFn.apply(x, mz_lo, mz_hi, mt, stash_key)


def zt_inv(y, Z, T, mz_lo, mz_hi, out_dtype=None):
    """Fused padded 2-D synthesis back to the (Z, T) extents."""
    out_bf16 = out_dtype == torch.bfloat16
    return _ZtInvFn.apply(y, Z, T, mz_lo, mz_hi, out_bf16)


# ---------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------

def rfft_bf16_native_ok(x, dim, m) -> bool:
    """bf16-IO r2c coverage (last dim, staged+converted at the LDS write)."""
    d = dim % x.dim()
    m = min(m, x.shape[d] // 2 + 1)
    return (d == x.dim() - 1 and x.is_cuda and x.dtype == torch.bfloat16
            and dft_caps_ok(x.shape[d], m))


def rfft_trunc(x, dim, m):
    d = dim % x.dim()
    # Clamp to the half-spectrum size: modes > n//2+1 keep the whole spectrum
    # (matches the reference's graceful [:m] slice, /root/reference/dfno/dfno.py:195).
    m = min(m, x.shape[d] // 2 + 1)
    if d == x.dim() - 1 and (rfft_bf16_native_ok(x, dim, m)
                             or _native_ok(x, x.shape[d], m, "rfft_trunc")):
        return _RfftTruncFn.apply(x, d, m)
    if x.is_cuda and d != x.dim() - 1:
        note_fallback("rfft_trunc", f"non-last transform dim {d}")
    if x.dtype == torch.bfloat16:
        x = x.float()   # torch.fft has no bf16 path
    return _t_rfft_trunc(x, dim, m)


def fft_trunc(x, dim, m_lo, m_hi):
    d = dim % x.dim()
    n = x.shape[d]
    m_lo = min(m_lo, n)
    m_hi = min(m_hi, n - m_lo)
    if _native_ok(x, n, m_lo + m_hi, "fft_trunc"):
        return _FftTruncFn.apply(x, d, m_lo, m_hi)
    return _t_fft_trunc(x, dim, m_lo, m_hi)


def pad_ifft(y, dim, n, m_lo, m_hi):
    d = dim % y.dim()
    m_lo = min(m_lo, n)
    m_hi = min(m_hi, n - m_lo)
    if _native_ok(y, n, m_lo + m_hi, "pad_ifft"):
        return _PadIfftFn.apply(y, d, n, m_lo, m_hi)
    return _t_pad_ifft(y, dim, n, m_lo, m_hi)


def pad_irfft(y, dim, n_half, n_out, m, out_dtype=None):
    d = dim % y.dim()
    m = min(m, n_half)
    if d == y.dim() - 1 and _native_ok(y, n_out, m, "pad_irfft"):
        out_bf16 = (out_dtype == torch.bfloat16
                    and y.dtype == torch.complex64)
        return _PadIrfftFn.apply(y, d, n_half, n_out, m, out_bf16)
    if y.is_cuda and d != y.dim() - 1:
        note_fallback("pad_irfft", f"non-last transform dim {d}")
    out = _t_pad_irfft(y, dim, n_half, n_out, m)
    if out_dtype is not None and out.dtype != out_dtype:
        out = out.to(out_dtype)
    return out
