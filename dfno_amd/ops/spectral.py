"""Fused corner-block complex spectral contraction (the FNO hot spot).

Replaces the reference's per-corner sliced complex einsum over a freshly
zeroed clone of the full truncated spectrum
(``y = 0*x.clone(); y[sl] = torch.einsum(eqn, x[sl], w)``,
/root/reference/dfno/dfno.py:269-271).

The contraction is, per kept frequency point f:
    y[b, o, f] = sum_i x[b, i, f] * w[i, o, f]
i.e. a width x width complex matvec batched over frequencies.  At batch 1 and
width ~20 this is HBM-bandwidth-bound on the *weight* stream (intensity
~1 flop/byte), so the native kernel is a streaming VALU kernel (complex64
with even innermost extents: two complex weights, 16 bytes, per lane and
load; one otherwise) with the corner-box gather/scatter fused into its
addressing — the truncated spectrum is touched exactly once and no
per-corner slices are materialized.  (An MFMA formulation does not pay here:
each weight element is used `batch` times only, far below the fp32 ridge.)

Autograd: grad_x[b,i,f] = sum_o conj(w[i,o,f]) gy[b,o,f] (same kernel,
conjugate-transposed weight); grad_w[i,o,f] = sum_b conj(x[b,i,f]) gy[b,o,f]
(``spectral_corners_bwd_w``: one thread per (corner, frequency, o), with the
corner gather fused into the addressing).

Deferred grad-W.  grad_w is a per-frequency outer product of two small
spectra, and at batch 1 the optimizer is its only reader.  When every corner
weight of a call belongs to one ``dfno_amd.optim.Adam`` (``register_corners``)
the backward does not build it: it hands ``(x, gy, starts, weights)`` to that
optimizer as a pending entry and returns ``None`` for the weights, and
``Adam.step()`` rebuilds the gradient in registers inside the update kernel
(``spectral_gradw_adam_``).  With such an optimizer ``.grad`` of the corner
weights is therefore ``None`` after ``backward()`` and post-accumulate hooks
on them do not fire; ``Adam.materialize_grads()`` writes the gradients out
for callers who inspect or clip them.  ``DFNO_FUSED_SPECTRAL_ADAM=0``
restores the eager gradient.
"""

from __future__ import annotations

import os
import weakref
from typing import List, Sequence, Tuple

import torch

from .. import _ext

__all__ = ["spectral_conv"]


def _corner_slices(bounds: Sequence[Tuple[int, int]]):
    return (slice(None), slice(None)) + tuple(slice(a, b) for a, b in bounds)


# ---------------------------------------------------------------------------
# fp8 (e4m3) spectral-weight quantization (BASELINE.json config #5).
#
# The contraction is weight-stream bandwidth-bound; storing the corner
# weights as OCP e4m3 (one byte per real/imag component, one fp32 scale per
# corner, amax/448 scaling) cuts that stream 4x.  The fp32/complex64 master
# weights keep training (straight-through: grad-W is computed against the
# master, forward/bwd-x use the quantized copy).  Quantized copies are cached
# and refreshed once per training step (``bump_quant_epoch`` from the model
# forward under grad mode); eval reuses the cache indefinitely.
# ---------------------------------------------------------------------------

_E4M3_MAX = 448.0
_QUANT_EPOCH = [0]
_FP8_CACHE = {}   # id(w) -> (epoch, w16, scale)


def bump_quant_epoch() -> None:
    _QUANT_EPOCH[0] += 1
    # evict entries whose master stopped refreshing (model freed): live
    # masters touch their entry every epoch, so a lag > 8 means the id is
    # dead and its e4m3/amax buffers would otherwise pin GPU memory forever
    if _QUANT_EPOCH[0] % 64 == 0:
        cutoff = _QUANT_EPOCH[0] - 8
        for k in [k for k, ent in _FP8_CACHE.items() if ent[0] < cutoff]:
            del _FP8_CACHE[k]


def _fp8_weights(weights):
    """Quantized (w16, amax) device pairs for each master, requantized at
    most once per quant epoch by ONE fused amax+encode kernel pair over all
    stale corners — no host sync anywhere on the path."""
    from .. import _ext
    stale, stale16, stale_am = [], [], []
    for w in weights:
        ent = _FP8_CACHE.get(id(w))
        if ent is not None and (ent[1].shape != w.shape
                                or ent[1].device != w.device):
            ent = None   # id() reuse after a freed master (fresh models)
        if ent is None:
            w16 = torch.empty(w.shape, dtype=torch.uint16, device=w.device)
            amax = torch.zeros(1, dtype=torch.float32, device=w.device)
            ent = [-1, w16, amax]
            _FP8_CACHE[id(w)] = ent
        if ent[0] != _QUANT_EPOCH[0]:
            ent[0] = _QUANT_EPOCH[0]
            stale.append(w.detach().contiguous())
            stale16.append(ent[1])
            stale_am.append(ent[2])
    if stale:
        ext = _ext.get(required=True)
        for i in range(0, len(stale), 64):
            ext.fp8_quant_corners(stale[i:i + 64], stale16[i:i + 64],
                                  stale_am[i:i + 64])
    out16 = [_FP8_CACHE[id(w)][1] for w in weights]
    amaxes = [_FP8_CACHE[id(w)][2] for w in weights]
    return out16, amaxes


def dequantize_fp8(w16: torch.Tensor, amax) -> torch.Tensor:
    """Reference dequant (tests): uint16 packed pairs -> complex64."""
    if isinstance(amax, torch.Tensor):
        scale = float(amax.clamp_min(1e-30)) / _E4M3_MAX
    else:
        scale = float(amax)
    w8 = w16.unsqueeze(-1).view(torch.uint8).view(torch.float8_e4m3fn)
    return torch.view_as_complex(w8.to(torch.float32) * scale)


# ---------------------------------------------------------------------------
# deferred grad-W: which optimizer owns which corner weight
# ---------------------------------------------------------------------------

CORNER_TAG = "_dfno_spectral_corner"   # set by DistributedFNOBlock
_CORNER_OWNER = {}   # id(w) -> (weakref(w), weakref(optimizer))


def fused_spectral_adam_enabled() -> bool:
    return os.environ.get("DFNO_FUSED_SPECTRAL_ADAM", "1") != "0"


def register_corners(optimizer, params) -> None:
    """Record ``optimizer`` as the owner of the tagged complex64 corner
    weights among ``params`` (weakly: neither side is kept alive)."""
    dead = [k for k, (wr, orf) in _CORNER_OWNER.items()
            if wr() is None or orf() is None]
    for k in dead:
        del _CORNER_OWNER[k]
    for p in params:
        if getattr(p, CORNER_TAG, False) and p.dtype == torch.complex64:
            _CORNER_OWNER[id(p)] = (weakref.ref(p), weakref.ref(optimizer))


def _corner_owner(weights):
    """The live optimizer every one of ``weights`` is registered with, or
    None."""
    owner = None
    for w in weights:
        ent = _CORNER_OWNER.get(id(w))
        if ent is None or ent[0]() is not w:
            return None
        opt = ent[1]()
        if opt is None or (owner is not None and opt is not owner):
            return None
        owner = opt
    return owner


def corner_grads(x, gy, bounds_list, weights):
    """grad-W of every corner: the native kernel on GPU (in_channels <= 64),
    the einsum otherwise."""
    if (gy.is_cuda and gy.numel() > 0 and x.shape[1] <= 64
            and gy.dtype in (torch.complex64, torch.complex128)):
        ext = _ext.get(required=True)
        gws = [torch.empty_like(w) for w in weights]
        ext.spectral_corners_bwd_w(
            x.contiguous(), gy, gws,
            [[a for a, _ in bounds] for bounds in bounds_list])
        return gws
    gws = []
    for w, bounds in zip(weights, bounds_list):
        sl = _corner_slices(bounds)
        gws.append(torch.einsum("bo...,bi...->io...", gy[sl], x[sl].conj()))
    return gws


class _SpectralConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: torch.Tensor, bounds_list, out_channels: int,
                fp8: bool, *weights: torch.Tensor):
        B, I = x.shape[0], x.shape[1]
        fdims = list(x.shape[2:])
        ctx.fp8 = fp8 = bool(fp8 and x.is_cuda and x.dtype == torch.complex64)
        y = torch.zeros((B, out_channels, *fdims), dtype=x.dtype, device=x.device)
        if fp8 and x.numel() > 0:
            ext = _ext.get(required=True)
            xc = x.contiguous()
            w16s, scales = _fp8_weights(weights)
            ext.spectral_corners_fwd_fp8(
                xc, w16s, scales, y,
                [[a for a, _ in bounds] for bounds in bounds_list])
            ctx.fp8_wq = (w16s, scales)
            x_saved = xc
        elif x.is_cuda and x.numel() > 0 and x.dtype in (torch.complex64, torch.complex128):
            ext = _ext.get(required=True)
            xc = x.contiguous()
            ext.spectral_corners_fwd(
                xc, [w.contiguous() for w in weights], y,
                [[a for a, _ in bounds] for bounds in bounds_list])
            x_saved = xc
        else:
            if x.is_cuda and x.numel() > 0:
                from ..dispatch import note_fallback
                note_fallback("spectral_conv", f"dtype {x.dtype} not complex64/128")
            x_saved = x
            for w, bounds in zip(weights, bounds_list):
                sl = _corner_slices(bounds)
                y[sl] = torch.einsum("bi...,io...->bo...", x[sl], w)
        ctx.save_for_backward(x_saved, *weights)
        ctx.bounds_list = bounds_list
        # the Parameter objects themselves (saved tensors may be unpacked
        # into new objects), kept only where a deferral is possible at all
        ctx.corner_params = (
            weights if weights and not fp8 and x.dtype == torch.complex64
            and _corner_owner(weights) is not None else None)
        return y

    @staticmethod
    def _deferral_owner(ctx, x):
        """The optimizer that takes this call's grad-W as a pending entry, or
        None when the gradient has to be built now."""
        params = ctx.corner_params
        if params is None or not fused_spectral_adam_enabled():
            return None
        if torch.is_grad_enabled() or x.shape[1] > 64:   # create_graph
            return None
        if not all(ctx.needs_input_grad[4:]):
            return None
        opt = _corner_owner(params)
        if opt is None:
            return None
        if opt.has_pending(params):
            # a second backward before step(): autograd has to accumulate,
            # so the first gradient is written out and this one follows it
            opt.materialize_grads()
            return None
        for w in params:
            ent = _FP8_CACHE.get(id(w))
            if w.grad is not None or (ent is not None
                                      and ent[1].shape == w.shape
                                      and ent[1].device == w.device):
                return None   # accumulate / keep the e4m3 side table path
        return opt if opt.accepts_deferred(params) else None

    @staticmethod
    def backward(ctx, gy: torch.Tensor):
        x = ctx.saved_tensors[0]
        weights = ctx.saved_tensors[1:]
        bounds_list = ctx.bounds_list
        gy = gy.contiguous()
        gx = torch.zeros_like(x)
        gws = []
        owner = _SpectralConvFn._deferral_owner(ctx, x)
        if owner is not None:
            gws = [None] * len(weights)
        if gy.is_cuda and gy.numel() > 0 and gy.dtype in (torch.complex64, torch.complex128):
            ext = _ext.get(required=True)
            starts = [[a for a, _ in bounds] for bounds in bounds_list]
            if getattr(ctx, "fp8", False):
                w16s, scales = ctx.fp8_wq
                ext.spectral_corners_bwd_x_fp8(gy, w16s, scales, gx, starts)
            else:
                ext.spectral_corners_bwd_x(
                    gy, [w.contiguous() for w in weights], gx, starts)
            if owner is None:
                if x.shape[1] > 64:
                    from ..dispatch import note_fallback
                    note_fallback("spectral_corners_bwd_w",
                                  f"in_channels {x.shape[1]} > 64 (einsum grad-W)")
                gws = corner_grads(x, gy, bounds_list, weights)
        else:
            for w, bounds in zip(weights, bounds_list):
                sl = _corner_slices(bounds)
                gx[sl] = torch.einsum("bo...,io...->bi...", gy[sl], w.conj())
            if owner is None:
                gws = corner_grads(x, gy, bounds_list, weights)
        if owner is not None:
            owner.add_pending(x, gy, bounds_list, ctx.corner_params)
        return (gx, None, None, None, *gws)


def spectral_conv(x: torch.Tensor, weights: List[torch.Tensor],
                  bounds_list: List[List[Tuple[int, int]]],
                  out_channels: int = None, fp8: bool = False) -> torch.Tensor:
    """Apply the corner-block spectral contraction.

    x: [B, I, *F] complex; weights[c]: [I, O, *box_c] complex;
    bounds_list[c]: per-frequency-dim (start, stop) of corner c within F.
    fp8: read the weights through their cached e4m3 quantization (the fp32
    masters keep the gradients — straight-through).
    Returns [B, O, *F] with zeros outside the corner boxes.
    """
    if out_channels is None:
        out_channels = weights[0].shape[1] if weights else x.shape[1]
    return _SpectralConvFn.apply(x, bounds_list, out_channels, fp8, *weights)
