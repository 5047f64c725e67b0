"""Fused irfft block epilogue at 33 to 64 input channels: the MFMA wide mix
(csrc/mix_wide.hip) with the time-axis synthesis as its addend, reached
through ``irfft_linear_res_gelu_fwd`` and the autograd op.

The model is not routed here (the kernel lost its A/B at the width-64 flagship
shape, see ``fused_epilogue_ok``), so the autograd op is taken directly:
``_IrfftLinearResGeluFn.apply``, which is what ``irfft_linear_res_gelu`` calls
inside the routed range.

Oracle and tolerances are those of tests/test_fused_epilogue_gpu.py: einsum +
``_t_pad_irfft`` + ``F.gelu`` with autograd for the gradients; IRFFT_TOL
downstream of the synthesis, MIX_TOL for gx, the S-scaled one for gW.  With
randn inputs and W ~ randn / sqrt(I) a dropped channel is an error near
1/sqrt(64) ~ 0.12 and a dropped or undoubled mode one near 2/N >= 0.03, both
more than ten times the atol."""

import math

import pytest
import torch
import torch.nn.functional as F

from test_fused_epilogue_gpu import IRFFT_TOL, MIX_TOL

pytestmark = pytest.mark.gpu

SHAPES = [
    # x shape,              O,  n_out, m
    ((1, 33, 3, 3, 5, 30), 33, 30, 8),   # K padded to 36, one live row in the
                                         # third row group, S%4==2, 45 lines
    ((1, 64, 4, 3, 5, 30), 64, 30, 8),   # full width, vector variant
    ((2, 40, 7, 17), 48, 17, 3),         # odd N, B=2 with odd S, I != O
    ((2, 64, 5, 14), 33, 14, 8),         # Nyquist bin kept, O < I
    ((1, 48, 2, 17), 48, 17, 3),         # S = 34, below one tile
    ((1, 33, 3, 64), 33, 64, 32),        # the caps of N and m
    ((1, 64, 257, 30), 64, 30, 8),       # many tiles, ragged last one
    # The grid is capped at 1024 blocks: past 1024 tiles a block runs its tile
    # loop again, with the spectrum tile staged over the dead x rows, the
    # next tile's rows prefetched in registers across the synthesis and the
    # closing barrier between the two.  2063 tiles: every block loops.
    ((1, 64, 4400, 30), 64, 30, 8),      # vector variant
    ((1, 33, 4401, 30), 33, 30, 8),      # S%4==2: the per-element variant,
                                         # K..K4 pad rows re-zeroed per tile
    # 64 rows of three 32-mode lines do not fit the x tile: the spectrum tile
    # lives in dynamic LDS, 104 KiB per block with the static tiles
    ((1, 64, 3, 62), 64, 62, 32),
]


def _inputs(xshape, O, n_out, m):
    torch.manual_seed(21)
    I = xshape[1]
    x = torch.randn(*xshape, device="cuda")
    W = torch.randn(O, I, device="cuda") / math.sqrt(I)
    # fully random complex spectrum: the imaginary parts of k=0 (and of the
    # Nyquist bin where kept) are non-zero and must be ignored
    yshape = (xshape[0], O, *xshape[2:-1], m)
    Y = torch.randn(*yshape, device="cuda", dtype=torch.complex64)
    gy = torch.randn(xshape[0], O, *xshape[2:], device="cuda")
    return x, W, Y, gy


@pytest.mark.parametrize("xshape,O,n_out,m", SHAPES)
def test_wide_epilogue_vs_torch(xshape, O, n_out, m):
    from dfno_amd import _ext
    from dfno_amd.ops.epilogue import _IrfftLinearResGeluFn
    from dfno_amd.ops.fft import _t_pad_irfft

    def irfft_linear_res_gelu(x, W, Y, n_half, n_out, m):
        out = _IrfftLinearResGeluFn.apply(x, W, Y, n_out)
        return out.reshape(x.shape[0], W.shape[0], *x.shape[2:])

    ext = _ext.get(required=True)
    n_half = n_out // 2 + 1
    x, W, Y, gy = _inputs(xshape, O, n_out, m)
    B, I = xshape[0], xshape[1]
    S = x.numel() // (B * I)
    assert I > 32

    # oracle
    xr = x.clone().requires_grad_(True)
    Wr = W.clone().requires_grad_(True)
    Yr = Y.clone().requires_grad_(True)
    z_ref = (torch.einsum("oi,bis->bos", Wr, xr.reshape(B, I, S))
             + _t_pad_irfft(Yr, -1, n_half, n_out, m).reshape(B, O, S))
    y_ref = F.gelu(z_ref)
    y_ref.backward(gy.reshape(B, O, S))

    # raw kernel: y and z, and need_z=False bit-identical y
    Y4 = Y.reshape(B, O, S // n_out, m).contiguous()
    y_k, z_k = ext.irfft_linear_res_gelu_fwd(x.reshape(B, I, S), W, Y4,
                                             n_out, True)
    y_n, z_n = ext.irfft_linear_res_gelu_fwd(x.reshape(B, I, S), W, Y4,
                                             n_out, False)
    assert z_n.numel() == 0
    assert torch.equal(y_k, y_n)
    print(f"y {(y_k - y_ref).abs().max():.3e} z {(z_k - z_ref).abs().max():.3e}")
    assert torch.allclose(z_k, z_ref, **IRFFT_TOL), \
        f"z {(z_k - z_ref).abs().max()}"
    assert torch.allclose(y_k, y_ref, **IRFFT_TOL), \
        f"y {(y_k - y_ref).abs().max()}"

    # autograd op
    xa = x.clone().requires_grad_(True)
    Wa = W.clone().requires_grad_(True)
    Ya = Y.clone().requires_grad_(True)
    y = irfft_linear_res_gelu(xa, Wa, Ya, n_half, n_out, m)
    assert y.shape == gy.shape
    assert torch.equal(y.reshape(B, O, S), y_k)
    y.backward(gy)
    print(f"gx {(xa.grad - xr.grad).abs().max():.3e} "
          f"gW {(Wa.grad - Wr.grad).abs().max():.3e} "
          f"gY {(Ya.grad - Yr.grad).abs().max():.3e}")
    assert torch.allclose(xa.grad, xr.grad, **MIX_TOL), \
        f"gx {(xa.grad - xr.grad).abs().max()}"
    scale = max(1, S // 4096)
    assert torch.allclose(Wa.grad, Wr.grad, rtol=1e-4 * scale,
                          atol=1e-3 * scale), \
        f"gW {(Wa.grad - Wr.grad).abs().max()}"
    assert torch.allclose(Ya.grad, Yr.grad, **IRFFT_TOL), \
        f"gY {(Ya.grad - Yr.grad).abs().max()}"

    # no-grad forward (need_z=False inside) equals the grad-mode forward
    with torch.no_grad():
        y0 = irfft_linear_res_gelu(x, W, Y, n_half, n_out, m)
    assert torch.equal(y0, y.detach())
