"""Last-dim r2c (csrc/dft.hip) on a tensor that does not end on a 16-byte
packet.

The LDS-DMA kernel fills its ring by whole packets and clamps the last tile's
packets into the tensor; a packet that straddles the end was moved back by a
part of itself, so the last line was staged shifted (error 0.12 in its modes).
``launch_r2c`` takes the staged kernel for such tensors.  Reference and
tolerance are those of test_dft_pad_irfft in tests/test_kernels_gpu.py
(rtol 2e-4, atol 2e-3): the torch composition through autograd."""

import pytest
import torch

pytestmark = pytest.mark.gpu

IRFFT_TOL = dict(rtol=2e-4, atol=2e-3)


@pytest.mark.parametrize("lines,n,m", [(1485, 30, 8), (7, 30, 8), (33, 17, 3)])
def test_pad_irfft_adj_odd_total(lines, n, m):
    from dfno_amd import _ext
    from dfno_amd.ops.fft import _t_pad_irfft

    ext = _ext.get(required=True)
    assert (lines * n) % 4 != 0
    torch.manual_seed(22)
    g = torch.randn(1, 1, lines, n, device="cuda")
    Y = torch.zeros(1, 1, lines, m, device="cuda", dtype=torch.complex64,
                    requires_grad=True)
    _t_pad_irfft(Y, -1, n // 2 + 1, n, m).backward(g)
    got = ext.dft_pad_irfft_adj(g, 3, m)
    print(f"gY {(got - Y.grad).abs().max():.3e} "
          f"last line {(got[..., -1, :] - Y.grad[..., -1, :]).abs().max():.3e}")
    assert torch.allclose(got, Y.grad, **IRFFT_TOL)


@pytest.mark.parametrize("lines,n,m", [(1485, 30, 8), (33, 17, 3)])
def test_rfft_trunc_odd_total(lines, n, m):
    from dfno_amd import _ext
    from dfno_amd.ops.fft import _t_rfft_trunc

    ext = _ext.get(required=True)
    torch.manual_seed(23)
    x = torch.randn(1, 1, lines, n, device="cuda")
    got = ext.dft_rfft_trunc(x, 3, m)
    ref = _t_rfft_trunc(x, -1, m)
    assert torch.allclose(torch.view_as_real(got), torch.view_as_real(ref),
                          **IRFFT_TOL), f"{(got - ref).abs().max()}"
