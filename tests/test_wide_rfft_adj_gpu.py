"""Adjoint mode of the wide fused epilogue: ``rfft_adj_mix`` with more than
32 contracted channels (the MFMA wide mix of csrc/mix_wide.hip in its ``wt``
mode with the rfft adjoint synthesized as the addend), and the stash wiring
that feeds it at width 40.

Mirrors tests/test_fused_rfft_adj_gpu.py: the shape list is that of
tests/test_wide_epilogue_gpu.py with the roles swapped (the mix's O channels
are the contracted ones), the tolerances are that file's.  The model is not
routed here (``rfft_adj_mix_ok`` stays at 32 channels after the kernel lost
its A/B at the width-64 flagship shape), so the stash test hands the epilogue
op its key and token the way ``block_epilogue`` does inside the routed range.
``G`` is a full random complex tensor, so a kernel that applied ``pad_irfft``'s
factors (the forward mode's staging) is off by O(1)."""

import math

import pytest
import torch
import torch.nn.functional as F

from test_fused_rfft_adj_gpu import ADJ_TOL, _gw_tol
from test_wide_epilogue_gpu import SHAPES

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from dfno_amd import _ext
    return _ext.get(required=True)


@pytest.mark.parametrize("xshape,O,n,m", SHAPES)
def test_wide_rfft_adj_mix_vs_oracle(ext, xshape, O, n, m):
    from dfno_amd.ops.fft import _t_rfft_trunc
    from dfno_amd.ops.pointwise import _mix_bwd_x

    torch.manual_seed(31)
    B, I = xshape[0], xshape[1]
    S = math.prod(xshape[2:])
    L = S // n
    assert O > 32
    gz = torch.randn(B, O, S, device="cuda")
    W = torch.randn(O, I, device="cuda") / math.sqrt(I)
    G = torch.randn(B, I, *xshape[2:-1], m, device="cuda",
                    dtype=torch.complex64)
    assert G[..., 0].imag.abs().min() > 0
    G4 = G.reshape(B, I, L, m).contiguous()

    gx = ext.rfft_adj_mix(gz, W, G4, n)
    assert gx.shape == (B, I, S) and gx.dtype == torch.float32

    # torch oracle: autograd adjoint of the rfft + the transposed mix
    xr = torch.zeros(*xshape, device="cuda", requires_grad=True)
    _t_rfft_trunc(xr, -1, m).backward(G)
    ref = torch.einsum("oi,bos->bis", W, gz) + xr.grad.reshape(B, I, S)
    # the native pair this kernel replaces: the transposed wide mix, then the
    # rfft adjoint accumulated onto it
    pair = ext.dft_rfft_trunc_adj_acc(
        G4, 3, n,
        _mix_bwd_x(gz, W, "test").reshape(B, I, L, n)).reshape(B, I, S)
    print(f"vs torch {(gx - ref).abs().max():.3e} "
          f"vs native pair {(gx - pair).abs().max():.3e}")
    assert torch.allclose(gx, ref, **ADJ_TOL), f"{(gx - ref).abs().max()}"
    assert torch.allclose(gx, pair, **ADJ_TOL), f"{(gx - pair).abs().max()}"
    # no atomics: bitwise reproducible
    assert torch.equal(gx, ext.rfft_adj_mix(gz, W, G4, n))


def test_wide_autograd_stash(ext, monkeypatch):
    """The block's arrangement by hand at width 40: rfft_trunc_stash on x, a
    linear complex op on the spectrum, the fused epilogue fed by the stash."""
    from dfno_amd.ops.epilogue import _IrfftLinearResGeluFn
    from dfno_amd.ops.fft import (_GRAD_STASH, _t_pad_irfft, _t_rfft_trunc,
                                  new_stash_key, rfft_trunc_stash)

    torch.manual_seed(33)
    xshape, O, n, m = (1, 40, 3, 3, 5, 30), 40, 30, 8
    B, I = xshape[0], xshape[1]
    S = math.prod(xshape[2:])
    x0 = torch.randn(*xshape, device="cuda")
    W0 = torch.randn(O, I, device="cuda") / math.sqrt(I)
    A0 = torch.randn(1, O, *([1] * (len(xshape) - 3)), m, device="cuda",
                     dtype=torch.complex64) / n
    gy = torch.randn(B, O, *xshape[2:], device="cuda")

    calls = []
    orig = ext.rfft_adj_mix
    monkeypatch.setattr(ext, "rfft_adj_mix",
                        lambda *a: (calls.append(1), orig(*a))[1])
    monkeypatch.setenv("DFNO_FUSED_RFFT_ADJ", "1")
    x = x0.clone().requires_grad_(True)
    W = W0.clone().requires_grad_(True)
    A = A0.clone().requires_grad_(True)
    key = new_stash_key()
    Xs, tok = rfft_trunc_stash(x, -1, m, key)
    # block_epilogue's deferred grad-x arrangement: detached x, key and token
    # (once a wide mode is routed, go through irfft_linear_res_gelu(...,
    # stash=(key, tok)) so that block_epilogue's own choice is exercised)
    y = _IrfftLinearResGeluFn.apply(x.detach(), W, Xs * A, n, key, tok)
    y = y.reshape(gy.shape)
    y.backward(gy)
    torch.cuda.synchronize()
    assert len(calls) == 1, "fused adjoint not taken once"
    assert not _GRAD_STASH, "stash entry left behind"
    got = (y.detach(), x.grad, W.grad, A.grad)

    x = x0.clone().requires_grad_(True)
    W = W0.clone().requires_grad_(True)
    A = A0.clone().requires_grad_(True)
    Yt = _t_rfft_trunc(x, -1, m) * A
    z = (torch.einsum("oi,bis->bos", W, x.reshape(B, I, S))
         + _t_pad_irfft(Yt, -1, n // 2 + 1, n, m).reshape(B, O, S))
    yr = F.gelu(z).reshape(gy.shape)
    yr.backward(gy)
    ref = (yr.detach(), x.grad, W.grad, A.grad)

    d = [(a - b).abs().max().item() for a, b in zip(got, ref)]
    print(f"y {d[0]:.3e} gx {d[1]:.3e} gW {d[2]:.3e} gA {d[3]:.3e}")
    assert torch.allclose(got[0], ref[0], **ADJ_TOL), f"y {d[0]}"
    assert torch.allclose(got[1], ref[1], **ADJ_TOL), f"gx {d[1]}"
    assert torch.allclose(got[2], ref[2], **_gw_tol(S)), f"gW {d[2]}"
    assert torch.allclose(torch.view_as_real(got[3]),
                          torch.view_as_real(ref[3]), **ADJ_TOL), f"gA {d[3]}"
