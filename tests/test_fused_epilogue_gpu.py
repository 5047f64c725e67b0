"""Fused irfft + residual-linear + gelu block epilogue (csrc/epilogue.hip,
ops/epilogue.py) vs the torch composition, and the model-level A/B of the
DFNO_FUSED_EPILOGUE knob.

Tolerances are the fp32 ones of tests/test_kernels_gpu.py: test_dft_pad_irfft
(rtol 2e-4, atol 2e-3) for everything downstream of the synthesis, and
test_channel_mix_bwd_fused's (2e-4 / 2e-4 for gx, S-scaled for gW)."""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

IRFFT_TOL = dict(rtol=2e-4, atol=2e-3)      # test_dft_pad_irfft, complex64
MIX_TOL = dict(rtol=2e-4, atol=2e-4)        # test_channel_mix_bwd_fused gx/gz

SHAPES = [
    # x shape,            O,  n_out, m
    ((1, 20, 4, 3, 5, 30), 20, 30, 8),   # pinned path, S%4==0, chunks straddle lines
    ((1, 20, 3, 3, 5, 30), 20, 30, 8),   # S%4==2, 45 lines (2 tiles + tail)
    ((2, 4, 7, 17), 6, 17, 3),           # odd N, B>1, I != O
    ((2, 8, 5, 14), 12, 14, 8),          # Nyquist bin kept
    ((1, 20, 257, 30), 20, 30, 8),       # line count not a tile multiple
]


def _inputs(xshape, O, n_out, m):
    torch.manual_seed(21)
    I = xshape[1]
    x = torch.randn(*xshape, device="cuda")
    W = torch.randn(O, I, device="cuda") / math.sqrt(I)
    # random complex spectrum: the imaginary parts of k=0 (and of the
    # Nyquist bin where kept) are non-zero and must be ignored
    yshape = (xshape[0], O, *xshape[2:-1], m)
    Y = torch.randn(*yshape, device="cuda", dtype=torch.complex64)
    gy = torch.randn(xshape[0], O, *xshape[2:], device="cuda")
    return x, W, Y, gy


@pytest.mark.parametrize("xshape,O,n_out,m", SHAPES)
def test_fused_epilogue_vs_torch(xshape, O, n_out, m):
    from dfno_amd import _ext
    from dfno_amd.ops import irfft_linear_res_gelu
    from dfno_amd.ops.fft import _t_pad_irfft

    ext = _ext.get(required=True)
    n_half = n_out // 2 + 1
    x, W, Y, gy = _inputs(xshape, O, n_out, m)
    B, I = xshape[0], xshape[1]
    S = x.numel() // (B * I)

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


def _run_model(knob, monkeypatch):
    import dfno_amd as dfno
    from dfno_amd import dispatch

    monkeypatch.setenv("DFNO_FUSED_EPILOGUE", knob)
    dispatch.reset_fallbacks()
    device = torch.device("cuda:0")
    torch.manual_seed(3)
    _, P_x, _ = dfno.create_standard_partitions((1, 1, 1, 1, 1, 1))
    model = dfno.DistributedFNONd(P_x, [1, 2, 8, 8, 8, 1], 10, 20,
                                  (2, 2, 2, 3), num_blocks=2, device=device,
                                  dtype=torch.float32)
    torch.manual_seed(4)
    x = torch.rand(1, 2, 8, 8, 8, 1, device=device)
    with torch.no_grad():
        y_ng = model(x)
    y = model(x)
    tgt = torch.rand_like(y)
    dfno.DistributedRelativeLpLoss(P_x)(y, tgt).backward()
    torch.cuda.synchronize()
    dispatch.assert_all_native()
    assert torch.equal(y_ng, y.detach()), "no-grad forward != grad-mode forward"
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()
             if p.grad is not None}
    return y.detach().clone(), grads


def test_model_knob_on_off(monkeypatch):
    import dfno_amd.ops.epilogue as epi

    calls = []
    orig = epi._IrfftLinearResGeluFn.apply

    def counting(*a):
        calls.append(1)
        return orig(*a)

    monkeypatch.setattr(epi._IrfftLinearResGeluFn, "apply", counting)
    y_on, g_on = _run_model("1", monkeypatch)
    n_on = len(calls)
    y_off, g_off = _run_model("0", monkeypatch)
    # 2 blocks x (no-grad + grad forward) fused; none with the knob off
    assert n_on == 4 and len(calls) == n_on

    print(f"y {(y_on - y_off).abs().max():.3e}")
    assert torch.allclose(y_on, y_off, **IRFFT_TOL), \
        f"y {(y_on - y_off).abs().max()}"
    assert g_on.keys() == g_off.keys() and g_on
    for n in g_on:
        a, b = g_on[n], g_off[n]
        if a.is_complex():
            a, b = torch.view_as_real(a), torch.view_as_real(b)
        print(f"{n} {(a - b).abs().max():.3e}")
        assert torch.allclose(a, b, **IRFFT_TOL), \
            f"{n} {(a - b).abs().max()}"
