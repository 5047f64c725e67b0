"""Kernel-level tests of the width 33..128 routes: the wide channel mix
(csrc/mix_wide.hip), grad-W up to 64 input channels, spectral grad-W up to 64.

References are torch.einsum on fp32-upcast inputs.  Tolerances are the
project's: fp32 rtol = atol = 2e-5 (test_kernels_gpu.tol) with W ~ randn /
sqrt(I); bf16 BT = 2**-7 (test_bf16_gpu) with that file's input scaling.
"""

import math

import pytest
import torch
import torch.nn.functional as F

from dfno_amd import dispatch

pytestmark = pytest.mark.gpu

BT = 2 ** -7
F32 = dict(rtol=2e-5, atol=2e-5)

# (B, I, O, S, bias, res, act, wt, need_z); I is always the contraction depth
# and O the output rows, wt hands the kernel W as [I, O] (the grad-x form)
FWD_CASES = [
    (1, 33, 33, 64, False, True, True, False, True),     # one over the cap, one tile
    (2, 64, 64, 515, False, True, True, False, True),    # unaligned 2nd batch row, tail
    (1, 48, 40, 5, True, False, False, False, False),    # fewer columns than a wave
    (1, 64, 128, 264, True, False, True, False, True),   # linear3, O at its maximum
    (1, 128, 64, 264, False, False, False, True, False),  # its grad-x: K at its maximum
    (1, 36, 64, 1024, False, False, False, False, False),  # plain, z not requested
    (2, 40, 40, 70001, False, True, True, False, True),  # blocks walk several tiles
]
BF16_S = [64, 520, 8, 264, 264, 1024, 70008]


def _ext():
    from dfno_amd import _ext as e
    return e.get(required=True)


def _ref(x, W, b, r, act):
    z = torch.einsum("oi,bis->bos", W.float(), x.float())
    if b is not None:
        z = z + b.float().view(1, -1, 1)
    if r is not None:
        z = z + r.float()
    return (F.gelu(z) if act else z), z


@pytest.mark.parametrize("B,I,O,S,bias,res,act,wt,need_z", FWD_CASES)
def test_wide_mix_fwd_fp32(B, I, O, S, bias, res, act, wt, need_z):
    ext = _ext()
    torch.manual_seed(0)
    x = torch.randn(B, I, S, device="cuda")
    W = torch.randn(O, I, device="cuda") / math.sqrt(I)
    e = torch.empty(0, device="cuda")
    b = torch.randn(O, device="cuda") if bias else None
    r = torch.randn(B, O, S, device="cuda") if res else None
    y, z = ext.wide_channel_mix(x, W.t().contiguous() if wt else W,
                                b if bias else e, r if res else e, act, wt, need_z)
    y_ref, z_ref = _ref(x, W, b, r, act)
    assert y.shape == (B, O, S)
    assert torch.allclose(y, y_ref, **F32), f"max {(y - y_ref).abs().max()}"
    if need_z:
        assert torch.allclose(z, z_ref, **F32), f"max {(z - z_ref).abs().max()}"
    else:
        assert z.numel() == 0


@pytest.mark.parametrize("case,S", list(zip(FWD_CASES, BF16_S)))
def test_wide_mix_fwd_bf16(case, S):
    B, I, O, _, bias, res, act, wt, need_z = case
    ext = _ext()
    torch.manual_seed(4)
    x = (torch.rand(B, I, S, device="cuda") - 0.5).bfloat16()
    W = ((torch.rand(O, I, device="cuda") - 0.5) / I).bfloat16()
    e = torch.empty(0, dtype=torch.bfloat16, device="cuda")
    b = (torch.rand(O, device="cuda") - 0.5).bfloat16() if bias else None
    r = (torch.rand(B, O, S, device="cuda") - 0.5).bfloat16() if res else None
    y, z = ext.wide_channel_mix(x, W.t().contiguous() if wt else W,
                                b if bias else e, r if res else e, act, wt, need_z)
    y_ref, z_ref = _ref(x, W, b, r, act)
    assert y.shape == (B, O, S) and y.dtype == torch.bfloat16
    assert torch.allclose(y.float(), y_ref, rtol=BT, atol=BT), \
        f"max {(y.float() - y_ref).abs().max()}"
    if need_z:
        assert torch.allclose(z.float(), z_ref, rtol=BT, atol=BT)
    else:
        assert z.numel() == 0


def test_wide_mix_refuses_out_of_range():
    ext = _ext()
    e = torch.empty(0, device="cuda")
    for I, O in ((20, 20), (32, 32), (129, 64)):
        x = torch.zeros(1, I, 64, device="cuda")
        W = torch.zeros(O, I, device="cuda")
        with pytest.raises(RuntimeError, match="wide_channel_mix"):
            ext.wide_channel_mix(x, W, e, e, False, False, False)
    xb = torch.zeros(1, 64, 12, device="cuda", dtype=torch.bfloat16)
    Wb = torch.zeros(64, 64, device="cuda", dtype=torch.bfloat16)
    eb = torch.empty(0, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="wide_channel_mix"):
        ext.wide_channel_mix(xb, Wb, eb, eb, False, False, False)


def test_linear_res_gelu_fp64_wide_composes():
    """fp64 past 32 input channels with a residual: the LDS-path mix plus
    add_gelu, no raise and no fallback note."""
    from dfno_amd.ops.pointwise import linear_res_gelu
    dispatch.reset_fallbacks()
    torch.manual_seed(1)
    B, I, O, S = 2, 40, 40, 131
    x = torch.randn(B, I, S, device="cuda", dtype=torch.float64, requires_grad=True)
    W = (torch.randn(O, I, device="cuda", dtype=torch.float64) / math.sqrt(I)
         ).requires_grad_()
    r = torch.randn(B, O, S, device="cuda", dtype=torch.float64, requires_grad=True)
    y = linear_res_gelu(x, W, r)
    gy = torch.randn_like(y)
    y.backward(gy)
    xc, Wc, rc = (t.detach().cpu().requires_grad_() for t in (x, W, r))
    yc = F.gelu(torch.einsum("oi,bis->bos", Wc, xc) + rc)
    yc.backward(gy.cpu())
    t = dict(rtol=1e-11, atol=1e-11)
    assert torch.allclose(y.detach().cpu(), yc.detach(), **t)
    assert torch.allclose(x.grad.cpu(), xc.grad, **t)
    assert torch.allclose(r.grad.cpu(), rc.grad, **t)
    assert torch.allclose(W.grad.cpu(), Wc.grad, rtol=1e-11, atol=1e-9)
    assert not dispatch.fallback_counts()


# ---------------------------------------------------------------------------
# grad-W
# ---------------------------------------------------------------------------

def _gw_tol32(ref):
    return dict(rtol=1e-4, atol=float(ref.abs().max()) * 1e-5)


@pytest.mark.parametrize("B,I,O,S,bias", [
    (1, 64, 64, 4096, False),    # MFMA route, 64 x rows
    (2, 40, 33, 1001, True),     # unaligned generic route, two i-slabs
    (1, 33, 128, 4096, False),   # MFMA route, one row into the second slab
    (1, 64, 128, 4096, True),    # linear3: MFMA route, bias as the ones column
    (2, 33, 40, 256, True),      # the same with ragged i- and o-tiles
])
def test_wide_grad_w_fp32(B, I, O, S, bias):
    ext = _ext()
    torch.manual_seed(3)
    gz = torch.randn(B, O, S, device="cuda")
    x = torch.randn(B, I, S, device="cuda")
    gW, gb = ext.channel_mix_bwd_w(gz, x, bias)
    refW = torch.einsum("bos,bis->oi", gz, x)
    assert gW.shape == (O, I)
    assert torch.allclose(gW, refW, **_gw_tol32(refW)), \
        f"max {(gW - refW).abs().max()}"
    if bias:
        refb = gz.sum(dim=(0, 2))
        assert torch.allclose(gb, refb, **_gw_tol32(refW))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_wide_grad_w_role_swap(dtype):
    """linear4's grad-W (128 -> 1, with bias) through the host dispatch: the
    existing reduction with the roles swapped."""
    from dfno_amd.ops.pointwise import _mix_bwd_w
    dispatch.reset_fallbacks()
    torch.manual_seed(5)
    B, I, O, S = 2, 128, 1, 777
    gz = torch.randn(B, O, S, device="cuda", dtype=dtype)
    x = torch.randn(B, I, S, device="cuda", dtype=dtype)
    W = torch.zeros(O, I, device="cuda", dtype=dtype)
    gW, gb = _mix_bwd_w(gz, x, W, True)
    refW = torch.einsum("bos,bis->oi", gz, x)
    refb = gz.sum(dim=(0, 2))
    t = _gw_tol32(refW) if dtype == torch.float32 else dict(rtol=1e-11, atol=1e-9)
    assert gW.shape == (O, I) and gW.is_contiguous()
    assert torch.allclose(gW, refW, **t), f"max {(gW - refW).abs().max()}"
    assert torch.allclose(gb, refb, **t)
    assert not dispatch.fallback_counts()


@pytest.mark.parametrize("B,I,O,S,bias", [
    (1, 64, 64, 4096, True),     # MFMA, 16 tile pairs
    (2, 48, 128, 512, False),    # MFMA, 24 tile pairs
    (1, 40, 24, 384, True),      # S % 256 != 0: the LDS-tiled kernel, 64 x rows
])
def test_wide_grad_w_bf16(B, I, O, S, bias):
    ext = _ext()
    torch.manual_seed(2)
    gz = (torch.rand(B, O, S, device="cuda") - 0.5).bfloat16()
    x = (torch.rand(B, I, S, device="cuda") - 0.5).bfloat16()
    gW, gb = ext.bf16_channel_mix_bwd_w(gz, x, bias)
    refW = torch.einsum("bos,bis->oi", gz.float(), x.float())
    assert torch.allclose(gW, refW, rtol=2e-3, atol=refW.abs().max() * 2e-3), \
        f"max {(gW - refW).abs().max()}"
    if bias:
        refb = gz.float().sum(dim=(0, 2))
        assert torch.allclose(gb, refb, rtol=2e-3, atol=refb.abs().max() * 2e-3)


# ---------------------------------------------------------------------------
# spectral conv at 33 and 64 channels
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("cdtype", [torch.complex64, torch.complex128])
@pytest.mark.parametrize("C", [33, 64])
def test_wide_spectral_conv(cdtype, C):
    from dfno_amd.ops.spectral import spectral_conv
    dispatch.reset_fallbacks()
    torch.manual_seed(6)
    B = 2
    bounds = [[(0, 2), (0, 2), (0, 3)], [(2, 4), (0, 2), (0, 3)]]
    x = torch.randn(B, C, 4, 4, 3, dtype=cdtype)
    ws = [torch.randn(C, C, 2, 2, 3, dtype=cdtype) / math.sqrt(C) for _ in bounds]
    gy = torch.randn(B, C, 4, 4, 3, dtype=cdtype)

    # einsum composition on the CPU
    xc = x.clone().requires_grad_()
    wc = [w.clone().requires_grad_() for w in ws]
    yc = torch.zeros(B, C, 4, 4, 3, dtype=cdtype)
    for w, bd in zip(wc, bounds):
        sl = (slice(None), slice(None)) + tuple(slice(a, b) for a, b in bd)
        yc[sl] = torch.einsum("bi...,io...->bo...", xc[sl], w)
    yc.backward(gy)

    xg = x.cuda().requires_grad_()
    wg = [w.cuda().requires_grad_() for w in ws]
    yg = spectral_conv(xg, wg, bounds, C)
    yg.backward(gy.cuda())

    t = F32 if cdtype == torch.complex64 else dict(rtol=1e-11, atol=1e-11)
    assert torch.allclose(yg.detach().cpu(), yc.detach(), **t)
    assert torch.allclose(xg.grad.cpu(), xc.grad, **t)
    for a, b in zip(wg, wc):
        assert torch.allclose(a.grad.cpu(), b.grad, **t), \
            f"max {(a.grad.cpu() - b.grad).abs().max()}"
    assert not dispatch.fallback_counts()


# ---------------------------------------------------------------------------
# host dispatch: the autograd ops at a wide shape, with and without grad
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_wide_ops_autograd(dtype):
    """linear_nd (bias, GELU) then linear_res_gelu at 40 channels: forward,
    the no-grad forward (z not stored) and every gradient, no fallback."""
    from dfno_amd.ops.pointwise import linear_nd, linear_res_gelu
    dispatch.reset_fallbacks()
    torch.manual_seed(7)
    B, C, S = 2, 40, 256
    bf = dtype == torch.bfloat16
    mk = (lambda *s: ((torch.rand(*s) - 0.5).to(dtype))) if bf else \
        (lambda *s: torch.randn(*s))
    x, r = mk(B, C, S), mk(B, C, S)
    W1, W2 = mk(C, C) / (C if bf else math.sqrt(C)), mk(C, C) / (C if bf else math.sqrt(C))
    b1 = mk(C)
    gy = mk(B, C, S)

    def run(dev, up):
        ts = [t.to(dev).to(up).requires_grad_() for t in (x, W1, b1, W2, r)]
        h = linear_nd(ts[0], ts[1], ts[2], 1, "gelu")
        y = linear_res_gelu(h, ts[3], ts[4])
        y.backward(gy.to(dev).to(up))
        with torch.no_grad():
            y0 = linear_res_gelu(linear_nd(ts[0], ts[1], ts[2], 1, "gelu"),
                                 ts[3], ts[4])
        return [y.detach(), y0] + [t.grad for t in ts]

    got = run("cuda", dtype)
    ref = run("cpu", torch.float32)
    names = ["y", "y_nograd", "gx", "gW1", "gb1", "gW2", "gres"]
    for n, a, b in zip(names, got, ref):
        a = a.float().cpu()
        if bf:
            scale = b.abs().max().clamp_min(1e-6)
            # the composed-bf16 metric and bound of test_bf16_model_stash_grads
            assert (a - b).abs().max() / scale < 0.12, f"{n}: {(a - b).abs().max() / scale}"
        else:
            t = _gw_tol32(b) if n.startswith("gW") or n == "gb1" else F32
            assert torch.allclose(a, b, **t), f"{n}: max {(a - b).abs().max()}"
    assert not dispatch.fallback_counts()
