"""GPU kernel unit tests: every HIP kernel vs a plain PyTorch fp32/fp64
reference of the same op (numerics contract per the build rules)."""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from dfno_amd import _ext
    e = _ext.get(required=True)
    assert e is not None
    return e


def tol(dtype):
    return dict(rtol=2e-5, atol=2e-5) if dtype in (torch.float32, torch.complex64) \
        else dict(rtol=1e-11, atol=1e-11)


# ---------------------------------------------------------------------------
# channel mix
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,I,O,S,bias,act", [
    (1, 20, 20, 4096, True, True),     # width-20 block linear shapes
    (2, 2, 20, 1003, True, True),      # channel lift, odd S tail
    (1, 20, 128, 2048, True, True),    # projection to 128
    (1, 128, 1, 2048, True, False),    # projection head (O-resident path)
    (2, 40, 64, 515, False, True),     # LDS fallback path
    (1, 33, 7, 130, True, False),      # O-resident, odd sizes
])
def test_channel_mix_fwd(ext, dtype, B, I, O, S, bias, act):
    torch.manual_seed(0)
    x = torch.randn(B, I, S, device="cuda", dtype=dtype)
    W = torch.randn(O, I, device="cuda", dtype=dtype) / math.sqrt(I)
    b = torch.randn(O, device="cuda", dtype=dtype) if bias else \
        torch.empty(0, device="cuda", dtype=dtype)
    y, z = ext.channel_mix_fwd(x, W, b, act)
    z_ref = torch.einsum("oi,bis->bos", W, x)
    if bias:
        z_ref = z_ref + b.view(1, -1, 1)
    y_ref = F.gelu(z_ref) if act else z_ref
    assert torch.allclose(y, y_ref, **tol(dtype)), f"max {(y - y_ref).abs().max()}"
    if act:
        assert torch.allclose(z, z_ref, **tol(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,S,bias,gzout", [
    (1, 4096, True, False),    # trunk mix (has bias, gz discarded)
    (1, 4099, False, True),    # linear_res_gelu shape: gz is the res grad
    (2, 70001, True, True),    # grid wrap + tail + batch
])
def test_channel_mix_bwd_fused(ext, dtype, B, S, bias, gzout):
    """One-kernel trunk 20x20 mix backward (mix_bwd.hip) vs the torch
    composition: gz = gy*gelu'(z), gx = W^T gz, gW = gz x^T, gb = sum gz."""
    torch.manual_seed(5)
    C = 20
    x = torch.randn(B, C, S, device="cuda").to(dtype)
    W = torch.randn(C, C, device="cuda") / C
    z = torch.randn(B, C, S, device="cuda").to(dtype)
    gy = torch.randn(B, C, S, device="cuda").to(dtype)
    gx, gW, gb, gz = ext.channel_mix_bwd_fused(gy, z, x, W, bias, gzout)
    assert gx.dtype == dtype and gW.dtype == torch.float32
    zr = z.detach().float().requires_grad_(True)
    gz_ref = gy.float() * torch.autograd.grad(F.gelu(zr).sum(), zr)[0]
    gx_ref = torch.einsum("oi,bos->bis", W, gz_ref)
    gW_ref = torch.einsum("bos,bis->oi", gz_ref, x.float())
    tt = (dict(rtol=2e-4, atol=2e-4) if dtype == torch.float32
          else dict(rtol=2e-2, atol=2e-2))
    assert torch.allclose(gx.float(), gx_ref, **tt), \
        f"gx {(gx.float()-gx_ref).abs().max()}"
    # accumulated over S: scale tolerance with the reduction length
    scale = max(1, S // 4096) * (1 if dtype == torch.float32 else 40)
    wt = dict(rtol=1e-4 * scale, atol=1e-3 * scale)
    assert torch.allclose(gW, gW_ref, **wt), f"gW {(gW-gW_ref).abs().max()}"
    if bias:
        gb_ref = gz_ref.sum(dim=(0, 2))
        assert torch.allclose(gb, gb_ref, **wt), f"gb {(gb-gb_ref).abs().max()}"
    if gzout:
        assert torch.allclose(gz.float(), gz_ref, **tt), \
            f"gz {(gz.float()-gz_ref).abs().max()}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,I,O,S", [(1, 20, 20, 4096), (1, 20, 128, 999), (2, 128, 1, 777)])
def test_channel_mix_fwd_t(ext, dtype, B, I, O, S):
    torch.manual_seed(1)
    gz = torch.randn(B, O, S, device="cuda", dtype=dtype)
    W = torch.randn(O, I, device="cuda", dtype=dtype)
    gx = ext.channel_mix_fwd_t(gz, W)
    gx_ref = torch.einsum("oi,bos->bis", W, gz)
    assert torch.allclose(gx, gx_ref, **tol(dtype)), f"max {(gx - gx_ref).abs().max()}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,I,O,S,bias", [
    (1, 20, 20, 4096, True),      # width-20 (glds3 OW=5 path)
    (1, 20, 128, 7936, False),    # proj lift gW3: the f32-MFMA tile path
    (2, 20, 128, 4096, False),    # batched MFMA path
    (1, 16, 64, 4096, False),     # MFMA path, ragged o-slab
    (1, 20, 128, 1000, False),    # S % 128 != 0 -> glds3 fallback
])
def test_channel_mix_bwd_w(ext, dtype, B, I, O, S, bias):
    torch.manual_seed(3)
    gz = torch.randn(B, O, S, device="cuda", dtype=dtype)
    x = torch.randn(B, I, S, device="cuda", dtype=dtype)
    gW, gb = ext.channel_mix_bwd_w(gz, x, bias)
    refW = torch.einsum("bos,bis->oi", gz, x)
    t = dict(rtol=1e-4, atol=float(refW.abs().max()) * 1e-5) \
        if dtype == torch.float32 else dict(rtol=1e-11, atol=1e-9)
    assert torch.allclose(gW, refW, **t), f"max {(gW - refW).abs().max()}"
    if bias:
        refb = gz.sum(dim=(0, 2))
        assert torch.allclose(gb, refb, **t)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,I,O,S,bias", [
    # one shape per row of the grad-W launch table (the fp32 row is named;
    # fp64 lands on the generic / i-slab non-vector rows)
    (2, 16, 65, 256, False),     # gw_mfma_f32<2>, second o-slab of one row
    (1, 40, 16, 132, True),      # i-slab, vector, OW 2, second slab of 8 rows
    (1, 33, 5, 132, True),       # i-slab, vector, OW 1
    (1, 33, 5, 130, False),      # i-slab, non-vector, OW 1
    (2, 9, 8, 4100, False),      # glds3 <20,5,256>, 4 s-chunks, 4-element tail
    (1, 2, 20, 4100, True),      # glds3 <8,4,256>, 2 o-tiles, chunks 4 -> 8
    (1, 8, 128, 4100, False),    # glds3 <8,4,256>, 8 o-tiles, XCD swizzle
    (1, 24, 24, 4100, True),     # glds3 <24,2,256>
    (1, 32, 64, 4100, True),     # glds3 <32,2,128>, bias keeps it off MFMA
    (1, 25, 12, 1284, False),    # glds3 <32,2,256>, chunks 1 -> 8, two empty
    (2, 7, 9, 1003, True),       # generic cap 8 / OW 4, non-vector
    (1, 20, 20, 1003, False),    # generic cap 24 / OW 2, non-vector
    (1, 30, 10, 1003, True),     # generic cap 32 / OW 2, non-vector
    (1, 20, 5, 1003, True),      # generic cap 32 / OW 1, non-vector
    (1, 20, 5, 1000, False),     # generic cap 32 / OW 1, vector
])
def test_channel_mix_bwd_w_exact(ext, dtype, B, I, O, S, bias):
    """Integer-valued inputs in [-2, 2]: every partial sum is an integer of
    magnitude at most B * S * 4 <= 32800 < 2^24, so fp32 adds and fp32 MFMA
    are exact in any order and the result must EQUAL the fp64 einsum.  A
    dropped row, tile, chunk or tail element cannot hide in a tolerance."""
    g = torch.Generator().manual_seed(11)
    gz = torch.randint(-2, 3, (B, O, S), generator=g).to("cuda", dtype)
    g.manual_seed(12)   # another stream for x: a transpose cannot pass
    x = torch.randint(-2, 3, (B, I, S), generator=g).to("cuda", dtype)
    gW, gb = ext.channel_mix_bwd_w(gz, x, bias)
    refW = torch.einsum("bos,bis->oi", gz.double(), x.double())
    assert gW.dtype == dtype and gW.shape == (O, I)
    assert torch.equal(gW.double(), refW), \
        f"{int((gW.double() != refW).sum())} of {O * I} entries differ"
    if bias:
        assert torch.equal(gb.double(), gz.double().sum(dim=(0, 2)))
    else:
        assert gb.numel() == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("B,I,O,S", [
    (2, 20, 20, 1003),  # the pinned block shape, odd S (element-wise tail)
    (1, 7, 9, 64),       # generic cap-8 kernel, float4 path in fp32
])
def test_linear_res_gelu_fwd(ext, dtype, B, I, O, S):
    """y = gelu(z), z = W x + res: the x-resident mix with its residual."""
    torch.manual_seed(4)
    x = torch.randn(B, I, S, device="cuda", dtype=dtype)
    W = torch.randn(O, I, device="cuda", dtype=dtype) / math.sqrt(I)
    res = torch.randn(B, O, S, device="cuda", dtype=dtype)
    y, z = ext.linear_res_gelu_fwd(x, W, res)
    z_ref = torch.einsum("oi,bis->bos", W, x) + res
    assert torch.allclose(z, z_ref, **tol(dtype)), f"max {(z - z_ref).abs().max()}"
    assert torch.allclose(y, F.gelu(z_ref), **tol(dtype)), \
        f"max {(y - F.gelu(z_ref)).abs().max()}"


# ---------------------------------------------------------------------------
# gelu / add+gelu
# ---------------------------------------------------------------------------

def _elementwise_tol(dtype):
    # fp32: the rational-erf GELU is good to 1e-5 relative; fp64 calls erf
    return dict(rtol=1e-5, atol=1e-6) if dtype == torch.float32 else tol(dtype)


@pytest.mark.parametrize("n", [1, 17, 4096, 100003])
def test_gelu_fwd_bwd(ext, n, dtype=torch.float32):
    t = _elementwise_tol(dtype)
    torch.manual_seed(2)
    x = torch.randn(n, device="cuda", dtype=dtype) * 3
    y = ext.gelu_fwd(x)
    assert torch.allclose(y, F.gelu(x), **t)

    gy = torch.randn(n, device="cuda", dtype=dtype)
    gz = ext.gelu_bwd(gy, x)
    xr = x.clone().requires_grad_(True)
    F.gelu(xr).backward(gy)
    assert torch.allclose(gz, xr.grad, **t)


def test_gelu_fwd_bwd_fp64(ext):
    test_gelu_fwd_bwd(ext, 17, torch.float64)


def test_add_gelu(ext, shape=(2, 5, 333), dtype=torch.float32):
    t = _elementwise_tol(dtype)
    torch.manual_seed(3)
    a = torch.randn(*shape, device="cuda", dtype=dtype)
    b = torch.randn(*shape, device="cuda", dtype=dtype)
    y, z = ext.add_gelu_fwd(a, b)
    assert torch.allclose(z, a + b)
    assert torch.allclose(y, F.gelu(a + b), **t)


def test_add_gelu_fp64(ext):
    test_add_gelu(ext, (17,), torch.float64)


# ---------------------------------------------------------------------------
# spectral corner contraction
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
@pytest.mark.parametrize("B,I,O,F_,boxes", [
    # full 2D+t truncated spectrum with 2 corners
    (1, 20, 20, (24, 24, 8), [((0, 0, 0), (12, 12, 8)), ((0, 12, 0), (12, 12, 8))]),
    (2, 8, 8, (10, 9, 5), [((0, 0, 0), (3, 4, 5)), ((7, 5, 0), (3, 4, 5))]),
    (1, 6, 6, (7, 6, 6, 4), [((0, 0, 0, 0), (3, 3, 3, 2))]),   # 3D+t
    (1, 20, 20, (16, 8), [((1, 1), (5, 3))]),                  # offset box
])
def test_spectral_corner_fwd(ext, dtype, B, I, O, F_, boxes):
    torch.manual_seed(4)
    x = torch.randn(B, I, *F_, device="cuda", dtype=dtype)
    y = torch.zeros(B, O, *F_, device="cuda", dtype=dtype)
    y_ref = torch.zeros_like(y)
    for starts, ext_shape in boxes:
        w = torch.randn(I, O, *ext_shape, device="cuda", dtype=dtype) / (I * O)
        ext.spectral_corner_fwd(x, w, y, list(starts))
        sl = (slice(None), slice(None)) + tuple(
            slice(s, s + e) for s, e in zip(starts, ext_shape))
        y_ref[sl] = torch.einsum("bi...,io...->bo...", x[sl], w)
    torch.cuda.synchronize()
    assert torch.allclose(y, y_ref, **tol(dtype)), f"max {(y - y_ref).abs().max()}"


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_spectral_corner_bwd_x(ext, dtype):
    torch.manual_seed(5)
    B, I, O = 1, 20, 20
    F_ = (24, 24, 8)
    boxes = [((0, 0, 0), (12, 12, 8)), ((12, 12, 0), (12, 12, 8))]
    gy = torch.randn(B, O, *F_, device="cuda", dtype=dtype)
    gx = torch.zeros(B, I, *F_, device="cuda", dtype=dtype)
    gx_ref = torch.zeros_like(gx)
    for starts, ext_shape in boxes:
        w = torch.randn(I, O, *ext_shape, device="cuda", dtype=dtype) / (I * O)
        ext.spectral_corner_bwd_x(gy, w, gx, list(starts))
        sl = (slice(None), slice(None)) + tuple(
            slice(s, s + e) for s, e in zip(starts, ext_shape))
        gx_ref[sl] = torch.einsum("bo...,io...->bi...", gy[sl], w.conj())
    torch.cuda.synchronize()
    assert torch.allclose(gx, gx_ref, **tol(dtype)), f"max {(gx - gx_ref).abs().max()}"


# ---------------------------------------------------------------------------
# op-level autograd (through the Python dispatch)
# ---------------------------------------------------------------------------

def test_op_linear_nd_autograd_gpu():
    from dfno_amd.ops import linear_nd
    torch.manual_seed(6)
    for dtype, tt in [(torch.float32, 1e-4), (torch.float64, 1e-10)]:
        x = torch.randn(2, 6, 9, 11, device="cuda", dtype=dtype, requires_grad=True)
        W = torch.randn(4, 6, device="cuda", dtype=dtype, requires_grad=True)
        b = torch.randn(4, device="cuda", dtype=dtype, requires_grad=True)
        y = linear_nd(x, W, b, dim=1, activation="gelu")
        gy = torch.randn_like(y)
        y.backward(gy)

        xr = x.detach().clone().requires_grad_(True)
        Wr = W.detach().clone().requires_grad_(True)
        br = b.detach().clone().requires_grad_(True)
        yr = F.gelu(torch.einsum("oi,bihw->bohw", Wr, xr) + br.view(1, -1, 1, 1))
        yr.backward(gy)

        assert torch.allclose(y, yr, rtol=tt, atol=tt)
        assert torch.allclose(x.grad, xr.grad, rtol=tt, atol=tt)
        assert torch.allclose(W.grad, Wr.grad, rtol=tt, atol=tt)
        assert torch.allclose(b.grad, br.grad, rtol=tt, atol=tt)


def test_op_spectral_autograd_gpu():
    from dfno_amd.ops import spectral_conv
    torch.manual_seed(7)
    B, I, O = 1, 8, 8
    F_ = (12, 10, 6)
    bounds = [[(0, 5), (0, 4), (0, 3)], [(7, 12), (6, 10), (0, 3)]]
    for dtype, tt in [(torch.complex64, 1e-4), (torch.complex128, 1e-10)]:
        x = torch.randn(B, I, *F_, device="cuda", dtype=dtype, requires_grad=True)
        ws = [torch.randn(I, O, *[b - a for a, b in bb], device="cuda", dtype=dtype,
                          requires_grad=True) for bb in bounds]
        y = spectral_conv(x, ws, bounds, O)
        gy = torch.randn_like(y)
        y.backward(gy)

        xr = x.detach().clone().requires_grad_(True)
        wr = [w.detach().clone().requires_grad_(True) for w in ws]
        yr = torch.zeros_like(y)
        for w, bb in zip(wr, bounds):
            sl = (slice(None), slice(None)) + tuple(slice(a, b) for a, b in bb)
            yr[sl] = torch.einsum("bi...,io...->bo...", xr[sl], w)
        yr.backward(gy)

        assert torch.allclose(y, yr, rtol=tt, atol=tt)
        assert torch.allclose(x.grad, xr.grad, rtol=tt, atol=tt)
        for w, w2 in zip(ws, wr):
            assert torch.allclose(w.grad, w2.grad, rtol=tt, atol=tt)


# ---------------------------------------------------------------------------
# fused projection head
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,tt", [(torch.float32, 3e-4), (torch.float64, 1e-10)])
@pytest.mark.parametrize("B,I,M,O2,S", [
    (1, 20, 128, 1, 4096),    # flagship head shape -> fused backward (fp32)
    (2, 12, 64, 2, 1001),     # odd S (scalar path), multi-batch, O2=2
    (2, 20, 128, 2, 4099),    # fused backward: O2=2, tail tile, B=2
    (1, 20, 128, 1, 51233),   # fused backward: > 768 tiles (grid wrap) + tail
    (2, 28, 40, 3, 1003),     # <32, 8> row, element-wise, across the batch
    (1, 28, 40, 3, 1024),     # <32, 8> row, float4 IO in fp32
    (1, 12, 64, 2, 1024),     # <24, 2> row, float4 IO in fp32
    (1, 32, 128, 8, 260),     # I and O2 at their caps, one partial block;
                              # backward LDS 39,424 B fp32 / 78,848 B fp64
])
def test_proj_head(dtype, tt, B, I, M, O2, S):
    from dfno_amd.ops import proj_head
    torch.manual_seed(8)
    x = torch.randn(B, I, S, device="cuda", dtype=dtype, requires_grad=True)
    W3 = (torch.randn(M, I, device="cuda", dtype=dtype) / I).requires_grad_(True)
    b3 = torch.randn(M, device="cuda", dtype=dtype).requires_grad_(True)
    W4 = (torch.randn(O2, M, device="cuda", dtype=dtype) / M).requires_grad_(True)
    b4 = torch.randn(O2, device="cuda", dtype=dtype).requires_grad_(True)

    y = proj_head(x, W3, b3, W4, b4)
    gy = torch.randn_like(y)
    y.backward(gy)

    xr = x.detach().clone().requires_grad_(True)
    W3r = W3.detach().clone().requires_grad_(True)
    b3r = b3.detach().clone().requires_grad_(True)
    W4r = W4.detach().clone().requires_grad_(True)
    b4r = b4.detach().clone().requires_grad_(True)
    h = F.gelu(torch.einsum("mi,bis->bms", W3r, xr) + b3r.view(1, -1, 1))
    yr = torch.einsum("om,bms->bos", W4r, h) + b4r.view(1, -1, 1)
    yr.backward(gy)

    assert torch.allclose(y, yr, rtol=tt, atol=tt), f"fwd max {(y-yr).abs().max()}"
    for a, b in [(x, xr), (W3, W3r), (b3, b3r), (W4, W4r), (b4, b4r)]:
        assert torch.allclose(a.grad, b.grad, rtol=tt * 30, atol=tt * 30), \
            f"grad max {(a.grad - b.grad).abs().max()}"


def test_proj_head_entry_checks(ext):
    """The extension refuses mismatched or out-of-range calls before any
    launch."""
    def args(dtype, B, I, M, O2, S):
        dev = "cuda"
        return [torch.randn(B, I, S, device=dev).to(dtype),
                torch.randn(M, I, device=dev).to(dtype),
                torch.randn(M, device=dev).to(dtype),
                torch.randn(O2, M, device=dev).to(dtype),
                torch.randn(O2, device=dev).to(dtype)]

    x, W3, b3, W4, b4 = args(torch.float32, 1, 12, 64, 2, 256)
    gy = torch.randn(1, 2, 252, device="cuda")            # wrong S
    with pytest.raises(RuntimeError, match="gy must be"):
        ext.proj_head_bwd(gy, x, W3, b3, W4)
    W4bad = torch.randn(2, 65, device="cuda")             # W4.size(1) != M
    with pytest.raises(RuntimeError, match="proj_head shapes"):
        ext.proj_head_fwd(x, W3, b3, W4bad, b4)
    with pytest.raises(RuntimeError, match="flagship shape only"):
        ext.proj_head_fwd(*args(torch.bfloat16, 1, 12, 64, 1, 256))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# fused truncated-spectrum DFTs vs torch.fft compositions
# ---------------------------------------------------------------------------

_ROW_LINES = 2 * 256 + 37


@pytest.mark.parametrize("dtype,tt", [(torch.float32, 2e-4), (torch.float64, 1e-11)])
@pytest.mark.parametrize("shape,dim,N,m", [
    ((1, 20, 9, 9, 6, 30), 5, 30, 8),    # flagship t-dim rfft
    ((2, 4, 7, 15), 3, 15, 5),           # odd N
    # launch rows at 2 * 256 + 37 lines (two full tiles and a ragged tail);
    # the backward is the c2r adjoint of the same (N, m)
    ((_ROW_LINES, 64), 1, 64, 16),       # fp32: pinned (64, 16) r2c and c2r
    ((_ROW_LINES, 48), 1, 48, 12),       # fp32: runtime-N ring, N <= 64 class
    ((_ROW_LINES, 20), 1, 20, 5),        # fp32: runtime-N ring, N <= 32 class
])
def test_dft_rfft_trunc(dtype, tt, shape, dim, N, m):
    from dfno_amd.ops.fft import rfft_trunc, _t_rfft_trunc
    torch.manual_seed(10)
    x = torch.randn(*shape, device="cuda", dtype=dtype, requires_grad=True)
    y = rfft_trunc(x, dim, m)
    xr = x.detach().clone().requires_grad_(True)
    yr = _t_rfft_trunc(xr, dim, m)
    assert torch.allclose(y, yr, rtol=tt, atol=tt * 10), f"fwd {(y-yr).abs().max()}"
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g)
    assert torch.allclose(x.grad, xr.grad, rtol=tt, atol=tt * 10), \
        f"bwd {(x.grad-xr.grad).abs().max()}"


@pytest.mark.parametrize("N,m,misaligned", [
    (40, 24, False),                     # pinned (40, 24)
    (32, 32, False),                     # pinned (32, 32)
    (30, 8, True),                       # unaligned base: tile kernel, not the ring
])
def test_dft_rfft_trunc_rows_direct(ext, N, m, misaligned, tt=2e-4):
    # fp32 r2c rows that ops.fft.rfft_trunc cannot reach (it clamps m to
    # N // 2 + 1, and hands over aligned tensors), through the entry point:
    # the first m bins of the full spectrum of a real line
    torch.manual_seed(14)
    if misaligned:
        x = torch.randn(_ROW_LINES * N + 1, device="cuda")[1:].view(_ROW_LINES, N)
        assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    else:
        x = torch.randn(_ROW_LINES, N, device="cuda")
    y = ext.dft_rfft_trunc(x, 1, m)
    yr = torch.fft.fft(x, dim=1)[:, :m]
    assert torch.allclose(y, yr, rtol=tt, atol=tt * 10), f"fwd {(y-yr).abs().max()}"


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("N,tt", [(64, 2e-4), (40, 2e-4), (128, 6e-4)])
def test_dft_rfft_trunc_adj_rows_direct(ext, N, tt, acc, m=16):
    # fp32 c2r rows: pinned (64, 16) and (40, 16), and the 128-line tiles of
    # N = 128, each with and without the fused addend, against the autograd
    # adjoint of the torch.fft composition
    from dfno_amd.ops.fft import _t_rfft_trunc
    torch.manual_seed(15)
    gy = torch.randn(_ROW_LINES, m, device="cuda", dtype=torch.complex64)
    xr = torch.zeros(_ROW_LINES, N, device="cuda", requires_grad=True)
    _t_rfft_trunc(xr, 1, m).backward(gy)
    ref = xr.grad
    if acc:
        a = torch.randn(_ROW_LINES, N, device="cuda")
        gx = ext.dft_rfft_trunc_adj_acc(gy, 1, N, a)
        ref = ref + a
    else:
        gx = ext.dft_rfft_trunc_adj(gy, 1, N)
    assert torch.allclose(gx, ref, rtol=tt, atol=tt * 10), f"{(gx-ref).abs().max()}"


@pytest.mark.parametrize("dtype,tt", [(torch.complex64, 3e-4), (torch.complex128, 1e-11)])
@pytest.mark.parametrize("shape,dim,mlo,mhi", [
    ((1, 20, 64, 24, 8), 2, 12, 12),     # z-dim with inner>1 (radix-8x8)
    ((1, 6, 10, 5), 1, 3, 2),
    ((2, 5, 12), 2, 4, 3),               # last dim c2c
    ((2, 20, 64, 4), 2, 12, 12),         # radix-8x8 with tiny inner (pairs=2)
    ((1, 4, 64, 3), 2, 10, 10),          # N=64 odd inner -> non-paired fallback
    ((1, 3, 64, 8), 2, 16, 16),          # radix-8x8 at the LCAP=17 boundary
])
def test_dft_fft_trunc_and_pad_ifft(dtype, tt, shape, dim, mlo, mhi):
    from dfno_amd.ops.fft import fft_trunc, pad_ifft, _t_fft_trunc, _t_pad_ifft
    torch.manual_seed(11)
    n = shape[dim]
    x = torch.randn(*shape, device="cuda", dtype=dtype, requires_grad=True)
    y = fft_trunc(x, dim, mlo, mhi)
    xr = x.detach().clone().requires_grad_(True)
    yr = _t_fft_trunc(xr, dim, mlo, mhi)
    assert torch.allclose(y, yr, rtol=tt, atol=tt * 10), f"fwd {(y-yr).abs().max()}"
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g)
    assert torch.allclose(x.grad, xr.grad, rtol=tt, atol=tt * 10), \
        f"bwd {(x.grad-xr.grad).abs().max()}"

    # inverse path
    z = torch.randn_like(y).requires_grad_(True)
    w = pad_ifft(z, dim, n, mlo, mhi)
    zr = z.detach().clone().requires_grad_(True)
    wr = _t_pad_ifft(zr, dim, n, mlo, mhi)
    assert torch.allclose(w, wr, rtol=tt, atol=tt * 10), f"ifft fwd {(w-wr).abs().max()}"
    g2 = torch.randn_like(w)
    w.backward(g2)
    wr.backward(g2)
    assert torch.allclose(z.grad, zr.grad, rtol=tt, atol=tt * 10), \
        f"ifft bwd {(z.grad-zr.grad).abs().max()}"


@pytest.mark.parametrize("dtype,tt", [(torch.complex64, 2e-4), (torch.complex128, 1e-11)])
@pytest.mark.parametrize("shape,n_half,n_out,m", [
    ((1, 20, 9, 9, 6, 8), 16, 30, 8),    # flagship irfft
    ((2, 4, 3), 9, 17, 3),               # odd n_out
    ((2, 4, 8), 8, 14, 8),               # m hits the Nyquist bin (even n)
])
def test_dft_pad_irfft(dtype, tt, shape, n_half, n_out, m):
    from dfno_amd.ops.fft import pad_irfft, _t_pad_irfft
    torch.manual_seed(12)
    y = torch.randn(*shape, device="cuda", dtype=dtype, requires_grad=True)
    x = pad_irfft(y, -1, n_half, n_out, m)
    yr = y.detach().clone().requires_grad_(True)
    xr = _t_pad_irfft(yr, -1, n_half, n_out, m)
    assert torch.allclose(x, xr, rtol=tt, atol=tt * 10), f"fwd {(x-xr).abs().max()}"
    g = torch.randn_like(x)
    x.backward(g)
    xr.backward(g)
    assert torch.allclose(y.grad, yr.grad, rtol=tt, atol=tt * 10), \
        f"bwd {(y.grad-yr.grad).abs().max()}"


# ---------------------------------------------------------------------------
# big-N (64 < N <= 256) native transforms: radix-8xNB c2c and LB-tiled
# r2c/c2r (VERDICT.md round-1 item 2 — the 128^3/256^3 and nt>=64 grids)
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,tt", [(torch.float32, 6e-4), (torch.float64, 1e-10)])
@pytest.mark.parametrize("shape,dim,m", [
    ((1, 4, 6, 6, 128), 4, 16),          # nt=128 temporal scaling rfft
    ((1, 3, 4, 4, 256), 4, 32),          # nt=256
    ((2, 5, 100), 2, 12),                # 64 < N < 128, odd-ish lines
])
def test_dft_rfft_trunc_bigN(dtype, tt, shape, dim, m):
    from dfno_amd.ops.fft import rfft_trunc, _t_rfft_trunc
    torch.manual_seed(40)
    x = torch.randn(*shape, device="cuda", dtype=dtype, requires_grad=True)
    y = rfft_trunc(x, dim, m)
    xr = x.detach().clone().requires_grad_(True)
    yr = _t_rfft_trunc(xr, dim, m)
    assert torch.allclose(y, yr, rtol=tt, atol=tt * 10), f"fwd {(y-yr).abs().max()}"
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g)
    assert torch.allclose(x.grad, xr.grad, rtol=tt, atol=tt * 10), \
        f"bwd {(x.grad-xr.grad).abs().max()}"


@pytest.mark.parametrize("N", [30, 20])   # compile-time-N and runtime-N kernels
def test_dft_rfft_trunc_many_tiles_per_block(N):
    # The fp32 r2c kernel runs a grid of at most 4096 blocks over 256-line
    # tiles with a two-buffer LDS ring.  Only from the third tile of a block
    # on is a tile staged into buffer 0 while buffer 1 is consumed, and at
    # these N the last staging instruction of a tile is a pad: it must stay
    # inside its own buffer.  3 * 4096 tiles give every block three tiles.
    # Needs this size: no smaller one reaches the ring's second lap.
    from dfno_amd.ops.fft import rfft_trunc, _t_rfft_trunc
    torch.manual_seed(41)
    m = 8
    x = torch.rand(3 * 4096 * 256, N, device="cuda")
    with torch.no_grad():
        y1 = rfft_trunc(x, 1, m)
        y2 = rfft_trunc(x, 1, m)
        yr = _t_rfft_trunc(x, 1, m)
    # same input, same kernel, no atomics: bitwise reproducible
    assert torch.equal(torch.view_as_real(y1), torch.view_as_real(y2))
    # a naive fp32 DFT of N terms in [0, 1): |err| <~ N * eps * sum|x| =
    # 30 * 6e-8 * 30 = 5.4e-5; a line read from a clobbered tile is off by O(1)
    err = (y1 - yr).abs().max().item()
    assert err < 1e-4, f"fwd {err}"


@pytest.mark.parametrize("dtype,tt", [(torch.complex64, 8e-4), (torch.complex128, 1e-10)])
@pytest.mark.parametrize("shape,dim,mlo,mhi", [
    ((1, 4, 128, 16, 8), 2, 8, 8),       # radix-8x16 (128^2 weak-scaling x-dim)
    ((1, 3, 256, 8, 8), 2, 16, 16),      # radix-8x32 at the LCAP=17 boundary
    ((1, 4, 128, 5), 2, 8, 8),           # odd inner -> generic naive big-N
    ((1, 2, 96, 6), 2, 8, 8),            # N=96: paired generic (not radix)
])
def test_dft_fft_trunc_and_pad_ifft_bigN(dtype, tt, shape, dim, mlo, mhi):
    from dfno_amd.ops.fft import fft_trunc, pad_ifft, _t_fft_trunc, _t_pad_ifft
    torch.manual_seed(41)
    n = shape[dim]
    x = torch.randn(*shape, device="cuda", dtype=dtype, requires_grad=True)
    y = fft_trunc(x, dim, mlo, mhi)
    xr = x.detach().clone().requires_grad_(True)
    yr = _t_fft_trunc(xr, dim, mlo, mhi)
    assert torch.allclose(y, yr, rtol=tt, atol=tt * 10), f"fwd {(y-yr).abs().max()}"
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g)
    assert torch.allclose(x.grad, xr.grad, rtol=tt, atol=tt * 10), \
        f"bwd {(x.grad-xr.grad).abs().max()}"

    z = torch.randn_like(y).requires_grad_(True)
    w = pad_ifft(z, dim, n, mlo, mhi)
    zr = z.detach().clone().requires_grad_(True)
    wr = _t_pad_ifft(zr, dim, n, mlo, mhi)
    assert torch.allclose(w, wr, rtol=tt, atol=tt * 10), f"ifft fwd {(w-wr).abs().max()}"
    g2 = torch.randn_like(w)
    w.backward(g2)
    wr.backward(g2)
    assert torch.allclose(z.grad, zr.grad, rtol=tt, atol=tt * 10), \
        f"ifft bwd {(z.grad-zr.grad).abs().max()}"


@pytest.mark.parametrize("dtype,tt", [(torch.complex64, 6e-4), (torch.complex128, 1e-10)])
@pytest.mark.parametrize("shape,n_half,n_out,m", [
    ((1, 4, 6, 6, 16), 65, 128, 16),     # nt=128 irfft
    ((1, 3, 4, 4, 32), 129, 256, 32),    # nt=256
])
def test_dft_pad_irfft_bigN(dtype, tt, shape, n_half, n_out, m):
    from dfno_amd.ops.fft import pad_irfft, _t_pad_irfft
    torch.manual_seed(42)
    y = torch.randn(*shape, device="cuda", dtype=dtype, requires_grad=True)
    x = pad_irfft(y, -1, n_half, n_out, m)
    yr = y.detach().clone().requires_grad_(True)
    xr = _t_pad_irfft(yr, -1, n_half, n_out, m)
    assert torch.allclose(x, xr, rtol=tt, atol=tt * 10), f"fwd {(x-xr).abs().max()}"
    g = torch.randn_like(x)
    x.backward(g)
    xr.backward(g)
    assert torch.allclose(y.grad, yr.grad, rtol=tt, atol=tt * 10), \
        f"bwd {(y.grad-yr.grad).abs().max()}"


# ---------------------------------------------------------------------------
# fused (z,t) boundary 2-D transform vs the 1-D composition
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape,mzl,mzh,mt,bf16", [
    ((1, 5, 9, 64, 30), 12, 12, 8, False),   # flagship (z,t)
    ((2, 3, 7, 48, 32), 8, 8, 9, False),     # even T edge mode in range
    ((1, 4, 6, 64, 30), 12, 12, 8, True),    # bf16 IO
])
def test_zt_fused_transform(shape, mzl, mzh, mt, bf16):
    from dfno_amd.ops.fft import (zt_fwd, zt_inv, _t_rfft_trunc, _t_fft_trunc,
                                  _t_pad_ifft, _t_pad_irfft)
    torch.manual_seed(13)
    Z, T = shape[-2], shape[-1]
    dt = torch.bfloat16 if bf16 else torch.float32
    tol = 2e-2 if bf16 else 3e-4
    x = torch.randn(*shape, device="cuda").to(dt).requires_grad_(True)
    y = zt_fwd(x, mzl, mzh, mt)
    xr = x.detach().float().requires_grad_(True)
    yr = _t_fft_trunc(_t_rfft_trunc(xr, -1, mt), -2, mzl, mzh)
    assert torch.allclose(y, yr, rtol=tol, atol=tol * 10), \
        f"zt fwd {(y-yr).abs().max()}"
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g)
    assert torch.allclose(x.grad.float(), xr.grad, rtol=tol, atol=tol * 10), \
        f"zt fwd bwd {(x.grad.float()-xr.grad).abs().max()}"

    # inverse: kept modes -> (Z, T) real
    z = torch.randn(*shape[:-2], mzl + mzh, mt, dtype=torch.complex64,
                    device="cuda").requires_grad_(True)
    w = zt_inv(z, Z, T, mzl, mzh, out_dtype=dt)
    assert w.dtype == dt
    zr = z.detach().clone().requires_grad_(True)
    wr = _t_pad_irfft(_t_pad_ifft(zr, -2, Z, mzl, mzh), -1, T // 2 + 1, T, mt)
    assert torch.allclose(w.float(), wr, rtol=tol, atol=tol * 10), \
        f"zt inv {(w.float()-wr).abs().max()}"
    g2 = torch.randn_like(w)
    w.backward(g2)
    wr.backward(g2.float())
    assert torch.allclose(z.grad, zr.grad, rtol=tol, atol=tol * 10), \
        f"zt inv bwd {(z.grad-zr.grad).abs().max()}"


def test_zt_stash_accumulate():
    """The zt adjoint's fused accumulate (residual-grad stash) matches the
    unfused add."""
    from dfno_amd.ops.fft import zt_fwd, StashGradFn, new_stash_key
    torch.manual_seed(14)
    shape, mzl, mzh, mt = (1, 4, 8, 64, 30), 12, 12, 8
    x = torch.randn(*shape, device="cuda", requires_grad=True)
    key = new_stash_key()
    y, tok = zt_fwd(x, mzl, mzh, mt, stash_key=key)
    x_epi = StashGradFn.apply(x, tok, key)
    out = y.abs().square().sum() + (x_epi * 3.0).sum()
    out.backward()
    g_fused = x.grad.clone()

    xr = x.detach().clone().requires_grad_(True)
    yr = zt_fwd(xr, mzl, mzh, mt)
    outr = yr.abs().square().sum() + (xr * 3.0).sum()
    outr.backward()
    assert torch.allclose(g_fused, xr.grad, rtol=1e-5, atol=1e-5), \
        f"stash acc {(g_fused-xr.grad).abs().max()}"


# ---------------------------------------------------------------------------
# fused Adam vs torch.optim.Adam
# ---------------------------------------------------------------------------

def test_fused_adam_matches_torch():
    from dfno_amd.optim import Adam as FusedAdam
    torch.manual_seed(20)

    def make_params():
        return [torch.randn(1000, device="cuda", requires_grad=True),
                torch.randn(20, 20, 123, device="cuda", dtype=torch.complex64,
                            requires_grad=True),
                torch.randn(7, device="cuda", dtype=torch.float64, requires_grad=True),
                # bf16 params take the fused bf16 multi-tensor kernel
                # (8-wide + ragged tail)
                torch.randn(20, 20, device="cuda", dtype=torch.bfloat16,
                            requires_grad=True),
                torch.randn(37, device="cuda", dtype=torch.bfloat16,
                            requires_grad=True)]

    p1 = make_params()
    torch.manual_seed(20)
    p2 = make_params()
    for a, b in zip(p1, p2):
        assert torch.equal(a.detach(), b.detach())

    o1 = FusedAdam(p1, lr=1e-2, weight_decay=1e-4)
    o2 = torch.optim.Adam(p2, lr=1e-2, weight_decay=1e-4)
    for it in range(5):
        torch.manual_seed(100 + it)
        for a, b in zip(p1, p2):
            g = torch.randn_like(a)
            a.grad = g.clone()
            b.grad = g.clone()
        o1.step()
        o2.step()
    for a, b in zip(p1, p2):
        tt = dict(rtol=1e-5, atol=1e-6) if a.dtype != torch.bfloat16 \
            else dict(rtol=2e-2, atol=2e-2)   # bf16 state rounding differs
        assert torch.allclose(a.detach().float(), b.detach().float(), **tt), \
            f"{a.dtype}: max {(a.detach().float()-b.detach().float()).abs().max()}"


# ---------------------------------------------------------------------------
# fused lift head
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,tt", [(torch.float32, 3e-4), (torch.float64, 1e-10)])
def test_lift_head(dtype, tt, B=1, C=2, S=5000, Tn=30, W=20):
    from dfno_amd.ops import lift_head
    torch.manual_seed(21)
    x = torch.randn(B, C, S, 1, device="cuda", dtype=dtype, requires_grad=True)
    W1 = torch.randn(Tn, 1, device="cuda", dtype=dtype).requires_grad_(True)
    b1 = torch.randn(Tn, device="cuda", dtype=dtype).requires_grad_(True)
    W2 = (torch.randn(W, C, device="cuda", dtype=dtype) / C).requires_grad_(True)
    b2 = torch.randn(W, device="cuda", dtype=dtype).requires_grad_(True)

    y = lift_head(x, W1, b1, W2, b2)
    assert y.shape == (B, W, S, Tn)
    gy = torch.randn_like(y)
    y.backward(gy)

    xr = x.detach().clone().requires_grad_(True)
    W1r = W1.detach().clone().requires_grad_(True)
    b1r = b1.detach().clone().requires_grad_(True)
    W2r = W2.detach().clone().requires_grad_(True)
    b2r = b2.detach().clone().requires_grad_(True)
    h = F.gelu(torch.einsum("ti,bcsi->bcst", W1r, xr) + b1r.view(1, 1, 1, -1))
    yr = F.gelu(torch.einsum("wc,bcst->bwst", W2r, h) + b2r.view(1, -1, 1, 1))
    yr.backward(gy)

    assert torch.allclose(y, yr, rtol=tt, atol=tt), f"fwd {(y-yr).abs().max()}"
    for a, b in [(x, xr), (W1, W1r), (b1, b1r), (W2, W2r), (b2, b2r)]:
        assert torch.allclose(a.grad, b.grad, rtol=tt * 30, atol=tt * 30), \
            f"grad max {(a.grad-b.grad).abs().max()}"


@pytest.mark.parametrize("C,Tn,W,S", [
    (4, 32, 24, 5),      # every cap at once, fewer points than one wave
    (1, 9, 20, 300),     # off the caps, pinned width, more than one block
])
def test_lift_head_fp64_single_step(C, Tn, W, S):
    """fp64 with T_in == 1 runs the chunked general-lift kernels."""
    test_lift_head(torch.float64, 1e-10, 1, C, S, Tn, W)
