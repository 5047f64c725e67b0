"""Residual grad-x folded into the rfft adjoint (fp32 backward).

``rfft_adj_mix(gz, W, G, n) = W^T gz + rfft_trunc_adj(G, n)`` (the adjoint
mode of csrc/epilogue.hip), ``channel_mix_bwd_fused(..., want_gx=False)``
(csrc/mix_bwd.hip), the autograd wiring through the rfft stash
(ops/epilogue.py, ops/fft.py) and the model-level A/B of the
DFNO_FUSED_RFFT_ADJ knob.

Tolerances are the fp32 ones of tests/test_kernels_gpu.py:
test_dft_rfft_trunc's (rtol 2e-4, atol 2e-3) for everything downstream of
the synthesis and test_channel_mix_bwd_fused's S-scaled one for gW.

The spectrum gradient ``G`` is a full random complex tensor: the imaginary
parts of bin 0 and of a kept Nyquist bin are non-zero.  The rfft adjoint does
not drop them, it multiplies them by the table's sin(0) and sin(pi t); a
kernel that scaled or doubled bins the way ``pad_irfft`` does (the forward
mode's staging) is off by O(1) against both references here."""

import math

import pytest
import torch
import torch.nn.functional as F

from test_fused_epilogue_gpu import SHAPES

pytestmark = pytest.mark.gpu

ADJ_TOL = dict(rtol=2e-4, atol=2e-3)        # test_dft_rfft_trunc, fp32


@pytest.fixture(scope="module")
def ext():
    from dfno_amd import _ext
    return _ext.get(required=True)


def _gw_tol(S, dtype=torch.float32):
    # test_channel_mix_bwd_fused: accumulated over S, atomics reorder
    scale = max(1, S // 4096) * (1 if dtype == torch.float32 else 40)
    return dict(rtol=1e-4 * scale, atol=1e-3 * scale)


@pytest.mark.parametrize("xshape,O,n,m", SHAPES)
def test_rfft_adj_mix_vs_oracle(ext, xshape, O, n, m):
    from dfno_amd.ops.fft import _t_rfft_trunc

    torch.manual_seed(31)
    B, I = xshape[0], xshape[1]
    S = math.prod(xshape[2:])
    L = S // n
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
    # the native pair this kernel replaces
    pair = ext.dft_rfft_trunc_adj_acc(G4, 3, n,
                                      ext.channel_mix_fwd_t(gz, W)
                                      .reshape(B, I, L, n)).reshape(B, I, S)
    print(f"vs torch {(gx - ref).abs().max():.3e} "
          f"vs native pair {(gx - pair).abs().max():.3e}")
    assert torch.allclose(gx, ref, **ADJ_TOL), f"{(gx - ref).abs().max()}"
    assert torch.allclose(gx, pair, **ADJ_TOL), f"{(gx - pair).abs().max()}"
    # no atomics: bitwise reproducible
    assert torch.equal(gx, ext.rfft_adj_mix(gz, W, G4, n))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("S", [1350, 200])
def test_mix_bwd_fused_without_gx(ext, dtype, B, S):
    torch.manual_seed(32)
    C = 20
    x = torch.randn(B, C, S, device="cuda").to(dtype)
    W = torch.randn(C, C, device="cuda") / C
    z = torch.randn(B, C, S, device="cuda").to(dtype)
    gy = torch.randn(B, C, S, device="cuda").to(dtype)
    gx1, gW1, _, gz1 = ext.channel_mix_bwd_fused(gy, z, x, W, False, True)
    gx0, gW0, gb0, gz0 = ext.channel_mix_bwd_fused(gy, z, x, W, False, True,
                                                   False)
    assert gx1.shape == (B, C, S)
    assert gx0.numel() == 0 and gb0.numel() == 0
    assert gz0.dtype == dtype and torch.equal(gz0, gz1)
    # reference as in test_channel_mix_bwd_fused: gz in fp32 (the kernel's
    # gW sums its fp32 tile, not the bf16-rounded gz it streams out)
    zr = z.detach().float().requires_grad_(True)
    gz_ref = gy.float() * torch.autograd.grad(F.gelu(zr).sum(), zr)[0]
    gW_ref = torch.einsum("bos,bis->oi", gz_ref, x.float())
    print(f"gW {(gW0 - gW_ref).abs().max():.3e} "
          f"on/off {(gW0 - gW1).abs().max():.3e}")
    assert torch.allclose(gW0, gW_ref, **_gw_tol(S, dtype)), \
        f"gW {(gW0 - gW_ref).abs().max()}"
    assert torch.allclose(gW0, gW1, **_gw_tol(S, dtype))
    with pytest.raises(RuntimeError, match="want_gx"):
        ext.channel_mix_bwd_fused(gy, z, x, W, False, False, False)


def _stash_graph(knob, monkeypatch, x0, W0, A0, gy, n, m):
    """The block's arrangement by hand: rfft_trunc_stash on x, a linear
    complex op on the spectrum, the fused epilogue fed by the stash."""
    from dfno_amd.ops import irfft_linear_res_gelu
    from dfno_amd.ops.fft import (_GRAD_STASH, new_stash_key,
                                  rfft_trunc_stash)

    monkeypatch.setenv("DFNO_FUSED_RFFT_ADJ", knob)
    out = None
    mem = []
    for _ in range(2):              # twice: nothing may leak between rounds
        x = x0.clone().requires_grad_(True)
        W = W0.clone().requires_grad_(True)
        A = A0.clone().requires_grad_(True)
        key = new_stash_key()
        Xs, tok = rfft_trunc_stash(x, -1, m, key)
        y = irfft_linear_res_gelu(x, W, Xs * A, n // 2 + 1, n, m,
                                  stash=(key, tok))
        y.backward(gy)
        torch.cuda.synchronize()
        assert not _GRAD_STASH, "stash entry left behind"
        out = (y.detach(), x.grad, W.grad, A.grad)
        del x, W, A, Xs, tok, y
        mem.append(torch.cuda.memory_allocated())
    assert mem[1] == mem[0], f"allocated {mem[0]} -> {mem[1]}"
    return out


@pytest.mark.parametrize("xshape,O,n,m", SHAPES[:2])
def test_autograd_stash_on_off_torch(ext, monkeypatch, xshape, O, n, m):
    from dfno_amd.ops.fft import _t_pad_irfft, _t_rfft_trunc

    torch.manual_seed(33)
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
    on = _stash_graph("1", monkeypatch, x0, W0, A0, gy, n, m)
    assert len(calls) == 2, "fused adjoint not taken with the knob on"
    off = _stash_graph("0", monkeypatch, x0, W0, A0, gy, n, m)
    assert len(calls) == 2, "fused adjoint taken with the knob off"

    x = x0.clone().requires_grad_(True)
    W = W0.clone().requires_grad_(True)
    A = A0.clone().requires_grad_(True)
    Yt = _t_rfft_trunc(x, -1, m) * A
    z = (torch.einsum("oi,bis->bos", W, x.reshape(B, I, S))
         + _t_pad_irfft(Yt, -1, n // 2 + 1, n, m).reshape(B, O, S))
    y = F.gelu(z).reshape(gy.shape)
    y.backward(gy)
    ref = (y.detach(), x.grad, W.grad, A.grad)

    assert torch.equal(on[0], off[0]), "the knob must not touch the forward"
    for name, other in (("off", off), ("torch", ref)):
        d = [(a - b).abs().max().item() for a, b in zip(on, other)]
        print(f"vs {name}: y {d[0]:.3e} gx {d[1]:.3e} gW {d[2]:.3e} "
              f"gA {d[3]:.3e}")
        assert torch.allclose(on[0], other[0], **ADJ_TOL), f"y {d[0]}"
        assert torch.allclose(on[1], other[1], **ADJ_TOL), f"gx {d[1]}"
        assert torch.allclose(on[2], other[2], **_gw_tol(S)), f"gW {d[2]}"
        assert torch.allclose(torch.view_as_real(on[3]),
                              torch.view_as_real(other[3]), **ADJ_TOL), \
            f"gA {d[3]}"


def _run_model(knob, monkeypatch):
    import dfno_amd as dfno
    from dfno_amd import dispatch
    from dfno_amd.ops.fft import _GRAD_STASH

    monkeypatch.setenv("DFNO_FUSED_RFFT_ADJ", knob)
    dispatch.reset_fallbacks()
    device = torch.device("cuda:0")
    torch.manual_seed(3)
    _, P_x, _ = dfno.create_standard_partitions((1, 1, 1, 1, 1, 1))
    model = dfno.DistributedFNONd(P_x, [1, 2, 8, 8, 8, 1], 10, 20,
                                  (2, 2, 2, 3), num_blocks=2, device=device,
                                  dtype=torch.float32)
    torch.manual_seed(4)
    x = torch.rand(1, 2, 8, 8, 8, 1, device=device)
    y = model(x)
    tgt = torch.rand_like(y)
    dfno.DistributedRelativeLpLoss(P_x)(y, tgt).backward()
    torch.cuda.synchronize()
    dispatch.assert_all_native()
    assert not _GRAD_STASH, "stash entry left behind"
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()
             if p.grad is not None}
    return y.detach().clone(), grads


def test_model_rfft_adj_knob_on_off(ext, monkeypatch):
    calls = []
    orig = ext.rfft_adj_mix
    monkeypatch.setattr(ext, "rfft_adj_mix",
                        lambda *a: (calls.append(1), orig(*a))[1])
    y_on, g_on = _run_model("1", monkeypatch)
    # once per block per backward; never with the knob off
    assert len(calls) == 2
    y_off, g_off = _run_model("0", monkeypatch)
    assert len(calls) == 2

    assert torch.equal(y_on, y_off), "the knob must not touch the forward"
    assert g_on.keys() == g_off.keys() and g_on
    for n in g_on:
        a, b = g_on[n], g_off[n]
        if a.is_complex():
            a, b = torch.view_as_real(a), torch.view_as_real(b)
        print(f"{n} {(a - b).abs().max():.3e}")
        assert torch.allclose(a, b, **ADJ_TOL), f"{n} {(a - b).abs().max()}"
