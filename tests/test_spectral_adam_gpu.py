"""Fused spectral grad-W + Adam (``spectral_gradw_adam_``) against the
two-kernel chain it replaces, and the deferred-gradient training step against
the eager one."""

import pytest
import torch

pytestmark = pytest.mark.gpu

ADAM_TOL = dict(rtol=1e-5, atol=1e-6)   # as test_fused_adam_matches_torch
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-4)


@pytest.fixture(scope="module")
def ext():
    from dfno_amd import _ext
    e = _ext.get(required=True)
    assert e is not None
    return e


def _c64(*shape, offset8=False):
    """Random complex64 tensor; ``offset8`` puts its first element 8 bytes
    past a 16-byte boundary."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.randn(n + 1, device="cuda", dtype=torch.complex64)
    t = buf[1:] if offset8 else buf[:n]
    assert t.data_ptr() % 16 == (8 if offset8 else 0)
    return t.view(*shape)


def _flat(t):
    return torch.view_as_real(t).view(-1)


@pytest.mark.parametrize("B,I,O", [(1, 20, 20), (2, 8, 8), (1, 5, 7)])
@pytest.mark.parametrize("inner,offset8", [(4, False), (3, False), (4, True)],
                         ids=["vec", "odd-inner", "offset8"])
def test_fused_op_matches_chain(ext, B, I, O, inner, offset8):
    torch.manual_seed(31)
    F = (6, 5, inner)
    box = (3, 2, inner)
    starts = [[0, 0, 0], [3, 3, 0]]
    ps = [_c64(I, O, *box, offset8=offset8) for _ in starts]
    ms = [torch.zeros_like(p) for p in ps]
    vs = [torch.zeros_like(p) for p in ps]
    ps_r = [p.clone() for p in ps]
    ms_r = [m.clone() for m in ms]
    vs_r = [v.clone() for v in vs]
    h = HYPER
    for step in (1, 2, 3):
        x = _c64(B, I, *F)
        gy = _c64(B, O, *F)
        ext.spectral_gradw_adam_(x, gy, ps, ms, vs, starts, h["lr"], h["b1"],
                                 h["b2"], h["eps"], h["wd"], [step] * 2)
        gws = [torch.empty_like(p) for p in ps_r]
        ext.spectral_corners_bwd_w(x, gy, gws, starts)
        ext.adam_step_batch_([_flat(p) for p in ps_r], [_flat(g) for g in gws],
                             [_flat(m) for m in ms_r], [_flat(v) for v in vs_r],
                             h["lr"], h["b1"], h["b2"], h["eps"], h["wd"],
                             [step] * 2)
    torch.cuda.synchronize()
    for name, got, ref in (("p", ps, ps_r), ("m", ms, ms_r), ("v", vs, vs_r)):
        for c, (a, b) in enumerate(zip(got, ref)):
            d = (torch.view_as_real(a) - torch.view_as_real(b)).abs().max()
            print(f"{name}[{c}] max abs diff {float(d):.3e}")
            assert torch.allclose(torch.view_as_real(a), torch.view_as_real(b),
                                  **ADAM_TOL), f"{name}[{c}]: {float(d)}"


def test_fused_op_rejects_box_outside_spectrum(ext):
    x = _c64(1, 4, 6, 5, 4)
    gy = _c64(1, 4, 6, 5, 4)
    p = _c64(4, 4, 3, 2, 4)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    with pytest.raises(RuntimeError, match="outside the spectrum"):
        ext.spectral_gradw_adam_(x, gy, [p], [m], [v], [[4, 0, 0]], 1e-3, 0.9,
                                 0.999, 1e-8, 0.0, [1])


@pytest.mark.parametrize("B,I,O", [(1, 20, 20), (2, 8, 8), (1, 5, 7)])
@pytest.mark.parametrize("inner", [4, 3], ids=["pair", "odd-inner"])
def test_pair_contraction(ext, monkeypatch, B, I, O, inner):
    """Forward and grad-x of the element-pair contraction against the einsum,
    and bit for bit against the 8-byte kernel (DFNO_SPECTRAL_PAIR=0; an odd
    innermost extent takes that kernel either way)."""
    torch.manual_seed(41)
    F = (6, 5, inner)
    box = (3, 2, inner)
    starts = [[0, 0, 0], [3, 3, 0]]
    ws = [_c64(I, O, *box) for _ in starts]
    x = _c64(B, I, *F)
    gy = _c64(B, O, *F)

    def run():
        y = torch.zeros(B, O, *F, device="cuda", dtype=torch.complex64)
        gx = torch.zeros(B, I, *F, device="cuda", dtype=torch.complex64)
        ext.spectral_corners_fwd(x, ws, y, starts)
        ext.spectral_corners_bwd_x(gy, ws, gx, starts)
        return y, gx

    monkeypatch.delenv("DFNO_SPECTRAL_PAIR", raising=False)
    y, gx = run()
    monkeypatch.setenv("DFNO_SPECTRAL_PAIR", "0")
    y8, gx8 = run()
    assert torch.equal(y, y8) and torch.equal(gx, gx8)

    yr, gxr = torch.zeros_like(y), torch.zeros_like(gx)
    for w, st in zip(ws, starts):
        sl = (slice(None), slice(None)) + tuple(
            slice(a, a + n) for a, n in zip(st, box))
        yr[sl] = torch.einsum("bi...,io...->bo...", x[sl], w)
        gxr[sl] = torch.einsum("bo...,io...->bi...", gy[sl], w.conj())
    assert torch.allclose(y, yr, rtol=1e-4, atol=1e-4)
    assert torch.allclose(gx, gxr, rtol=1e-4, atol=1e-4)


def _train(monkeypatch, on):
    import dfno_amd as dfno
    from dfno_amd.optim import Adam

    monkeypatch.setenv("DFNO_FUSED_SPECTRAL_ADAM", "1" if on else "0")
    torch.manual_seed(17)
    _, P_x, _ = dfno.create_standard_partitions((1, 1, 1, 1, 1, 1))
    model = dfno.DistributedFNONd(P_x, [1, 2, 8, 8, 8, 1], 6, 8, (2, 2, 2, 2),
                                  num_blocks=2, device=torch.device("cuda"))
    crit = dfno.DistributedRelativeLpLoss(P_x)
    opt = Adam(model.parameters(), lr=1e-3)
    x = torch.rand(1, 2, 8, 8, 8, 1, device="cuda")
    y = torch.rand(1, 1, 8, 8, 8, 6, device="cuda")
    corner_grads = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        crit(model(x), y).backward()
        corner_grads += [w.grad for blk in model.blocks for w in blk.weights]
        opt.step()
    torch.cuda.synchronize()
    return model, corner_grads


def test_model_knob_on_matches_off(monkeypatch):
    from dfno_amd import dispatch

    dispatch.reset_fallbacks()
    ref, grads_off = _train(monkeypatch, on=False)
    model, grads_on = _train(monkeypatch, on=True)
    assert all(g is not None for g in grads_off)
    assert all(g is None for g in grads_on)
    for (n, p), q in zip(model.named_parameters(), ref.parameters()):
        a, b = p.detach(), q.detach()
        if a.is_complex():
            a, b = torch.view_as_real(a), torch.view_as_real(b)
        assert torch.allclose(a, b, **ADAM_TOL), \
            f"{n}: {float((a - b).abs().max())}"
    dispatch.assert_all_native()
