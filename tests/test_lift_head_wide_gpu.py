"""Fused lift head at trunk widths 25..64 (the wide kernel rows).

Op-level forward + backward of ``dfno_amd.ops.lift_head`` against the plain
torch composition, gradcheck, the width-65 refusal, and whole models of width
40 / 64 running with no fallback note at all in fp32 and fp64 (bf16 models
keep the composed lift at these widths; the op itself takes bf16).

Bounds are measured in the test, per tensor (y, gx, gW1, gb1, gW2, gb2):

* fp32: the reference is the composition in fp64; d_ref is the error of the
  same composition run by torch in fp32.  The kernel must satisfy
  d_kernel <= 10 * d_ref + 1e-6 * max|fp64|: the factor covers summation order
  (MFMA chain, atomics), while a dropped or duplicated width row is an error
  near 1/width.
* fp64: rtol = atol = 1e-10.
* bf16: the reference is the fp32 composition on the bf16-rounded inputs;
  d_ref is the error of the torch composition run in bf16.  The kernel
  computes in fp32 and rounds once on store:
  d_kernel <= 2 * d_ref + 2^-8 * max|ref|.
"""

import pytest
import torch
import torch.nn.functional as F

import dfno_amd as dfno
from dfno_amd import dispatch

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
NAMES = ["y", "gx", "gW1", "gb1", "gW2", "gb2"]


def _inputs(dtype, B, C, S, Ti, To, W, seed=53):
    torch.manual_seed(seed)
    dev = "cuda"
    x = torch.randn(B, C, S, Ti, device=dev, dtype=dtype)
    W1 = torch.randn(To, Ti, device=dev, dtype=dtype)
    b1 = torch.randn(To, device=dev, dtype=dtype)
    W2 = torch.randn(W, C, device=dev, dtype=dtype) / C
    b2 = torch.randn(W, device=dev, dtype=dtype)
    gy = torch.randn(B, W, S, To, device=dev, dtype=dtype)
    return [x, W1, b1, W2, b2], gy


def _composition(ts, gy, dtype):
    """The two einsums and GELUs in plain torch, run in ``dtype``:
    [y, gx, gW1, gb1, gW2, gb2]."""
    x, W1, b1, W2, b2 = [t.detach().to(dtype).requires_grad_(True) for t in ts]
    h = F.gelu(torch.einsum("ti,bcsi->bcst", W1, x) + b1.view(1, 1, 1, -1))
    y = F.gelu(torch.einsum("wc,bcst->bwst", W2, h) + b2.view(1, -1, 1, 1))
    y.backward(gy.to(dtype))
    return [y.detach()] + [t.grad for t in (x, W1, b1, W2, b2)]


def _kernel(ts, gy):
    from dfno_amd.ops import lift_head
    ts = [t.detach().clone().requires_grad_(True) for t in ts]
    y = lift_head(*ts)
    assert y.shape == gy.shape and y.dtype == gy.dtype
    y.backward(gy)
    torch.cuda.synchronize()
    return [y.detach()] + [t.grad for t in ts]


def _mx(t):
    return float(t.abs().max())


def _check(dtype, B, C, S, Ti, To, W):
    ts, gy = _inputs(dtype, B, C, S, Ti, To, W)
    got = _kernel(ts, gy)
    if dtype == F64:
        want = _composition(ts, gy, F64)
        for n, a, b in zip(NAMES, got, want):
            assert a.shape == b.shape, n
            print(f"{n}: d_kernel {_mx(a - b):.3e} max {_mx(b):.3e}")
        for n, a, b in zip(NAMES, got, want):
            assert torch.allclose(a, b, rtol=1e-10, atol=1e-10), \
                f"{n}: max {_mx(a - b)}"
        return
    if dtype == F32:
        ref_dtype, factor, floor = F64, 10.0, 1e-6
    else:
        ref_dtype, factor, floor = F32, 2.0, 2.0 ** -8
    want = _composition(ts, gy, ref_dtype)      # inputs as stored, widened
    torch_run = _composition(ts, gy, dtype)
    bad = []
    for n, a, t, b in zip(NAMES, got, torch_run, want):
        assert a.shape == b.shape and a.dtype == dtype, n
        d_kernel = _mx(a.to(ref_dtype) - b)
        d_ref = _mx(t.to(ref_dtype) - b)
        bound = factor * d_ref + floor * _mx(b)
        print(f"{n}: d_kernel {d_kernel:.3e} d_ref {d_ref:.3e} "
              f"bound {bound:.3e} max {_mx(b):.3e}")
        if not d_kernel <= bound:
            bad.append((n, d_kernel, bound))
    assert not bad, f"outside {factor} * d_ref + {floor} * max: {bad}"


# 1: first width past the narrow rows ([B,C,S] form): a partly filled slab
#    whose second m-tile has 9 live rows over 7 never-written tile rows; odd
#    S, so a pair of points crosses the batch boundary
@pytest.mark.parametrize("dtype", [F32, BF16, F64])
def test_wide_lift_w25_lane_k(dtype):
    _check(dtype, B=2, C=2, S=37, Ti=1, To=30, W=25)


# 2: an exact slab and one row past it (second slab with a single live row);
#    two points per wave, odd point count
@pytest.mark.parametrize("W", [32, 33])
@pytest.mark.parametrize("dtype", [F32, F64])
def test_wide_lift_slab_edge(dtype, W):
    _check(dtype, B=1, C=3, S=129, Ti=4, To=6, W=W)


# 3: every cap at its limit, less than one block of work
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_wide_lift_all_caps(dtype):
    _check(dtype, B=1, C=4, S=5, Ti=16, To=64, W=64)


# 4: 16411 points at one point per wave: more than the 8192 waves of the
#    forward grid and the 3072 of the backward grid, so every wave iterates
#    carrying its four fragments, and every block lands on the same
#    weight-grad atomics
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_wide_lift_large_s(dtype):
    _check(dtype, B=1, C=1, S=16411, Ti=10, To=40, W=40)


# 5: Ti == 1 routed to the general kernels (To > 32), 64 lanes per point
def test_wide_lift_tin1_wide_tout():
    _check(F32, B=1, C=2, S=50, Ti=1, To=48, W=48)


# 6: single-point batches, T_out one past the 32-lane layout
def test_wide_lift_to33_s1():
    _check(F32, B=3, C=2, S=1, Ti=2, To=33, W=64)


# 7: one case per launch row <LP, TIC> at a wide width
@pytest.mark.parametrize("Ti,To", [(3, 20), (12, 30), (3, 50), (12, 50)])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_wide_lift_launch_rows(dtype, Ti, To):
    _check(dtype, B=1, C=2, S=45, Ti=Ti, To=To, W=40)


def test_wide_lift_gradcheck_fp64():
    from dfno_amd.ops import lift_head
    ts, _ = _inputs(F64, B=1, C=2, S=3, Ti=3, To=5, W=33)
    ts = [t.requires_grad_(True) for t in ts]
    # weight grads go through atomics: allow last-bit reordering noise
    assert torch.autograd.gradcheck(lift_head, ts, nondet_tol=1e-12)


def test_width_65_is_refused():
    from dfno_amd import _ext
    ext = _ext.get(required=True)
    ts, gy = _inputs(F32, B=1, C=2, S=4, Ti=3, To=8, W=65)
    with pytest.raises(RuntimeError, match="unsupported dims"):
        ext.lift_head_fwd(*ts)
    with pytest.raises(RuntimeError, match="unsupported dims"):
        ext.lift_head_bwd(gy, *ts)
    ts, gy = _inputs(F32, B=1, C=2, S=4, Ti=1, To=8, W=65)
    x3 = ts[0].reshape(1, 2, 4)
    with pytest.raises(RuntimeError, match="unsupported dims"):
        ext.lift_head_fwd(x3, *ts[1:])
    with pytest.raises(RuntimeError, match="unsupported dims"):
        ext.lift_head_bwd(gy, x3, *ts[1:])
    torch.cuda.synchronize()


# ---- model level ----

IN_SHAPE = [2, 2, 8, 8, 8, 1]
T_OUT = 10
MODES = (2, 2, 2, 3)


def _model(width, dtype, device="cpu", in_shape=IN_SHAPE, t_out=T_OUT,
           modes=MODES, num_blocks=2):
    _, P_x, _ = dfno.create_standard_partitions((1,) * len(in_shape))
    return dfno.DistributedFNONd(P_x, in_shape, t_out, width, modes,
                                 num_blocks=num_blocks,
                                 device=torch.device(device), dtype=dtype)


def _cast_state(sd, dtype):
    cdtype = torch.complex128 if dtype == F64 else torch.complex64
    out = {}
    for k, v in sd.items():
        if v.is_complex():
            out[k] = v.to(cdtype)
        elif v.is_floating_point():
            out[k] = v.to(dtype)
        else:
            out[k] = v
    return out


def _step(model, x, gy):
    y = model(x)
    y.backward(gy)
    grads = {n: p.grad.detach().cpu() for n, p in model.named_parameters()
             if p.grad is not None and p.grad.numel() > 0}
    return y.detach().cpu(), grads


_REF = {}


def _reference(width):
    """CPU fp64 model, its input and output gradient, and its results;
    computed once per width and left unchanged."""
    if width not in _REF:
        torch.manual_seed(200 + width)
        m64 = _model(width, F64)
        x = torch.rand(*IN_SHAPE, dtype=F64)
        y = m64(x)
        gy = torch.rand_like(y)
        y.backward(gy)
        grads = {n: p.grad.detach().clone() for n, p in m64.named_parameters()
                 if p.grad is not None and p.grad.numel() > 0}
        _REF[width] = (m64.state_dict(), x, gy, y.detach(), grads)
    return _REF[width]


def _cmx(t):
    return float(torch.view_as_real(t).abs().max() if t.is_complex()
                 else t.abs().max())


@pytest.mark.parametrize("width", [40, 64])
def test_wide_model_fp32_all_native(width):
    sd, x, gy, y64, g64 = _reference(width)
    cpu = _model(width, F32)
    cpu.load_state_dict(_cast_state(sd, F32))
    y_cpu, g_cpu = _step(cpu, x.float(), gy.float())

    dispatch.reset_fallbacks()
    gpu = _model(width, F32, "cuda")
    gpu.load_state_dict({k: v.cuda() for k, v in _cast_state(sd, F32).items()})
    y_gpu, g_gpu = _step(gpu, x.float().cuda(), gy.float().cuda())
    torch.cuda.synchronize()
    dispatch.assert_all_native()

    assert set(g_gpu) == set(g_cpu) == set(g64)
    tensors = [("y", y_gpu, y_cpu, y64)] + [
        (n, g_gpu[n], g_cpu[n], g64[n]) for n in sorted(g64)]
    bad = []
    for n, a_gpu, a_cpu, a64 in tensors:
        cd = torch.complex128 if a64.is_complex() else F64
        d_cpu = _cmx(a_cpu.to(cd) - a64)
        d_gpu = _cmx(a_gpu.to(cd) - a64)
        bound = 10 * d_cpu + 1e-6 * _cmx(a64)
        print(f"{n}: d_gpu {d_gpu:.3e} d_cpu {d_cpu:.3e} bound {bound:.3e} "
              f"max {_cmx(a64):.3e}")
        if not d_gpu <= bound:
            bad.append((n, d_gpu, bound))
    assert not bad, f"outside 10 * d_cpu + 1e-6 * max: {bad}"


def test_wide_model_fp64_all_native():
    sd, x, gy, _, _ = _reference(40)
    dispatch.reset_fallbacks()
    gpu = _model(40, F64, "cuda")
    gpu.load_state_dict({k: v.cuda() for k, v in sd.items()})
    _step(gpu, x.cuda(), gy.cuda())
    torch.cuda.synchronize()
    dispatch.assert_all_native()


def test_wide_model_bf16_keeps_composed_lift(monkeypatch):
    """bf16 is not in lift_head_wide_range (the fused bf16 lift lost at the
    width-64 Navier-Stokes shape): the model must not call the fused op."""
    import dfno_amd.ops as ops
    torch.manual_seed(264)
    model = _model(64, BF16, "cuda")
    calls = []
    real = ops.lift_head

    def spy(x, *a):
        calls.append(tuple(x.shape))
        return real(x, *a)

    monkeypatch.setattr(ops, "lift_head", spy)
    x = torch.rand(*IN_SHAPE, device="cuda", dtype=BF16)
    dispatch.reset_fallbacks()
    y = model(x)
    y.float().square().mean().backward()
    torch.cuda.synchronize()
    assert calls == []
    assert y.dtype == BF16 and torch.isfinite(y.float()).all()
    for p in (model.linear1.W, model.linear1.b, model.linear2.W, model.linear2.b):
        assert p.grad is not None and torch.isfinite(p.grad.float()).all()
    dispatch.assert_all_native()


def test_wide_ns_model_fp32_all_native():
    torch.manual_seed(240)
    in_shape = [2, 1, 16, 16, 10]
    model = _model(40, F32, "cuda", in_shape=in_shape, t_out=40,
                   modes=(4, 4, 4), num_blocks=1)
    x = torch.rand(*in_shape, device="cuda")
    dispatch.reset_fallbacks()
    y = model(x)
    y.square().mean().backward()
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    dispatch.assert_all_native()
