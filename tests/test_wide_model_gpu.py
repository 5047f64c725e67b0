"""Whole-model tests at trunk widths 40 and 64 (past the 32-channel kernels).

Every trunk and projection-head op has to run on the native kernels: after a
forward + backward the only fallback note allowed is the lift head's (it stays
capped at width 24), nothing raises and the gradient stash is empty.

fp32 bound.  The reference is the CPU fp64 model.  For each tensor (output and
every parameter gradient) d_cpu = max|cpu_fp32 - fp64| is measured in the test
and the GPU must satisfy max|gpu_fp32 - fp64| <= 10 * d_cpu + 1e-6 * max|fp64|:
the factor 10 covers summation-order differences (atomics, MFMA chain against
blocked CPU sums), while a dropped or duplicated channel is a relative error
near 1/width (1.5e-2 at width 64).  A fixed atol would be vacuous here: max|y|
is about 2e-3 at these shapes.

The bound is tight enough to see the transforms: blocks.N.weights.4 (high modes
of the last spatial dim, DC in all others, DC-heavy torch.rand input) sat at
1.0e-8 against a bound of 4.0e-9 while the generic c2c kernel took its
recurrence step from sincosf of the unreduced angle; with the reduced step
(csrc/dft.hip mode_step) it measures 7e-10, like the other corners.
"""

import pytest
import torch

import dfno_amd as dfno
from dfno_amd import dispatch
from dfno_amd.ops.fft import _GRAD_STASH

pytestmark = pytest.mark.gpu

IN_SHAPE = [2, 2, 8, 8, 8, 1]
T_OUT = 10
MODES = (2, 2, 2, 3)


def _model(width, dtype, device="cpu"):
    _, P_x, _ = dfno.create_standard_partitions((1, 1, 1, 1, 1, 1))
    return dfno.DistributedFNONd(P_x, IN_SHAPE, T_OUT, width, MODES, num_blocks=2,
                                 device=torch.device(device), dtype=dtype)


def _cast_state(sd, dtype):
    cdtype = {torch.float32: torch.complex64, torch.float64: torch.complex128,
              torch.bfloat16: torch.complex64}[dtype]
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
        torch.manual_seed(100 + width)
        m64 = _model(width, torch.float64)
        x = torch.rand(*IN_SHAPE, dtype=torch.float64)
        y = m64(x)
        gy = torch.rand_like(y)
        y.backward(gy)
        grads = {n: p.grad.detach().clone() for n, p in m64.named_parameters()
                 if p.grad is not None and p.grad.numel() > 0}
        _REF[width] = (m64.state_dict(), x, gy, y.detach(), grads)
    return _REF[width]


def _check_native():
    ops = {op for (op, _) in dispatch.fallback_counts()}
    assert ops <= {"lift_head"}, f"non-native ops: {dispatch.fallback_counts()}"
    assert not _GRAD_STASH, "gradient stash not drained"


def _mx(t):
    return float(torch.view_as_real(t).abs().max() if t.is_complex()
                 else t.abs().max())


@pytest.mark.parametrize("width", [40, 64])
def test_wide_model_fp32(width):
    sd, x, gy, y64, g64 = _reference(width)
    cpu = _model(width, torch.float32)
    cpu.load_state_dict(_cast_state(sd, torch.float32))
    y_cpu, g_cpu = _step(cpu, x.float(), gy.float())

    dispatch.reset_fallbacks()
    gpu = _model(width, torch.float32, "cuda")
    gpu.load_state_dict({k: v.cuda() for k, v in
                         _cast_state(sd, torch.float32).items()})
    y_gpu, g_gpu = _step(gpu, x.float().cuda(), gy.float().cuda())
    torch.cuda.synchronize()
    _check_native()

    assert set(g_gpu) == set(g_cpu) == set(g64)
    tensors = [("y", y_gpu, y_cpu, y64)] + [
        (n, g_gpu[n], g_cpu[n], g64[n]) for n in sorted(g64)]
    bad = []
    for n, a_gpu, a_cpu, a64 in tensors:
        cd = torch.complex128 if a64.is_complex() else torch.float64
        d_cpu = _mx(a_cpu.to(cd) - a64)
        d_gpu = _mx(a_gpu.to(cd) - a64)
        bound = 10 * d_cpu + 1e-6 * _mx(a64)
        print(f"{n}: d_gpu {d_gpu:.3e} d_cpu {d_cpu:.3e} bound {bound:.3e} "
              f"max {_mx(a64):.3e}")
        if not d_gpu <= bound:
            bad.append((n, d_gpu, bound))
    assert not bad, f"outside 10 * d_cpu + 1e-6 * max: {bad}"


def test_wide_model_fp64():
    width = 40
    sd, x, gy, y64, g64 = _reference(width)
    dispatch.reset_fallbacks()
    gpu = _model(width, torch.float64, "cuda")
    gpu.load_state_dict({k: v.cuda() for k, v in sd.items()})
    y_gpu, g_gpu = _step(gpu, x.cuda(), gy.cuda())
    torch.cuda.synchronize()
    _check_native()
    assert torch.allclose(y_gpu, y64, rtol=1e-10, atol=1e-10), \
        f"max {(y_gpu - y64).abs().max()}"
    assert set(g_gpu) == set(g64)
    for n in sorted(g64):
        assert torch.allclose(g_gpu[n], g64[n], rtol=1e-9, atol=1e-9), \
            f"{n}: max {_mx(g_gpu[n] - g64[n])}"


def test_wide_model_bf16():
    """bf16 model against the GPU fp32 model holding the bf16-rounded weights
    (the metric and bound of test_bf16_model_stash_grads)."""
    width = 64
    sd, x, gy, _, _ = _reference(width)
    sd_b = _cast_state(sd, torch.bfloat16)
    ref = _model(width, torch.float32, "cuda")
    ref.load_state_dict({k: (v.float() if v.dtype == torch.bfloat16 else v).cuda()
                         for k, v in sd_b.items()})
    xb = x.cuda().bfloat16()
    gyb = gy.cuda().bfloat16()
    y_ref, g_ref = _step(ref, xb.float(), gyb.float())

    dispatch.reset_fallbacks()
    bf = _model(width, torch.bfloat16, "cuda")
    bf.load_state_dict({k: v.cuda() for k, v in sd_b.items()})
    y_bf, g_bf = _step(bf, xb, gyb)
    torch.cuda.synchronize()
    _check_native()

    assert set(g_bf) == set(g_ref)
    for n, a, b in [("y", y_ref, y_bf)] + [(n, g_ref[n], g_bf[n])
                                           for n in sorted(g_ref)]:
        a, b = a, b.to(a.dtype)
        if a.is_complex():
            a, b = torch.view_as_real(a), torch.view_as_real(b)
        a, b = a.float(), b.float()
        scale = a.abs().max().clamp_min(1e-6)
        rel = float((a - b).abs().max() / scale)
        print(f"{n}: rel {rel:.3e}")
        assert rel < 0.12, f"{n}: rel {rel}"
