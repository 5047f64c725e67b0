"""Fused projection-head backward (csrc/proj_head.hip,
proj_head_bwd_fused_kernel) against an fp64 torch composition of the same
inputs, at the shapes where its 64-column tiling can go wrong.

Bounds: max abs error of each output, per IO dtype, over all the cases
below.  Each bound is 4x the largest error the kernel had before its MFMA
phases were reworked (measured with ``errors`` below on that build; the
margin covers the run-to-run atomic order of the weight sums):

    measured max abs error   gx        gW3       gb3       gW4       gb4
    fp32                     6.565e-7  9.216e-5  5.929e-5  1.114e-3  3.375e-4
    bf16                     3.901e-3  1.046e-4  5.098e-5  1.064e-3  1.201e-4
"""

import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

I, M = 20, 128
NAMES = ("gx", "gW3", "gb3", "gW4", "gb4")

# (B, S): one column; one short of a tile; exactly a tile; a tail tile of one
# column across the batch; several tiles plus a tail, batched; more tiles
# than the 768 blocks of the grid, so a block carries its fragments over a
# wrap
SHAPES = [(1, 1), (1, 63), (1, 64), (2, 65), (2, 64 * 5 + 17),
          (1, 64 * 769 + 5)]

# 4 x the measured values in the module docstring
BOUNDS = {
    torch.float32: dict(gx=2.626e-6, gW3=3.686e-4, gb3=2.372e-4, gW4=4.455e-3,
                        gb4=1.350e-3),
    torch.bfloat16: dict(gx=1.560e-2, gW3=4.185e-4, gb3=2.039e-4, gW4=4.256e-3,
                         gb4=4.805e-4),
}


@pytest.fixture(scope="module")
def ext():
    from dfno_amd import _ext
    e = _ext.get(required=True)
    assert e is not None
    return e


def make_inputs(B, S, O2, dtype):
    g = torch.Generator(device="cuda").manual_seed(1000 * B + S + 7 * O2)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    x = r(B, I, S).to(dtype)
    W3 = (r(M, I) / math.sqrt(I)).to(dtype)
    b3 = r(M).to(dtype)
    W4 = (r(O2, M) / math.sqrt(M)).to(dtype)
    gy = r(B, O2, S).to(dtype)
    return gy, x, W3, b3, W4


_REF = {}


def reference(B, S, O2, dtype):
    """fp64 gradients of W4 @ gelu(W3 @ x + b3) + b4 (computed once per
    case and shared)."""
    key = (B, S, O2, dtype)
    if key not in _REF:
        gy, x, W3, b3, W4 = (t.double() for t in make_inputs(B, S, O2, dtype))
        leaves = [t.requires_grad_(True) for t in (x, W3, b3, W4)]
        x, W3, b3, W4 = leaves
        h = F.gelu(torch.einsum("mi,bis->bms", W3, x) + b3.view(1, -1, 1))
        y = torch.einsum("om,bms->bos", W4, h)
        gx, gW3, gb3, gW4 = torch.autograd.grad(y, leaves, gy)
        _REF[key] = dict(gx=gx, gW3=gW3, gb3=gb3, gW4=gW4,
                         gb4=gy.sum(dim=(0, 2)))
    return _REF[key]


def errors(ext, B, S, O2, dtype):
    """max abs error of each output against the fp64 reference"""
    outs = ext.proj_head_bwd_fused(*make_inputs(B, S, O2, dtype))
    ref = reference(B, S, O2, dtype)
    assert outs[0].dtype == dtype
    assert all(o.dtype == torch.float32 for o in outs[1:])
    err = {}
    for name, o in zip(NAMES, outs):
        assert o.shape == ref[name].shape, name
        err[name] = float((o.double() - ref[name]).abs().max())
    return err


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("O2", [1, 2])
@pytest.mark.parametrize("B,S", SHAPES)
def test_proj_head_bwd_fused(ext, B, S, O2, dtype):
    err = errors(ext, B, S, O2, dtype)
    print(f"B={B} S={S} O2={O2} {dtype}: " +
          " ".join(f"{k}={v:.3e}" for k, v in err.items()))
    for name in NAMES:
        assert err[name] <= BOUNDS[dtype][name], \
            f"{name}: {err[name]:.3e} > {BOUNDS[dtype][name]:.3e}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("O2", [1, 2])
@pytest.mark.parametrize("B,S", [(1, 1), (2, 65), (1, 64 * 769 + 5)])
def test_zero_gy_gives_exact_zeros(ext, B, S, O2, dtype):
    """gz = (W4^T gy) gelu' is zero, so every output is exactly zero: a
    padded MFMA row or column that leaked into a kept output would show."""
    gy, x, W3, b3, W4 = make_inputs(B, S, O2, dtype)
    outs = ext.proj_head_bwd_fused(torch.zeros_like(gy), x, W3, b3, W4)
    for name, o in zip(NAMES, outs):
        assert int(torch.count_nonzero(o)) == 0, name
