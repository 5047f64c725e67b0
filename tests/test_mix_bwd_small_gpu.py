"""Fused trunk mix backward (csrc/mix_bwd.hip) at tile-edge sizes, against
the composition of tests/test_kernels_gpu.py evaluated in fp64:
gz = gy * gelu'(z), gx = W^T gz, gW = gz x^T, gb = sum gz.

Bounds: max abs error of each output, per IO dtype, over all the cases
below.  Each bound is 4x the largest error the kernel had before its MFMA
operands became unconditional 16-byte reads (measured with ``errors`` on
that build):

    measured max abs error   gx        gW        gb        gz
    fp32                     1.475e-7  5.446e-6  2.673e-6  4.489e-7
    bf16                     1.948e-3  5.842e-6  5.592e-6  7.774e-3
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C, B = 20, 2
NAMES = ("gx", "gW", "gb", "gz")

# 4 x the measured values in the module docstring
BOUNDS = {
    torch.float32: dict(gx=5.898e-7, gW=2.178e-5, gb=1.069e-5, gz=1.796e-6),
    torch.bfloat16: dict(gx=7.790e-3, gW=2.337e-5, gb=2.237e-5, gz=3.110e-2),
}


@pytest.fixture(scope="module")
def ext():
    from dfno_amd import _ext
    e = _ext.get(required=True)
    assert e is not None
    return e


def make_inputs(S, dtype):
    g = torch.Generator(device="cuda").manual_seed(31 + S)
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    x, z, gy = (r(B, C, S).to(dtype) for _ in range(3))
    return gy, z, x, r(C, C) / C


_REF = {}


def reference(S, dtype):
    key = (S, dtype)
    if key not in _REF:
        gy, z, x, W = (t.double() for t in make_inputs(S, dtype))
        z.requires_grad_(True)
        gz = gy * torch.autograd.grad(F.gelu(z).sum(), z)[0]
        _REF[key] = dict(gx=torch.einsum("oi,bos->bis", W, gz),
                         gW=torch.einsum("bos,bis->oi", gz, x),
                         gb=gz.sum(dim=(0, 2)), gz=gz)
    return _REF[key]


def errors(ext, S, dtype, bias, want_gx):
    """max abs error of each produced output against the fp64 reference"""
    gy, z, x, W = make_inputs(S, dtype)
    outs = ext.channel_mix_bwd_fused(gy, z, x, W, bias, True, want_gx)
    ref = reference(S, dtype)
    err = {}
    for name, o in zip(NAMES, outs):
        if (name == "gx" and not want_gx) or (name == "gb" and not bias):
            assert o.numel() == 0, name
            continue
        assert o.shape == ref[name].shape, name
        err[name] = float((o.double() - ref[name]).abs().max())
    return err


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("want_gx", [True, False])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("S", [1, 63, 65])
def test_channel_mix_bwd_fused_small(ext, S, bias, want_gx, dtype):
    err = errors(ext, S, dtype, bias, want_gx)
    print(f"S={S} bias={bias} want_gx={want_gx} {dtype}: " +
          " ".join(f"{k}={v:.3e}" for k, v in err.items()))
    for name, v in err.items():
        assert v <= BOUNDS[dtype][name], \
            f"{name}: {v:.3e} > {BOUNDS[dtype][name]:.3e}"
