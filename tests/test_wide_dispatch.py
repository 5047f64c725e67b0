"""Range predicate of the wide channel-mix route (ops/pointwise.py).

Pure host logic: which (dtype, I, O, S) the wide kernel takes.  Everything
at I, O <= 32 must stay on the routes it had.
"""

import pytest
import torch

from dfno_amd.ops.pointwise import _wide_mix_ok, wide_mix_range

DTYPES = [torch.float32, torch.bfloat16, torch.float64, torch.float16]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("I,O", [(1, 1), (8, 8), (20, 20), (20, 32), (32, 20),
                                 (32, 32), (2, 20), (24, 1)])
def test_narrow_shapes_keep_their_routes(dtype, I, O):
    for S in (8, 64, 515, 4096):
        assert not wide_mix_range(dtype, I, O, S)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("I,O", [(33, 33), (64, 64), (64, 128), (128, 64),
                                 (40, 30), (128, 128)])
def test_wide_shapes_in_range(dtype, I, O):
    assert wide_mix_range(dtype, I, O, 64)
    assert wide_mix_range(dtype, I, O, 70008)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("I,O", [(129, 64), (64, 129), (256, 256), (0, 64),
                                 (64, 0)])
def test_out_of_range(dtype, I, O):
    assert not wide_mix_range(dtype, I, O, 64)


def test_bf16_needs_whole_vectors():
    for S in (5, 12, 515, 70001):
        assert not wide_mix_range(torch.bfloat16, 64, 64, S)
        assert wide_mix_range(torch.float32, 64, 64, S)
    assert wide_mix_range(torch.bfloat16, 64, 64, 8)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16, torch.complex64])
def test_other_dtypes_have_no_wide_kernel(dtype):
    assert not wide_mix_range(dtype, 64, 64, 64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_tensors_never_take_it(dtype):
    x = torch.zeros(1, 64, 64, dtype=dtype)
    assert wide_mix_range(dtype, 64, 64, 64)
    assert not _wide_mix_ok(x, 64, 64)


def test_grad_w_caps():
    """The caps of the grad-W entry points as ops/pointwise.py states them:
    64 x rows in fp32 / fp64 (gz rows unbounded, so the role swap asks with
    the sides exchanged), and for bf16 also 128 gz rows and S % 128 == 0."""
    from dfno_amd.ops.pointwise import grad_w_caps_ok
    for dtype in (torch.float32, torch.float64):
        assert grad_w_caps_ok(dtype, 64, 4096, 1003)
        assert not grad_w_caps_ok(dtype, 65, 1, 1024)
        assert grad_w_caps_ok(dtype, 1, 128, 777)      # linear4, roles swapped
    assert grad_w_caps_ok(torch.bfloat16, 64, 128, 384)
    assert not grad_w_caps_ok(torch.bfloat16, 65, 128, 384)
    assert not grad_w_caps_ok(torch.bfloat16, 64, 129, 384)
    assert not grad_w_caps_ok(torch.bfloat16, 20, 20, 1000)
