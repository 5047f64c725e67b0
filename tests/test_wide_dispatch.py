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


def test_mix_t_slab():
    """gx = W^T gz goes through channel_mix_fwd_t in one call wherever one of
    its kernels takes the shape, and in 16-row output slabs where only the
    LDS-staged one is left and its tile does not fit 160 KiB."""
    from dfno_amd.ops.pointwise import mix_t_slab
    f32, f64 = torch.float32, torch.float64
    assert mix_t_slab(f64, 512, 32) == 16      # 8 * (512*32 + 32*512 + 32) B
    assert mix_t_slab(f64, 128, 20) == 0       # 8 * (128*32 + 20*128 + 20) fits
    assert mix_t_slab(f64, 512, 16) == 0       # accumulator kernel, one call
    assert mix_t_slab(f64, 32, 512) == 0       # x-resident kernel
    assert mix_t_slab(f32, 512, 32) == 0       # fp32 accumulators to 32 rows
    assert mix_t_slab(f32, 20, 20) == 0
    assert mix_t_slab(torch.bfloat16, 512, 32) == 0


def test_proj_head_range():
    """Support of the fused projection head as ops/projhead.py states it:
    the caps I <= 32, M <= 512, O2 <= 8 and the LDS bound of the backward
    (160 KiB) in fp32 / fp64, the pinned 20 -> 128 -> (<= 2) shape in bf16;
    the one-kernel backward at the pinned shape in fp32 / bf16 only.
    proj_head_supported is this plus x.is_cuda."""
    from dfno_amd.ops.projhead import (proj_head_bwd_lds, proj_head_fused_bwd,
                                       proj_head_range, proj_head_supported)
    f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
    assert proj_head_range(f32, 20, 128, 1)
    assert proj_head_bwd_lds(4, 32, 512, 8) == 157696
    assert proj_head_range(f32, 32, 512, 8)
    assert proj_head_bwd_lds(8, 20, 512, 1) == 122880
    assert proj_head_range(f64, 20, 512, 1)
    assert proj_head_bwd_lds(8, 32, 512, 2) == 192512
    assert not proj_head_range(f64, 32, 512, 2)
    assert not proj_head_range(f32, 33, 128, 1)
    assert not proj_head_range(bf16, 12, 64, 1)
    assert proj_head_range(bf16, 20, 128, 2)
    assert not proj_head_range(torch.float16, 20, 128, 1)

    assert proj_head_fused_bwd(f32, 20, 128, 1)
    assert proj_head_fused_bwd(bf16, 20, 128, 2)
    assert not proj_head_fused_bwd(f64, 20, 128, 1)
    assert not proj_head_fused_bwd(f32, 12, 64, 1)
    assert not proj_head_fused_bwd(f32, 20, 128, 3)

    # host tensors never take the fused head
    assert not proj_head_supported(torch.zeros(1), 20, 128, 1)
