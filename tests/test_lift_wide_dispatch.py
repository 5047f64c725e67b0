"""Host predicates of the fused lift head at widths 25..64 (no GPU).

``lift_head_wide_range`` is the pure range predicate of the wide kernel rows;
``lift_head_supported`` stays the predicate of the narrow rows and is false
for any CPU tensor.  bf16 is not in the wide range: the fused bf16 lift lost
to the composed one at the width-64 Navier-Stokes shape
(profiles/optimization_log.md, "Lift head for widths 25-64").
"""

import pytest
import torch

from dfno_amd.ops import lift_head_supported, lift_head_wide_range

DTYPES = [torch.float32, torch.float64]
ALL_DTYPES = DTYPES + [torch.bfloat16]
DIMS = [(1, 30, 2), (10, 40, 1), (16, 64, 4)]     # (t_in, t_out, c_in)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("width", [25, 33, 40, 64])
@pytest.mark.parametrize("t_in,t_out,c_in", DIMS)
def test_wide_range_true(dtype, width, t_in, t_out, c_in):
    assert lift_head_wide_range(dtype, t_in, t_out, c_in, width) is True


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("t_in,t_out,c_in,width", [
    (10, 40, 1, 24),      # the narrow rows' last width
    (10, 40, 1, 65),
    (10, 40, 1, 0),
    (17, 40, 1, 40),
    (10, 65, 1, 40),
    (10, 40, 5, 40),
])
def test_wide_range_false(dtype, t_in, t_out, c_in, width):
    assert lift_head_wide_range(dtype, t_in, t_out, c_in, width) is False


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("width", [25, 33, 40, 64])
def test_wide_range_refuses_fp16_and_bf16(dtype, width):
    for t_in, t_out, c_in in DIMS:
        assert not lift_head_wide_range(dtype, t_in, t_out, c_in, width)


@pytest.mark.parametrize("dtype", ALL_DTYPES)
def test_supported_is_false_on_cpu(dtype):
    x = torch.empty(1, dtype=dtype)
    for width in (1, 20, 24, 25, 33, 40, 64, 65):
        for t_in, t_out, c_in in DIMS:
            assert not lift_head_supported(x, t_in, t_out, c_in, width)
