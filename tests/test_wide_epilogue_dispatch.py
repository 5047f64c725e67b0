"""Range predicates of the fused irfft epilogue and its adjoint mode
(ops/epilogue.py).

The entry points take up to 64 channels on either side in fp32, but the wide
kernel lost to the pairs it would replace at the width-64 flagship shape
(profiles/optimization_log.md, "Time-axis irfft in the wide epilogue"), so the
predicates, which route the model, stay at the 32-channel range: nothing past
it, nothing but fp32, and exactly what they said before at 32 and below."""

import pytest
import torch

from dfno_amd.ops.epilogue import fused_epilogue_ok, rfft_adj_mix_ok

PREDS = [fused_epilogue_ok, rfft_adj_mix_ok]


@pytest.mark.parametrize("ok", PREDS)
@pytest.mark.parametrize("n,m", [(30, 8), (10, 3)])
def test_wide_widths_not_routed(ok, n, m):
    for w in (33, 40, 48, 64, 65):
        assert not ok(torch.float32, w, w, n, m), w


@pytest.mark.parametrize("ok", PREDS)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float64])
def test_other_dtypes_never(ok, dtype):
    for w in (8, 20, 32, 33, 40, 64, 65):
        assert not ok(dtype, w, w, 30, 8), w


def test_narrow_range_unchanged():
    assert fused_epilogue_ok(torch.float32, 20, 20, 30, 8)
    assert rfft_adj_mix_ok(torch.float32, 20, 20, 30, 8)
    # the register-resident side stops at 32, the other at 64
    assert fused_epilogue_ok(torch.float32, 32, 64, 30, 8)
    assert not fused_epilogue_ok(torch.float32, 33, 32, 30, 8)
    assert rfft_adj_mix_ok(torch.float32, 64, 32, 30, 8)
    assert not rfft_adj_mix_ok(torch.float32, 32, 33, 30, 8)
    # time extent and modes: as before
    assert not fused_epilogue_ok(torch.float32, 20, 20, 65, 8)
    assert not fused_epilogue_ok(torch.float32, 20, 20, 30, 17)
    assert not rfft_adj_mix_ok(torch.float32, 20, 20, 65, 8)
    assert not rfft_adj_mix_ok(torch.float32, 20, 20, 30, 17)
    assert not fused_epilogue_ok(torch.float32, 0, 20, 30, 8)
