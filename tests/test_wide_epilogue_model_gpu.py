"""Model-level routing of the fused irfft epilogue and its adjoint mode at
trunk widths 40 and 64 (fp32), with the two knobs at their defaults and off.

Both modes of the wide kernel lost their A/B at the width-64 flagship shape
(profiles/optimization_log.md), so the predicates keep wide blocks on the
composed route: the expected call counts are 0 in every setting, and the
knobs change nothing at these widths.

Model, reference and bound are those of tests/test_wide_model_gpu.py: every
tensor (output and each parameter gradient) must satisfy
max|gpu - fp64| <= 10 * d_cpu + 1e-6 * max|fp64| against the CPU fp64 model,
with d_cpu = max|cpu_fp32 - fp64| measured here.  No fixed atol: max|y| is
about 2e-3 at this shape."""

import pytest
import torch

from test_wide_model_gpu import _cast_state, _model, _mx, _reference, _step

pytestmark = pytest.mark.gpu

_CPU32 = {}


def _cpu_fp32(width):
    """The CPU fp32 model's results, once per width, left unchanged."""
    if width not in _CPU32:
        sd, x, gy, _, _ = _reference(width)
        cpu = _model(width, torch.float32)
        cpu.load_state_dict(_cast_state(sd, torch.float32))
        _CPU32[width] = _step(cpu, x.float(), gy.float())
    return _CPU32[width]


# (DFNO_FUSED_EPILOGUE, DFNO_FUSED_RFFT_ADJ) -> expected calls of
# (_IrfftLinearResGeluFn.apply, ext.rfft_adj_mix) over one forward + backward
# of the 2-block model
KNOBS = [
    (None, None, 0, 0),
    ("0", None, 0, 0),
    (None, "0", 0, 0),
]


@pytest.mark.parametrize("epi,adj,n_fwd,n_adj", KNOBS)
@pytest.mark.parametrize("width", [40, 64])
def test_wide_model_epilogue_routes(monkeypatch, width, epi, adj, n_fwd, n_adj):
    import dfno_amd.ops.epilogue as epilogue
    from dfno_amd import _ext, dispatch
    from dfno_amd.ops.fft import _GRAD_STASH

    ext = _ext.get(required=True)
    for name, val in (("DFNO_FUSED_EPILOGUE", epi), ("DFNO_FUSED_RFFT_ADJ", adj)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)

    fwd_calls, adj_calls = [], []
    orig_apply = epilogue._IrfftLinearResGeluFn.apply
    orig_adj = ext.rfft_adj_mix
    monkeypatch.setattr(epilogue._IrfftLinearResGeluFn, "apply",
                        lambda *a: (fwd_calls.append(1), orig_apply(*a))[1])
    monkeypatch.setattr(ext, "rfft_adj_mix",
                        lambda *a: (adj_calls.append(1), orig_adj(*a))[1])

    sd, x, gy, y64, g64 = _reference(width)
    y_cpu, g_cpu = _cpu_fp32(width)

    dispatch.reset_fallbacks()
    gpu = _model(width, torch.float32, "cuda")
    gpu.load_state_dict({k: v.cuda() for k, v in
                         _cast_state(sd, torch.float32).items()})
    y_gpu, g_gpu = _step(gpu, x.float().cuda(), gy.float().cuda())
    torch.cuda.synchronize()

    assert (len(fwd_calls), len(adj_calls)) == (n_fwd, n_adj)
    assert not dispatch.fallback_counts(), dispatch.fallback_counts()
    assert not _GRAD_STASH, "gradient stash not drained"

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
