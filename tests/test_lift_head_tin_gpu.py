"""Fused lift head for multi-step inputs (T_in > 1, T_out <= 64).

Op-level forward+backward against plain torch (fp64 reference for the
fp32/fp64 cases, fp32 for bf16), gradcheck, the support gate, and the
Navier-Stokes-shaped model running fully native.
"""

import pytest
import torch
import torch.nn.functional as F

import dfno_amd as dfno

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16


def _inputs(dtype, B, C, S, Ti, To, W, seed=31):
    torch.manual_seed(seed)
    dev = "cuda"
    x = torch.randn(B, C, S, Ti, device=dev, dtype=dtype)
    W1 = torch.randn(To, Ti, device=dev, dtype=dtype)
    b1 = torch.randn(To, device=dev, dtype=dtype)
    W2 = torch.randn(W, C, device=dev, dtype=dtype) / C
    b2 = torch.randn(W, device=dev, dtype=dtype)
    gy = torch.randn(B, W, S, To, device=dev, dtype=dtype)
    return [x, W1, b1, W2, b2], gy


def _reference(ts, gy, ref_dtype):
    xr, W1r, b1r, W2r, b2r = [t.detach().to(ref_dtype).requires_grad_(True)
                              for t in ts]
    h = F.gelu(torch.einsum("ti,bcsi->bcst", W1r, xr) + b1r.view(1, 1, 1, -1))
    yr = F.gelu(torch.einsum("wc,bcst->bwst", W2r, h) + b2r.view(1, -1, 1, 1))
    yr.backward(gy.to(ref_dtype))
    return yr.detach(), [t.grad for t in (xr, W1r, b1r, W2r, b2r)]


def _check(dtype, B, C, S, Ti, To, W):
    from dfno_amd.ops import lift_head
    ts, gy = _inputs(dtype, B, C, S, Ti, To, W)
    ts = [t.requires_grad_(True) for t in ts]
    y = lift_head(*ts)
    assert y.shape == (B, W, S, To) and y.dtype == dtype
    y.backward(gy)
    torch.cuda.synchronize()
    ref_dtype = torch.float32 if dtype == BF16 else torch.float64
    yr, gr = _reference(ts, gy, ref_dtype)

    names = ["gx", "gW1", "gb1", "gW2", "gb2"]
    if dtype == BF16:
        tols = [(2e-2, 2e-2), (5e-2, 5e-2)] + [(5e-2, 5e-1)] * 4
    elif dtype == F32:
        tols = [(3e-4, 3e-4)] + [(9e-3, 9e-3)] * 5
    else:
        tols = [(1e-10, 1e-10)] * 6
    got = [y] + [t.grad for t in ts]
    want = [yr] + gr
    for n, a, b, (rt, at) in zip(["fwd"] + names, got, want, tols):
        assert a.shape == b.shape, n
        err = (a.to(ref_dtype) - b).abs().max().item()
        print(f"{n}: max abs err {err:.3e} (max |ref| {b.abs().max().item():.3e})")
    for n, a, b, (rt, at) in zip(["fwd"] + names, got, want, tols):
        assert torch.allclose(a.to(ref_dtype), b, rtol=rt, atol=at), \
            f"{n}: max {(a.to(ref_dtype) - b).abs().max()}"


# 1: NS pins, one point per wave; odd S -> a wave's points cross the batch
#    boundary and the tail is partial
@pytest.mark.parametrize("dtype", [F32, F64, BF16])
def test_lift_ns_pins_odd_s(dtype):
    _check(dtype, B=2, C=1, S=37, Ti=10, To=40, W=20)


# 2: two points per wave, unpinned W, odd point count (half-empty last pair)
@pytest.mark.parametrize("dtype", [F32, F64])
def test_lift_two_points_per_wave(dtype):
    _check(dtype, B=1, C=3, S=129, Ti=4, To=6, W=12)


# 3: every cap at its limit, less than one block of work
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_lift_all_caps(dtype):
    _check(dtype, B=1, C=4, S=5, Ti=16, To=64, W=24)


# 4: first To past the 32-lane layout; W = 1; S = 1
def test_lift_to33_w1_s1():
    _check(F32, B=3, C=2, S=1, Ti=2, To=33, W=1)


# 5: B*S = 16411 points at one point per wave: more than twice the 8192
#    waves of the forward grid (2048 blocks) and five times the 3072 of the
#    backward grid (768 blocks), so every wave iterates and every block
#    lands on the same weight-grad atomics
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_lift_large_s(dtype):
    _check(dtype, B=1, C=1, S=16411, Ti=10, To=40, W=20)


# 6: Ti == 1 with 32 < To <= 64 is routed to the general kernels
def test_lift_tin1_wide_tout():
    _check(F32, B=1, C=2, S=50, Ti=1, To=48, W=20)


# 7: the launch rows <LP, TIC, WT> that no case above lands on (LP 32 / 64
#    lanes per point by To <= 32, TIC 4 / 16 by Ti <= 4, WT 20 at width 20,
#    else 0); S = 45 is an odd point count over more than one block
@pytest.mark.parametrize("dtype,Ti,To,W", [
    (F32, 3, 20, 20),     # <32, 4, 20>
    (F32, 12, 30, 20),    # <32, 16, 20>
    (F32, 12, 30, 7),     # <32, 16, 0>
    (BF16, 3, 20, 20),
    (BF16, 12, 30, 20),
    (BF16, 12, 30, 7),
    (BF16, 4, 6, 12),     # <32, 4, 0>
    (BF16, 3, 50, 9),     # <64, 4, 0>
    (BF16, 3, 50, 20),    # <64, 4, 20>
])
def test_lift_launch_rows(dtype, Ti, To, W):
    _check(dtype, B=1, C=2, S=45, Ti=Ti, To=To, W=W)


def test_lift_gradcheck_fp64():
    from dfno_amd.ops import lift_head
    ts, _ = _inputs(F64, B=1, C=2, S=3, Ti=3, To=5, W=4)
    ts = [t.requires_grad_(True) for t in ts]
    # weight grads go through atomics: allow last-bit reordering noise
    assert torch.autograd.gradcheck(lift_head, ts, nondet_tol=1e-12)


def test_lift_gate():
    from dfno_amd import _ext
    from dfno_amd.ops import lift_head_supported
    for dtype in (F32, BF16, F64):
        x = torch.empty(1, device="cuda", dtype=dtype)
        assert lift_head_supported(x, 10, 40, 1, 20)
        assert not lift_head_supported(x, 17, 40, 1, 20)
        assert not lift_head_supported(x, 10, 65, 1, 20)
        assert not lift_head_supported(x, 10, 40, 5, 20)
        assert not lift_head_supported(x, 10, 40, 1, 25)
        assert not lift_head_supported(x.cpu(), 10, 40, 1, 20)
        assert not lift_head_supported(x.cpu(), 1, 30, 1, 20)

    # the extension itself refuses an over-cap call before any launch
    ext = _ext.get(required=True)
    ts, gy = _inputs(F32, B=1, C=1, S=4, Ti=17, To=8, W=4)
    with pytest.raises(RuntimeError, match="unsupported dims"):
        ext.lift_head_fwd(*ts)
    with pytest.raises(RuntimeError, match="unsupported dims"):
        ext.lift_head_bwd(gy, *ts)
    # the [B,C,S] form (T_in == 1) goes through the same checks
    ts, gy = _inputs(F32, B=1, C=2, S=4, Ti=1, To=8, W=4)
    x3 = ts[0].reshape(1, 2, 4)
    with pytest.raises(RuntimeError, match="gy shape"):
        ext.lift_head_bwd(gy[..., :7].contiguous(), x3, *ts[1:])
    W2bad = torch.randn(4, 3, device="cuda")              # W2.size(1) != C
    with pytest.raises(RuntimeError, match="lift_head shapes"):
        ext.lift_head_fwd(x3, ts[1], ts[2], W2bad, ts[4])
    ts, gy = _inputs(F32, B=1, C=1, S=4, Ti=1, To=33, W=4)
    with pytest.raises(RuntimeError, match="unsupported dims"):
        ext.lift_head_fwd(ts[0].reshape(1, 1, 4), *ts[1:])
    torch.cuda.synchronize()


def _model(in_shape, t_out, width, modes, device, dtype=F32):
    _, P_x, _ = dfno.create_standard_partitions((1,) * len(in_shape))
    return dfno.DistributedFNONd(P_x, in_shape, t_out, width, modes,
                                 num_blocks=1, device=torch.device(device),
                                 dtype=dtype)


def _compare_with_cpu(gpu_model, cpu_model, in_shape):
    cpu_model.load_state_dict({k: v.cpu()
                               for k, v in gpu_model.state_dict().items()})
    x = torch.rand(*in_shape)
    y_cpu = cpu_model(x)
    y_gpu = gpu_model(x.cuda())
    y_cpu.square().mean().backward()
    y_gpu.square().mean().backward()
    torch.cuda.synchronize()
    assert torch.allclose(y_gpu.cpu(), y_cpu, rtol=3e-4, atol=3e-4), \
        f"max {(y_gpu.cpu() - y_cpu).abs().max()}"
    for (n, pc), (_, pg) in zip(cpu_model.named_parameters(),
                                gpu_model.named_parameters()):
        if pc.grad is None:
            assert pg.grad is None or pg.grad.numel() == 0
            continue
        assert torch.allclose(pg.grad.cpu(), pc.grad, rtol=3e-3, atol=3e-3), \
            f"{n}: max {(pg.grad.cpu() - pc.grad).abs().max()}"


def test_ns_model_fp32_all_native():
    from dfno_amd import dispatch
    torch.manual_seed(7)
    in_shape = [2, 1, 16, 16, 10]
    gpu_model = _model(in_shape, 40, 20, (4, 4, 4), "cuda")
    cpu_model = _model(in_shape, 40, 20, (4, 4, 4), "cpu")
    dispatch.reset_fallbacks()
    _compare_with_cpu(gpu_model, cpu_model, in_shape)
    dispatch.assert_all_native()


def test_ns_model_bf16_uses_fused_lift(monkeypatch):
    import dfno_amd.ops as ops
    from dfno_amd import dispatch
    torch.manual_seed(8)
    in_shape = [1, 1, 32, 32, 10]
    model = _model(in_shape, 40, 20, (4, 4, 4), "cuda", BF16)
    calls = []
    real = ops.lift_head

    def spy(x, *a):
        calls.append(tuple(x.shape))
        return real(x, *a)

    monkeypatch.setattr(ops, "lift_head", spy)
    x = torch.rand(*in_shape, device="cuda", dtype=BF16)
    dispatch.reset_fallbacks()
    y = model(x)
    y.float().square().mean().backward()
    torch.cuda.synchronize()
    assert calls == [tuple(in_shape)]
    assert y.dtype == BF16 and torch.isfinite(y.float()).all()
    for p in (model.linear1.W, model.linear1.b, model.linear2.W, model.linear2.b):
        assert p.grad is not None and torch.isfinite(p.grad.float()).all()
    dispatch.assert_all_native()


def test_out_of_range_lift_still_composed():
    from dfno_amd import dispatch
    torch.manual_seed(9)
    in_shape = [1, 2, 8, 8, 17]
    gpu_model = _model(in_shape, 6, 12, (2, 2, 2), "cuda")
    cpu_model = _model(in_shape, 6, 12, (2, 2, 2), "cpu")
    dispatch.reset_fallbacks()
    _compare_with_cpu(gpu_model, cpu_model, in_shape)
    assert any(op == "lift_head" for op, _ in dispatch.fallback_counts())
    dispatch.reset_fallbacks()
