"""Deferred spectral grad-W (ops/spectral.py, optim.py): the plumbing, on
CPU.  Without the extension ``step()`` materialises the pending gradients
with the einsum and takes the stock Adam path, so every result here must be
bit-identical to the undeferred one."""

import pytest
import torch

import dfno_amd as dfno
from dfno_amd.optim import Adam


@pytest.fixture
def knob(monkeypatch):
    def set_(on):
        monkeypatch.setenv("DFNO_FUSED_SPECTRAL_ADAM", "1" if on else "0")
    return set_


def _model(seed=11):
    torch.manual_seed(seed)
    _, P_x, _ = dfno.create_standard_partitions((1, 1, 1, 1, 1, 1))
    model = dfno.DistributedFNONd(P_x, [1, 2, 8, 8, 8, 1], 6, 8,
                                  (2, 2, 2, 2), num_blocks=2)
    return model, dfno.DistributedRelativeLpLoss(P_x)


def _data(seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(1, 2, 8, 8, 8, 1, generator=g),
            torch.rand(1, 1, 8, 8, 8, 6, generator=g))


def _corners(model):
    return [w for blk in model.blocks for w in blk.weights]


def _train(steps, backwards_per_step=1):
    model, crit = _model()
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    x, y = _data()
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        for _ in range(backwards_per_step):
            crit(model(x), y).backward()
        opt.step()
    return model, opt


def test_knob_on_equals_off(knob):
    knob(False)
    ref, _ = _train(3)
    knob(True)
    model, opt = _train(3)
    assert not opt._pending
    for (n, p), q in zip(model.named_parameters(), ref.parameters()):
        assert torch.equal(p, q), n


def test_corner_grad_is_deferred(knob):
    knob(True)
    model, crit = _model()
    opt = Adam(model.parameters(), lr=1e-3)
    x, y = _data()
    crit(model(x), y).backward()
    assert all(w.grad is None for w in _corners(model))
    assert len(opt._pending) == len(model.blocks)
    assert model.blocks[0].linear.W.grad is not None


def test_two_backwards_before_step(knob):
    knob(False)
    ref, _ = _train(2, backwards_per_step=2)
    knob(True)
    model, _ = _train(2, backwards_per_step=2)
    for (n, p), q in zip(model.named_parameters(), ref.parameters()):
        assert torch.equal(p, q), n


def test_zero_grad_drops_pending(knob):
    knob(True)
    model, crit = _model()
    opt = Adam(model.parameters(), lr=1e-3)
    x, y = _data()
    crit(model(x), y).backward()
    assert opt._pending
    before = [w.detach().clone() for w in _corners(model)]
    opt.zero_grad(set_to_none=True)
    assert not opt._pending
    opt.step()
    for w, b in zip(_corners(model), before):
        assert torch.equal(w.detach(), b)


def test_materialize_grads_matches_einsum(knob):
    from dfno_amd.ops.spectral import spectral_conv

    knob(True)
    model, _ = _model()
    blk = model.blocks[0]
    opt = Adam(model.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(3)
    F = blk.fft_shape[2:]
    x = torch.view_as_complex(torch.randn(2, 8, *F, 2, generator=g))
    gy = torch.view_as_complex(torch.randn(2, 8, *F, 2, generator=g))
    y = spectral_conv(x, list(blk.weights), blk.corner_bounds, 8)
    y.backward(gy)
    assert all(w.grad is None for w in blk.weights)
    opt.materialize_grads()
    assert not opt._pending
    for w, bounds in zip(blk.weights, blk.corner_bounds):
        sl = (slice(None), slice(None)) + tuple(slice(a, b) for a, b in bounds)
        ref = torch.einsum("bo...,bi...->io...", gy[sl], x[sl].conj())
        assert torch.allclose(w.grad, ref, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("make_opt", [None, torch.optim.Adam],
                         ids=["no-optimizer", "torch-adam"])
def test_without_fused_adam_grads_are_eager(knob, make_opt):
    knob(True)
    model, crit = _model()
    if make_opt is not None:
        make_opt(model.parameters(), lr=1e-3)
    x, y = _data()
    crit(model(x), y).backward()
    assert all(w.grad is not None for w in _corners(model))
