"""Fused Adam for MI355X.

``dfno_amd.optim.Adam`` subclasses ``torch.optim.Adam`` with an identical
state layout (``step``/``exp_avg``/``exp_avg_sq``) and semantics; on GPU
fp32/complex64 parameters the update runs as one fused HIP kernel per
parameter over flat real views (complex Adam is elementwise-identical on
the real view), ~3x less optimizer overhead than the foreach path at the
flagship config.  Any other parameter falls back to the stock step.

Spectral corner weights (tagged by ``DistributedFNOBlock``, complex64) are
registered with the optimizer that owns them.  Their backward then leaves a
pending ``(x, gy)`` entry here instead of a gradient tensor, and ``step()``
runs one kernel per entry that rebuilds the gradient in registers and applies
the update (ops/spectral.py, "Deferred grad-W").  ``.grad`` of those weights
stays ``None``; ``materialize_grads()`` writes the gradients out on request,
``zero_grad()`` drops the pending entries, and ``DFNO_FUSED_SPECTRAL_ADAM=0``
turns the deferral off.
"""

from __future__ import annotations

import torch

from . import _ext
from .ops import spectral as _spectral

__all__ = ["Adam"]


class Adam(torch.optim.Adam):
    """Flat views of (p, exp_avg, exp_avg_sq) are cached OUTSIDE self.state
    (keyed by id(p)) so state_dict()/load_state_dict() never serialize them;
    a cached view is rebuilt whenever any underlying storage pointer changed
    (e.g. after load_state_dict replaced the moment buffers)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._flat_cache = {}  # id(p) -> (ptrs, (pv, mv, vv))
        # deferred spectral grad-W: (x, gy, bounds_list, weights) per call
        self._pending = []
        for group in self.param_groups:
            _spectral.register_corners(self, group["params"])

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "_pending"):   # not during __init__
            _spectral.register_corners(self, self.param_groups[-1]["params"])

    # ---- deferred spectral grad-W ----------------------------------------
    def _group_of(self, p):
        for group in self.param_groups:
            if any(q is p for q in group["params"]):
                return group
        return None

    def accepts_deferred(self, weights) -> bool:
        """Whether ``step()`` can take these corner weights without a
        gradient tensor: one plain (not amsgrad, not maximize) group."""
        group = self._group_of(weights[0])
        return (group is not None
                and not group.get("amsgrad", False)
                and not group.get("maximize", False)
                and all(any(q is w for q in group["params"]) for w in weights))

    def has_pending(self, weights) -> bool:
        ids = {id(w) for w in weights}
        return any(id(w) in ids for ent in self._pending for w in ent[3])

    def add_pending(self, x, gy, bounds_list, weights) -> None:
        self._pending.append((x, gy, bounds_list, tuple(weights)))

    @torch.no_grad()
    def materialize_grads(self) -> None:
        """Write every pending corner gradient into ``.grad`` (accumulating
        onto an existing one) and clear the pending entries."""
        pending, self._pending = self._pending, []
        for x, gy, bounds_list, weights in pending:
            for w, gw in zip(weights, _spectral.corner_grads(
                    x, gy, bounds_list, weights)):
                if w.grad is None:
                    w.grad = gw
                else:
                    w.grad += gw

    def zero_grad(self, set_to_none: bool = True):
        self._pending = []
        return super().zero_grad(set_to_none=set_to_none)

    def _step_pending(self, ext) -> None:
        """One fused grad-W + Adam launch per pending entry."""
        pending, self._pending = self._pending, []
        for ent in pending:
            x, gy, bounds_list, weights = ent
            group = self._group_of(weights[0])
            if (not x.is_cuda or x.numel() == 0
                    or any(w.grad is not None or not w.is_contiguous()
                           for w in weights)):
                self._pending = [ent]
                self.materialize_grads()
                continue
            ms, vs, steps = [], [], []
            for w in weights:
                state = self.state[w]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0)
                    state["exp_avg"] = torch.zeros_like(w)
                    state["exp_avg_sq"] = torch.zeros_like(w)
                state["step"] += 1
                ms.append(state["exp_avg"])
                vs.append(state["exp_avg_sq"])
                steps.append(int(state["step"].item()))
            beta1, beta2 = group["betas"]
            for i in range(0, len(weights), 8):
                ext.spectral_gradw_adam_(
                    x, gy, [w.detach() for w in weights[i:i + 8]],
                    ms[i:i + 8], vs[i:i + 8],
                    [[a for a, _ in b] for b in bounds_list[i:i + 8]],
                    group["lr"], beta1, beta2, group["eps"],
                    group["weight_decay"], steps[i:i + 8])

    def _flat_views(self, p, state):
        def flat(t):
            r = torch.view_as_real(t) if t.is_complex() else t
            assert r.is_contiguous(), "fused Adam requires contiguous params"
            return r.view(-1)
        ptrs = (p.data_ptr(), state["exp_avg"].data_ptr(),
                state["exp_avg_sq"].data_ptr())
        cached = self._flat_cache.get(id(p))
        if cached is None or cached[0] != ptrs:
            cached = (ptrs, (flat(p), flat(state["exp_avg"]),
                             flat(state["exp_avg_sq"])))
            self._flat_cache[id(p)] = cached
        return cached[1]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()

        ext = _ext.get(required=False) if torch.cuda.is_available() else None
        if self._pending:
            if ext is None:
                self.materialize_grads()   # CPU: the stock path below
            else:
                self._step_pending(ext)
        fallback_groups = []
        for group in self.param_groups:
            lr = group["lr"]
            beta1, beta2 = group["betas"]
            eps = group["eps"]
            wd = group["weight_decay"]
            if group.get("amsgrad", False) or ext is None:
                fallback_groups.append(group)
                continue
            slow = []
            batch = ([], [], [], [], [])  # p, g, m, v, step
            fp8_q, fp8_in, fp8_out, origs = [], [], [], []
            try:
                from .ops.spectral import _FP8_CACHE, _QUANT_EPOCH
            except Exception:
                _FP8_CACHE, _QUANT_EPOCH = {}, [0]
            empty = None
            for p in group["params"]:
                if p.grad is None or p.numel() == 0:
                    continue
                if not (p.is_cuda and p.dtype in (torch.float32, torch.complex64,
                                                  torch.float64, torch.complex128,
                                                  torch.bfloat16)
                        and not p.grad.is_sparse and p.is_contiguous()):
                    slow.append(p)
                    continue
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0)
                    state["exp_avg"] = torch.zeros_like(p)
                    state["exp_avg_sq"] = torch.zeros_like(p)
                state.pop("_flat_pmv", None)  # stale entry from old checkpoints
                state["step"] += 1
                pv, mv, vv = self._flat_views(p, state)
                gv = torch.view_as_real(p.grad) if p.grad.is_complex() else p.grad
                batch[0].append(pv)
                batch[1].append(gv.reshape(-1).contiguous())
                batch[2].append(mv)
                batch[3].append(vv)
                batch[4].append(int(state["step"].item()))
                # fp8 quantize-in-Adam (delayed scaling): spectral corner
                # masters with a live e4m3 cache get their quantized copy
                # refreshed by the update kernel itself — the per-step
                # requantization pass disappears (docs/ROADMAP.md item 5)
                origs.append(p)
                ent = _FP8_CACHE.get(id(p)) if p.dtype == torch.complex64 else None
                if ent is not None and (ent[1].shape != p.shape
                                        or ent[1].device != p.device):
                    ent = None   # id() reuse after a freed master
                if ent is not None:
                    if len(ent) == 3:   # bootstrap the measured-amax slot
                        ent.append(ent[2].clone())
                    ent[2].zero_()      # receives the NEW measured amax
                    fp8_q.append(ent[1].view(torch.uint8))
                    fp8_in.append(ent[3])   # delayed scale (prev measurement)
                    fp8_out.append(ent[2])
                else:
                    if empty is None:
                        empty = torch.empty(0, device=p.device)
                    fp8_q.append(empty)
                    fp8_in.append(empty)
                    fp8_out.append(empty)
            if batch[0] and any(q.numel() for q in fp8_q):
                quantized = ext.adam_step_batch_fp8_(
                    batch[0], batch[1], batch[2], batch[3], lr, beta1, beta2,
                    eps, wd, batch[4], fp8_q, fp8_in, fp8_out)
                for idx in quantized:
                    ent = _FP8_CACHE[id(origs[idx])]
                    # the copy was quantized with ent[3]'s scale; make that
                    # the dequant scale and keep the fresh measurement as
                    # the next delayed scale
                    ent[2], ent[3] = ent[3], ent[2]
                    ent[0] = _QUANT_EPOCH[0] + 1   # fresh for the next fwd
            elif batch[0]:
                ext.adam_step_batch_(batch[0], batch[1], batch[2], batch[3],
                                     lr, beta1, beta2, eps, wd, batch[4])
            if slow:
                fallback_groups.append({**group, "params": slow})

        if fallback_groups:
            saved = self.param_groups
            try:
                self.param_groups = fallback_groups
                super().step()
            finally:
                self.param_groups = saved
        return loss
