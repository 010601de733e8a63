"""``ModelEMA``: an exponential moving average of a model's weights, updated after every
optimizer step (timm's ``ModelEmaV2``; the large-batch ImageNet recipes validate, checkpoint and
test the averaged weights).

    e <- e + w (p - e),   w = 1 - d
    d = min(decay, (1 + t) / (10 + t)) with ``warmup`` (t = updates done so far), else decay

Every parameter and every floating-point buffer is averaged (BatchNorm running statistics with
the same decay, as in timm); non-floating buffers (``num_batches_tracked``) are copied. The
tensors of the two models are paired by ``state_dict`` name.

On GPU one HIP launch (``csrc/ema.hip``) updates every averaged tensor: the work list is the
fused optimizers' (``optim/fused.py``: a chunk table built once, pointer tables re-uploaded only
when a tensor moved), and with ``write_bf16_shadow`` the same pass writes the bf16 copy of each
averaged parameter that the conv / GEMM kernels read, registered with ``register_shadow``, so a
validation forward on ``.module`` casts nothing. ``t``, ``d`` and ``w`` live in a small device
buffer that a tick kernel advances ahead of the update, eagerly and in a captured HIP graph
alike: a replayed graph advances the warm-up on the device and needs nothing from the host.
The tables are created by the first eager update; an update inside a graph capture that would
have to create them raises (their uploads would replay) -- capture after an eager warm-up step.
``t`` is kept as fp32 on the device, exact up to 2^24 updates.

Where a tensor is not on the GPU, not fp32, or not dense in its model's layout (the CPU / gloo
path), the update is ``torch._foreach_lerp_`` with the same decay sequence, formed on the host
in fp32 exactly as the tick kernel forms it.

Under data parallelism every rank holds identical weights after each step and the update is
deterministic (no atomics, fixed order), so the averaged weights are identical across ranks
with no collective.
"""
from __future__ import annotations

import copy

import torch

from .fused import _Plan, _bump_versions, _call, _native_ok, _ops, _to_device_async


def _unwrap(model):
    return model.module if hasattr(model, "module") and isinstance(model.module, torch.nn.Module) else model


def decay_step(t, decay, warmup):
    """One tick in numpy fp32, operation for operation what ``ema_tick_kernel`` does:
    ``(t, decay, warmup) -> (t + 1, d, w)``, all ``numpy.float32``.

    The tests keep a copy of this function (``tests/ema_ref.py:tick``) as their mirror of the
    kernel. What ties the two to the kernel rather than to each other is the GPU test that
    compares the kernel's device state with the mirror bit for bit after every update, and the
    CPU test that checks the mirror against the formula written out."""
    import numpy as np
    f = np.float32
    t = f(t)
    d = f(decay)
    if warmup:
        d = min(d, f((f(1) + t) / (f(10) + t)))
    return f(t + f(1)), f(d), f(f(1) - d)


def multi_tensor_ema_(plan, averaged, sources, shadows, dev, decay, warmup):
    """The native launch: tick ``dev = [t, d, w]``, then ``e <- e + w (p - e)`` over every tensor
    of ``averaged`` (fp32, laid out like its source; ``plan`` is their ``_Plan``), writing the bf16
    ``shadows`` (None, or a list with None entries, for none) in the same pass."""
    plan.update({"e": averaged, "p": sources, "s": shadows if shadows is not None else [None] * len(averaged)})
    _call("ema_update", plan.chunks.data_ptr(), plan.nchunks, plan.ptr("e"), plan.ptr("p"),
          plan.ptr("s") if shadows is not None else None, dev.data_ptr(), float(decay), int(bool(warmup)),
          torch.cuda.current_stream().cuda_stream)


class ModelEMA:
    """``.module`` is a second instance of the (unwrapped) model holding the averaged weights:
    ``requires_grad_(False)``, in ``eval()``. Build it before DDP wraps the model and before the
    first forward, so that no lazily attached kernel state is copied. The kernel layer's weight
    caches are keyed on the parameter object, so the second instance gets entries of its own.

    ``update(model)`` after every ``optimizer.step()``; ``state_dict()`` / ``load_state_dict()``
    for checkpoints (the averaged ``state_dict`` as plain tensors under the model's own names,
    ``num_updates``, ``decay``, ``warmup``; loading restores the weights and ``num_updates`` --
    ``decay`` and ``warmup`` stay the constructor's, as a config's do on resume).

    ``validate`` ("both" | "ema" | "model") is what a ``Trainer`` validates; ``runtime.build_ema``
    checks it and sets it from ``trainer.ema.validate``."""

    def __init__(self, model, decay=0.9999, warmup=True, write_bf16_shadow=False):
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"ModelEMA: decay must be in [0, 1], got {decay}")
        self.module = copy.deepcopy(_unwrap(model))
        self.module.requires_grad_(False)
        self.module.eval()
        self.decay = float(decay)
        self.warmup = bool(warmup)
        self.write_bf16_shadow = bool(write_bf16_shadow)
        self._t = 0          # updates done (host count: the torch path's, and what seeds ``_dev``)
        self._dev = None     # device [t, d, w]: the native path's state
        self._plan = None
        self._plan_for = None     # the list of averaged tensors the plan and the shadow list were made for
        self._shadow_list = None
        self._shadows = {}   # id(averaged parameter) -> its bf16 shadow
        self._pairs = None   # (the model paired last, averaged floats, their sources, other pairs)
        self.validate = "both"

    # ------------------------------------------------------------------ pairing
    def _paired(self, model):
        model = _unwrap(model)
        if self._pairs is not None and self._pairs[0] is model:
            return self._pairs[1:]
        mine = self.module.state_dict(keep_vars=True)
        theirs = model.state_dict(keep_vars=True)
        if list(mine) != list(theirs):
            raise ValueError("ModelEMA.update: the model's state_dict names differ from the averaged model's")
        # the lists every update walks, built once per model: the sources are the model's own
        # tensors (not detached aliases, which a ``p.data = ...`` would leave behind)
        es = [e for e in mine.values() if e.is_floating_point()]
        ps = [theirs[k] for k, e in mine.items() if e.is_floating_point()]
        other = ([e for e in mine.values() if not e.is_floating_point()],
                 [theirs[k] for k, e in mine.items() if not e.is_floating_point()])
        self._pairs = (model, es, ps, other)
        return es, ps, other

    @property
    def num_updates(self):
        """Updates done so far (read back from the device state when the native path holds it)."""
        return self._t if self._dev is None else int(round(float(self._dev[0].item())))

    # ------------------------------------------------------------------ update
    @torch.no_grad()
    def update(self, model):
        es, ps, other = self._paired(model)
        if es:
            if _native_ok(es + ps) and all(e.stride() == p.stride() and e.device == p.device
                                           for e, p in zip(es, ps)):
                self._native_update(es, ps)
            else:
                self._torch_update(es, ps)
        if other[0]:
            torch._foreach_copy_(other[0], other[1])

    def _shadow_for(self, e):
        if not self.write_bf16_shadow or not isinstance(e, torch.nn.Parameter):
            return None
        s = self._shadows.get(id(e))
        if s is None or s.data_ptr() == 0:
            # the kernel indexes a shadow like its tensor, and the conv kernels read a 4-d weight's
            # shadow as channels_last: a 4-d weight in another layout gets none (a null entry)
            if e.dim() == 4 and not e.is_contiguous(memory_format=torch.channels_last):
                return None
            s = torch.empty_like(e, dtype=torch.bfloat16, memory_format=torch.preserve_format)
            if s.stride() != e.stride():
                return None
            self._shadows[id(e)] = s
        return s

    def _native_update(self, es, ps):
        device = es[0].device
        # (``es`` is the list ``_paired`` built once: the same list means the same tensors)
        if self._plan_for is not es or self._dev is None or self._dev.device != device:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(
                    "ModelEMA: this update would create its chunk and pointer tables and its device state, "
                    "which cannot happen inside a graph capture (their uploads would replay); run an eager "
                    "update first")
            if self._plan_for is not es:
                if self._plan is None or self._plan.shape_key != _Plan._shape_key(es):
                    self._plan = _Plan(es, device)
                self._plan_for = es
                self._shadow_list = [self._shadow_for(e) for e in es] if self.write_bf16_shadow else None
            if self._dev is None or self._dev.device != device:
                self._dev = _to_device_async(
                    torch.tensor([float(self._t), self.decay, 1.0 - self.decay], dtype=torch.float32), device)
        shadows = self._shadow_list
        multi_tensor_ema_(self._plan, es, ps, shadows, self._dev, self.decay, self.warmup)
        _bump_versions(es)
        if self.write_bf16_shadow:
            register_shadow = _ops().register_shadow
            for e, s in zip(es, shadows):
                if s is not None:  # (buffers, and parameters not dense in their layout, have none)
                    register_shadow(e, s)

    def _torch_update(self, es, ps):
        if self._dev is not None:  # the native path held the count until now
            self._t = self.num_updates
            self._dev = None
        t, _, w = decay_step(self._t, self.decay, self.warmup)
        groups = {}
        for e, p in zip(es, ps):
            if p.device != e.device or p.dtype != e.dtype:
                p = p.to(device=e.device, dtype=e.dtype)
            g = groups.setdefault((e.device, e.dtype), ([], []))
            g[0].append(e)
            g[1].append(p)
        for ge, gp in groups.values():
            torch._foreach_lerp_(ge, gp, float(w))
        self._t = int(t)

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        return {"state_dict": dict(self.module.state_dict()),
                "num_updates": int(self.num_updates), "decay": self.decay, "warmup": self.warmup}

    @torch.no_grad()
    def load_state_dict(self, state):
        self.module.load_state_dict(state["state_dict"])
        self.set_num_updates(int(state.get("num_updates", 0)))
        self.sync_shadows()

    @torch.no_grad()
    def set_to(self, model, num_updates=0):
        """Start the average from ``model``'s current weights (a resume from a checkpoint that
        holds no averaged weights)."""
        self.module.load_state_dict(_unwrap(model).state_dict())
        self.set_num_updates(num_updates)
        self.sync_shadows()

    def set_num_updates(self, n):
        self._t = int(n)
        if self._dev is not None:
            self._dev[0].fill_(float(n))

    def mark_updated(self):
        """Tell the host that the averaged weights changed without an ``update()`` it ran: replays
        of a HIP graph that captured ``update()`` rewrite the averaged tensors and their shadows
        on the device but advance no version counter, so a forward on ``.module`` afterwards
        would read weights derived at an older version (the kernel layer caches space-to-depth,
        padded, transposed and fp8 weight copies per ``_version``). Bumps the version of every
        averaged floating-point tensor and registers the shadows again (they are current: the
        replays wrote them). ``Trainer`` calls it before validating ``.module`` after replays."""
        es = [e for e in self.module.state_dict(keep_vars=True).values() if e.is_floating_point()]
        _bump_versions(es)
        for e in es:
            sh = self._shadows.get(id(e))
            if sh is not None and sh.data_ptr() != 0 and sh.shape == e.shape:
                _ops().register_shadow(e, sh)

    @torch.no_grad()
    def sync_shadows(self):
        """Re-form every bf16 shadow from its averaged parameter and register it again (after the
        averaged weights were written outside ``update()``), as ``_FusedBase.sync_shadows``."""
        if not self._shadows:
            return
        for e in self.module.parameters():
            sh = self._shadows.get(id(e))
            if sh is None or sh.data_ptr() == 0 or sh.shape != e.shape:
                continue
            sh.copy_(e.detach())
            _ops().register_shadow(e, sh)
