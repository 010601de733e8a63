"""Multi-tensor fused SGD / Adam(W) (+AMSGrad) on MI355X.

Reference optimizer: ``torch.optim.Adam(lr=1e-3, weight_decay=0, amsgrad=True)`` (the
``optimizer`` entry of the reference project's ``config/config.json``), stepped once per batch
in its ``trainer/trainer.py``. Semantics match torch.optim exactly (tested against
it); the state_dict format is torch's (``momentum_buffer`` / ``exp_avg`` /
``exp_avg_sq`` / ``max_exp_avg_sq`` / ``step``), so checkpoints interchange
with the torch optimizers of the same name.

On GPU one HIP kernel (``csrc/optim.hip``) updates every parameter tensor:
the host builds a chunk table once per parameter set, re-uploads pointer
tables only when a tensor moved (asynchronously, from pinned memory: nothing in
``step()`` blocks the host) and each step is a single launch that also writes the
bf16 shadow copy of each parameter that the conv/GEMM kernels consume. On CPU
(gloo plumbing) the step falls back to torch's reference implementation.

``capturable=True`` (what a HIP-graph training step needs, cf. torch's capturable
Adam): the learning rate and Adam's step count live in a small device tensor per
param group that the kernels read, so a captured ``step()`` replays with the
current lr (the host rewrites it, outside the graph, in ``refresh_scalars()`` --
called by every eager ``step()`` too) and with the bias corrections of the current
step (t is incremented on the device, in the graph). ``state_dict()`` writes the
device step count back into each parameter's ``step`` so checkpoints stay torch's.
Capturable Adam keeps ONE step count per param group, so it requires every parameter of
a group to receive a gradient on every step (a captured graph assumes that anyway):
``step()`` raises if the set of parameters with gradients changes between steps --
torch's per-parameter counts would diverge from the group count there, and a checkpoint
reloaded into torch.optim would apply different bias corrections.

``max_grad_norm`` / ``skip_nonfinite`` (``_ClippedBase``): the three clip the global gradient
norm on the device -- the norm launches of the layer-wise optimizers, then the guarded step
kernels, which read the norm and the clip coefficient from device memory -- and decline a step
whose norm is inf or NaN, with no host sync, eagerly and in a captured step alike. Both off,
a step issues exactly the launches described above.

``FusedLARS`` / ``FusedLAMB`` (second half of this file, ``csrc/optim_layerwise.hip``) are the
layer-wise optimizers of the large-batch recipes, with global gradient-norm clipping on the
device; they are built on ``multi_tensor_l2norm``, a deterministic per-tensor L2 norm whose
results stay in device memory.

All five share ``_FusedBase.step()`` and what it needs (``csrc/optim_common.h`` is the kernels'
counterpart); a class adds its state, its pointer roles, its launches and its torch path.
"""
from __future__ import annotations

import os

import torch
from torch.optim import Optimizer

# elements per work-list chunk (one workgroup walks one chunk; PDT_OPT_CHUNK overrides):
# 32768 -- ResNet-50 FusedSGD step 248 us vs 289 us at 65536 (profiles/optim_chunk_round2.txt)
CHUNK = int(os.environ.get("PDT_OPT_CHUNK", "32768"))


def _ops():
    """``ops.native_ops``, imported on first use: this module must import where no kernel
    library is built."""
    from ..ops import native_ops
    return native_ops


def _call(entry, *args, what=None):
    """Call the kernel library's ``pdt_<entry>``; an error code raises (naming ``what``)."""
    ops = _ops()
    ops._chk(getattr(ops._load(), "pdt_" + entry)(*args), what or entry)


def _bump_versions(params):
    """The step kernel writes parameters through raw pointers, invisible to
    autograd's version counters: bump them so caches keyed on ``_version``
    (fp8 weight copies, saved-tensor checks) see the update."""
    from torch.autograd.graph import increment_version
    for p in params:
        increment_version(p)


def _to_device_async(host: torch.Tensor, device) -> torch.Tensor:
    """H2D copy that never blocks the host: stage through pinned memory (the
    caching host allocator keeps the pinned block alive until the copy has run)
    -- a pageable ``.to(device)`` waits for the whole queued step to drain."""
    if device.type != "cuda":
        return host.to(device)
    return host.pin_memory().to(device, non_blocking=True)


class _Plan:
    """Device-side pointer/chunk tables for one param group.

    The chunk table depends only on the parameter sizes and is built once; the
    pointer tables are re-uploaded (asynchronously) only when a tensor moved,
    e.g. after ``zero_grad(set_to_none=True)`` handed autograd fresh gradient
    buffers at new addresses."""

    def __init__(self, params, device):
        sz = _ops()._load().pdt_chunk_struct_size()
        assert sz == 24, sz
        import numpy as np
        sizes = [p.numel() for p in params]
        nch = sum((n + CHUNK - 1) // CHUNK for n in sizes)
        arr = np.zeros(nch, dtype=[("t", "<i4"), ("pad", "<i4"), ("off", "<i8"), ("len", "<i8")])
        i = 0
        for ti, n in enumerate(sizes):
            for off in range(0, n, CHUNK):
                arr[i] = (ti, 0, off, min(CHUNK, n - off))
                i += 1
        self.device = device
        self.chunks = _to_device_async(torch.from_numpy(arr.view(np.uint8).copy()), device)
        self.nchunks = nch
        self.shape_key = self._shape_key(params)
        self.tables = {}
        self.ptr_keys = {}

    @staticmethod
    def _shape_key(params):
        return tuple((id(p), p.numel()) for p in params)

    def update(self, tensors_by_role):
        for role, ts in tensors_by_role.items():
            ptrs = tuple(0 if t is None else t.data_ptr() for t in ts)
            if self.ptr_keys.get(role) != ptrs:
                self.tables[role] = _to_device_async(torch.tensor(ptrs, dtype=torch.int64), self.device)
                self.ptr_keys[role] = ptrs

    def ptr(self, role):
        t = self.tables.get(role)
        return None if t is None else t.data_ptr()


class _NormTables:
    """What the norm kernels need next to a ``_Plan``: ``chunk_begin[n + 1]`` (a tensor's
    chunks are consecutive in the chunk table), ``flags[n]`` (bit 0: layer-wise adaptation and
    weight decay apply), the per-chunk partial sums and the per-tensor norms ``[2, n]``."""

    def __init__(self, plan, params, adapt):
        import numpy as np
        n = len(params)
        begin = np.zeros(n + 1, dtype=np.int32)
        begin[1:] = np.cumsum([(p.numel() + CHUNK - 1) // CHUNK for p in params])
        assert int(begin[-1]) == plan.nchunks, (int(begin[-1]), plan.nchunks)
        dev = plan.device
        self.key = tuple(adapt)
        self.n = n
        self.chunk_begin = _to_device_async(torch.from_numpy(begin), dev)
        self.flags = _to_device_async(torch.tensor([int(a) for a in adapt], dtype=torch.int32), dev)
        self.partials = torch.zeros(2 * max(plan.nchunks, 1), dtype=torch.float32, device=dev)
        self.norms = torch.zeros((2, max(n, 1)), dtype=torch.float32, device=dev)


def _norm_tables(plan, params, adapt):
    nt = getattr(plan, "norm_tables", None)
    if nt is None or nt.key != tuple(adapt):
        nt = plan.norm_tables = _NormTables(plan, params, adapt)
    return nt


def _native_ok(params):
    return (len(params) > 0 and all(
        p.is_cuda and p.dtype == torch.float32 and (
            p.is_contiguous() or (p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last)))
        for p in params) and _ops().available())


def _dense_grads(params):
    """fp32 gradients laid out like their parameters (what the kernels index). torch refuses to
    assign a gradient of another dtype than its parameter's, but a swap of ``p.grad.data`` (or of
    ``p.data``) leaves one behind: hence the ``float()``."""
    grads = [p.grad if p.grad.dtype == torch.float32 else p.grad.float() for p in params]
    return [g if g.stride() == p.stride() else g.contiguous(memory_format=torch.channels_last
                                                             if p.dim() == 4 else torch.contiguous_format)
            for g, p in zip(grads, params)]


class _FusedBase(Optimizer):
    """What the five optimizers share: the frame of ``step()``, plans, shadows, device scalars.

    A subclass has ``_native_step(work)`` and ``_torch_step(work)``; ``work`` is a list of
    ``(group index, group, its parameters with a gradient)``. Without ``whole_step_fallback``
    every group takes the native path if it passes ``_native_ok`` and the torch path if not
    (``work`` then holds one group per call); with it, one failing group sends the whole step
    down the torch path.

    ``max_grad_norm`` / ``skip_nonfinite`` are optimizer-wide: the global gradient norm spans
    every param group (one device buffer, combined over the groups in group order), so with
    either set ``whole_step_fallback`` holds."""
    whole_step_fallback = False
    dev_width = 2  # floats of a group's device scalars

    def __init__(self, params, defaults, write_bf16_shadow=True, capturable=False, max_grad_norm=0.0,
                 skip_nonfinite=False):
        super().__init__(params, defaults)
        self.write_bf16_shadow = write_bf16_shadow
        self.capturable = bool(capturable)
        self.max_grad_norm = float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._plans = {}
        self._shadows = {}
        self._dev = {}      # group index -> device [lr, t] (capturable; Adam with skip_nonfinite)
        self._dev_lr = {}   # the lr last written into it
        self._grad_sets = {}  # device-counted Adam: group index -> ids of the params stepped first
        self._glob = None   # device [sum of squares (one double), gnorm, clip]
        self._gnorm = None  # the last step's global gradient norm (0-d; into _glob on the native path)
        self._skipped = None  # device int32 [1]: the steps skip_nonfinite declined

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._step_prologue()
        work = []
        for gi, group in enumerate(self.param_groups):
            params = [p for p in group["params"] if p.grad is not None]
            if params:
                work.append((gi, group, params))
        parts = [work] if self.whole_step_fallback else [[item] for item in work]
        for part in parts if work else []:
            if all(_native_ok(params) for _, _, params in part):
                self._native_step(part)
            else:
                self._torch_step(part)
        return loss

    def _dev_scalars(self, gi, group, device, t0=0.0):
        """The group's device ``[lr, t]`` and, up to ``dev_width``, the floats a tick kernel
        writes after them (created from the host values on first use)."""
        d = self._dev.get(gi)
        if d is None:
            d = torch.tensor([float(group["lr"]), float(t0)] + [1.0] * (self.dev_width - 2), dtype=torch.float32,
                             device=device)
            self._dev[gi] = d
            self._dev_lr[gi] = float(group["lr"])
        return d

    def _write_back_steps(self):
        """Capturable mode: set each parameter's ``step`` from its group's device step count
        (replayed graphs advance only that, and a step ``skip_nonfinite`` declined does not
        advance it), so that ``state_dict()`` stays torch's."""
        if not self._dev:
            return
        for gi, group in enumerate(self.param_groups):
            d = self._dev.get(gi)
            if d is None:
                continue
            t = float(d[1].item())
            for p in group["params"]:
                if p in self.state and "step" in self.state[p]:
                    self.state[p]["step"] = torch.tensor(t)

    def _adam_moments(self, name, work, dev_step, ok=None):
        """Adam's state for ``work``: created (``max_exp_avg_sq`` too in an ``amsgrad`` group) on a
        parameter's first step, and ``step`` advanced unless the device counts it (``dev_step``:
        the parameters with gradients must then be the same on every step). Returns this step's
        ``{group index: (bc1, bc2)}``. With ``ok`` (the torch path under ``skip_nonfinite``: a
        0-d bool tensor) ``step`` advances by it, next to the parameter, and the bias corrections
        are 0-d tensors: nothing here reads the predicate on the host."""
        bcs = {}
        for gi, group, params in work:
            if dev_step:
                key = tuple(id(p) for p in params)
                seen = self._grad_sets.setdefault(gi, key)
                if seen != key:
                    raise RuntimeError(
                        f"capturable {name}: the set of parameters with gradients changed between steps "
                        f"(group {gi}: {len(seen)} -> {len(key)} params); the group's single device step "
                        "count requires every parameter to receive a gradient on every step")
            for p in params:
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    if group.get("amsgrad"):
                        st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if ok is not None:
                    st["step"] = st["step"].to(ok.device) + ok.to(torch.float32)
                elif not dev_step:  # (capturable: the device count is the step, see _write_back_steps)
                    st["step"] += 1
            b1, b2 = group["betas"]
            step = self.state[params[0]]["step"]
            step = step if ok is not None else float(step) if not dev_step else 1.0
            bcs[gi] = (1 - b1 ** step, 1 - b2 ** step)
        return bcs

    def _finish(self, params, shadows):
        _bump_versions(params)
        if self.write_bf16_shadow:
            register_shadow = _ops().register_shadow
            for p, s in zip(params, shadows):
                register_shadow(p, s)

    @torch.no_grad()
    def sync_shadows(self):
        """Re-form every bf16 weight shadow from its fp32 parameter and register it again.

        After parameters were written outside ``step()`` (a state restore, a checkpoint load)
        the registered shadows no longer match the parameters' versions, so the next forward
        casts each weight into a NEW buffer -- and a HIP graph captured at that point records
        those casts and repeats them on every replay (53 extra cast kernels, 0.33 ms, per
        ResNet-50 replay: ``profiles/graph_vs_eager_resnet50_round6.txt``). Called before a
        capture, the captured forward reads the shadows the captured ``step()`` rewrites."""
        if not self.write_bf16_shadow:
            return
        for group in self.param_groups:
            for p in group["params"]:
                sh = self._shadows.get(id(p))
                if sh is None or sh.data_ptr() == 0 or sh.shape != p.shape:
                    continue
                sh.copy_(p.detach())
                _ops().register_shadow(p, sh)

    def mark_updated(self):
        """Tell the host that the parameters changed without a ``step()`` it ran: replays of a HIP
        graph that captured ``step()`` rewrite parameters and bf16 shadows on the device, but
        advance no version counter, so an eager forward afterwards would read weights derived at
        an older version (space-to-depth, padded, transposed and fp8 weight copies are cached per
        ``_version``). Bumps every parameter's version and registers the shadows again (they are
        current: the replays wrote them). Call it before an eager forward that follows replays."""
        for group in self.param_groups:
            params = list(group["params"])
            _bump_versions(params)
            if self.write_bf16_shadow:
                for p in params:
                    sh = self._shadows.get(id(p))
                    if sh is not None and sh.data_ptr() != 0 and sh.shape == p.shape:
                        _ops().register_shadow(p, sh)

    def refresh_scalars(self):
        """Write each group's current lr into its device scalars (capturable mode): call it
        before replaying a graph that captured ``step()`` -- an LR scheduler changes only the
        host value. A no-op for groups whose lr did not change (and without device scalars)."""
        if not self._dev:
            return
        for gi, group in enumerate(self.param_groups):
            d = self._dev.get(gi)
            if d is not None and self._dev_lr.get(gi) != float(group["lr"]):
                d[0].fill_(float(group["lr"]))
                self._dev_lr[gi] = float(group["lr"])

    def zero_grad(self, set_to_none: bool = True):
        """torch semantics; ``set_to_none=False`` (a graph-captured step must keep its gradient
        buffers) zeroes every gradient with one multi-tensor launch per device / dtype instead
        of one fill kernel per parameter (161 for ResNet-50)."""
        if set_to_none:
            return super().zero_grad(set_to_none=True)
        groups = {}
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    if p.grad.grad_fn is not None:
                        p.grad.detach_()
                    else:
                        p.grad.requires_grad_(False)
                    groups.setdefault((p.grad.device, p.grad.dtype), []).append(p.grad)
        for grads in groups.values():
            torch._foreach_zero_(grads)

    def _step_prologue(self):
        if self._dev and not torch.cuda.is_current_stream_capturing():
            self.refresh_scalars()

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._dev.clear()  # rebuilt from the loaded lr / step on the next step()
        self._dev_lr.clear()

    def _shadow(self, p):
        if not self.write_bf16_shadow:
            return None
        s = self._shadows.get(id(p))
        if s is None or s.data_ptr() == 0:
            if p.dim() == 4:
                s = torch.empty_like(p, dtype=torch.bfloat16, memory_format=torch.channels_last)
            else:
                s = torch.empty_like(p, dtype=torch.bfloat16)
            self._shadows[id(p)] = s
        return s

    def _plan(self, gi, params, roles, device):
        plan = self._plans.get(gi)
        if plan is None or plan.shape_key != _Plan._shape_key(params):
            plan = _Plan(params, device)
            self._plans[gi] = plan
        plan.update(roles)
        return plan

    @staticmethod
    def _stream():
        return torch.cuda.current_stream().cuda_stream

    # ---- the global gradient norm: clipping (max_grad_norm) and skip_nonfinite
    @staticmethod
    def _adapt(group, p):
        return False

    def _global(self, device):
        if self._glob is None or self._glob.device != device:
            self._glob = torch.zeros(4, dtype=torch.float32, device=device)
            self._glob[3] = 1.0
        self._gnorm = self._glob[2]
        return self._glob

    def _tables(self, gi, group, params, roles):
        plan = self._plan(gi, params, roles, params[0].device)
        return plan, _norm_tables(plan, params, [self._adapt(group, p) for p in params])

    def _sumsq(self, plan, nt, a, b):
        _call("sumsq_chunks", plan.chunks.data_ptr(), plan.nchunks, plan.ptr(a), plan.ptr(b) if b else None,
              nt.partials.data_ptr(), self._stream())

    def _finalize(self, nt, nroles, grole, glob, start_zero):
        _call("norm_finalize", nt.partials.data_ptr(), nt.chunk_begin.data_ptr(), nt.n, nroles, grole,
              nt.norms.data_ptr(), glob.data_ptr() if glob is not None else None, int(start_zero),
              self.max_grad_norm, self._stream())

    def _torch_norm(self, work):
        """The global gradient norm from an fp64 sum, 0-d fp64 (no host sync); kept, in fp32,
        for ``grad_norm()``."""
        sq = [p.grad.double().pow(2).sum() for _, _, params in work for p in params]
        gnorm = torch.stack([s.to(sq[0].device) for s in sq]).sum().sqrt()
        self._gnorm = gnorm.float()
        return gnorm

    def _torch_clip(self, work):
        """The clip coefficient as a 0-d fp32 tensor (no host sync), or None without clipping."""
        if self.max_grad_norm <= 0:
            return None
        return torch.clamp(self.max_grad_norm / (self._torch_norm(work) + 1e-6), max=1.0).float()

    def _torch_guard(self, work):
        """The torch path's ``(clip, ok)``: the clip coefficient as ``_torch_clip`` gives it and,
        under ``skip_nonfinite``, the 0-d bool tensor the kernels' ``gnorm <= FLT_MAX`` is (None
        without); a declined step is counted here."""
        clip = self._torch_clip(work)
        if not self.skip_nonfinite:
            return clip, None
        if clip is None:
            self._torch_norm(work)
        ok = torch.isfinite(self._gnorm)
        self._skip_counter(ok.device).add_((~ok).to(torch.int32))
        return clip, ok

    def _skip_counter(self, device):
        if self._skipped is None or self._skipped.device != device:
            self._skipped = torch.zeros(1, dtype=torch.int32, device=device)
        return self._skipped

    def _guard_args(self, glob, first_launch):
        """What a ``..._step3`` entry point takes after ``..._step2``'s arguments; the step's
        first launch alone counts a declined step."""
        count = self.skip_nonfinite and first_launch
        return (glob.data_ptr(), int(self.skip_nonfinite),
                self._skip_counter(glob.device).data_ptr() if count else None)

    def grad_norm(self):
        """The global gradient norm of the last step that took one, as a 0-d device tensor (before
        clipping; no host sync), or None if no step has."""
        return self._gnorm

    def skipped_steps(self):
        """How many steps ``skip_nonfinite`` declined, as a 0-d device int tensor (no host sync).
        Not part of ``state_dict()``."""
        if self._skipped is None:
            params = [p for group in self.param_groups for p in group["params"]]
            self._skip_counter(params[0].device)
        return self._skipped[0]


class _ClippedBase(_FusedBase):
    """Shared by FusedSGD / FusedAdam / FusedAdamW: ``max_grad_norm`` and ``skip_nonfinite``.

    With both at their defaults a step is what it is without them: one launch per param group
    (``pdt_..._step2``). With either set the step is, for every group, a sum-of-squares pass
    over its gradients and a finalize, which chain through one device buffer into the norm over
    ALL groups and ``clip = min(1, max_grad_norm / (gnorm + 1e-6))``; then, for every group, the
    step kernel's guarded instantiation (``pdt_..._step3``), which reads the two values from
    device memory, scales each gradient by ``clip`` and, under ``skip_nonfinite``, stores nothing
    when the norm is inf or NaN. No launch waits for the host and all of them are captured with
    the step; the buffers a captured step uses are created by the eager warm-up step, as the
    plans are. Under DDP the norm is computed from the averaged gradients, identical on every
    rank, with no collective.

    A non-finite norm clips to nothing useful (``inf * 0`` and ``NaN * 1`` are NaN), so only
    ``skip_nonfinite`` protects the weights: the declined step leaves parameters, state, bf16
    shadows and Adam's step count as they were and adds one to ``skipped_steps()``."""

    def __init__(self, params, defaults, write_bf16_shadow, capturable, max_grad_norm, skip_nonfinite):
        super().__init__(params, defaults, write_bf16_shadow, capturable, max_grad_norm, skip_nonfinite)
        if self.max_grad_norm < 0:
            raise ValueError(f"max_grad_norm must be >= 0 (0 disables clipping), got {max_grad_norm}")
        self._guard = self.max_grad_norm > 0 or self.skip_nonfinite
        if self._guard:  # the norm spans the groups: one that cannot run natively takes all along
            self.whole_step_fallback = True

    def _norm_launches(self, work, roles_of):
        """Per group of ``work``: its shadows, pointer roles (``roles_of(group, params, shadows)``)
        and plan; with the guard on, also its sum-of-squares and finalize launches. Returns the
        device buffer of the norm (None with the guard off) and ``(gi, group, params, shadows,
        plan, roles)`` per group -- the roles because a densified gradient is a temporary that
        must live until its step is enqueued. Every finalize has run before the first step
        launch, so that one reads the norm over all groups."""
        glob = self._global(work[0][2][0].device) if self._guard else None
        launches = []
        for k, (gi, group, params) in enumerate(work):
            shadows = [self._shadow(p) for p in params]
            roles = roles_of(group, params, shadows)
            if self._guard:
                plan, nt = self._tables(gi, group, params, roles)
                self._sumsq(plan, nt, "g", None)
                self._finalize(nt, 1, 0, glob, k == 0)
            else:
                plan = self._plan(gi, params, roles, params[0].device)
            launches.append((gi, group, params, shadows, plan, roles))
        return glob, launches

    @staticmethod
    def _keep_unless(ok, tensors, olds):
        """The torch path of a declined step: every tensor takes its old value back."""
        for t, old in zip(tensors, olds):
            t.copy_(torch.where(ok.to(t.device), t, old))


class FusedSGD(_ClippedBase):
    """torch.optim.SGD semantics (momentum, dampening, nesterov, weight_decay), and
    ``max_grad_norm`` / ``skip_nonfinite`` (``_ClippedBase``: the global gradient norm is clipped
    on the device; under DDP it is computed from the averaged gradients, identical on every rank,
    with no collective).

    The first-step flag (``buf = g``) is set on the host, which cannot know that the device
    declined a step: after a declined first step the buffer is still zero and the next step
    takes ``momentum * 0 + (1 - dampening) g``, which is ``g`` only without dampening. So
    ``skip_nonfinite`` with ``dampening != 0`` raises."""

    def __init__(self, params, lr=0.1, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False,
                 write_bf16_shadow=True, capturable=False, max_grad_norm=0.0, skip_nonfinite=False):
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                        nesterov=nesterov)
        super().__init__(params, defaults, write_bf16_shadow, capturable, max_grad_norm, skip_nonfinite)
        if self.skip_nonfinite and any(group["dampening"] != 0 for group in self.param_groups):
            raise ValueError("FusedSGD: skip_nonfinite needs dampening == 0 (after a declined first step the "
                             "zeroed momentum buffer gives (1 - dampening) g where torch takes g)")

    def _native_step(self, work):
        firsts = {}

        def roles_of(group, params, shadows):
            # ONE first-step flag for the group: a buffer created on a later step makes the
            # kernel take buf = g for every tensor of the group on that step
            first = False
            bufs = []
            for p in params:
                st = self.state[p]
                if group["momentum"] != 0:
                    if "momentum_buffer" not in st or st["momentum_buffer"] is None:
                        st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                        first = True
                    bufs.append(st["momentum_buffer"])
                else:
                    bufs.append(None)
            firsts[id(group)] = first
            return {"p": params, "g": _dense_grads(params), "b": bufs, "s": shadows}

        glob, launches = self._norm_launches(work, roles_of)
        for k, (gi, group, params, shadows, plan, _) in enumerate(launches):
            mom = group["momentum"] != 0
            dev = self._dev_scalars(gi, group, params[0].device) if self.capturable else None
            args = (plan.chunks.data_ptr(), plan.nchunks, plan.ptr("p"), plan.ptr("g"),
                    plan.ptr("b") if mom else None, plan.ptr("s") if self.write_bf16_shadow else None,
                    float(group["lr"]), float(group["momentum"]), float(group["dampening"]),
                    float(group["weight_decay"]), int(group["nesterov"]), int(firsts[id(group)]), 1.0,
                    dev.data_ptr() if dev is not None else None)
            if glob is None:
                _call("sgd_step2", *args, self._stream(), what="sgd_step")
            else:
                _call("sgd_step3", *args, *self._guard_args(glob, k == 0), self._stream(), what="sgd_step")
            self._finish(params, shadows)

    def _torch_step(self, work):
        clip, ok = self._torch_guard(work)
        for _, group, params in work:
            for p in params:
                g = p.grad if clip is None else p.grad * clip.to(p.device)
                mom = group["momentum"] != 0
                st = self.state[p] if mom else {}
                if ok is not None:  # (a buffer this step creates goes back to zero, as the kernel leaves it)
                    keep = [p, st["momentum_buffer"]] if mom and st.get("momentum_buffer") is not None else [p]
                    olds = [t.clone() for t in keep]
                if group["weight_decay"] != 0:
                    g = g.add(p, alpha=group["weight_decay"])
                if mom:
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = torch.clone(g).detach()
                        st["momentum_buffer"] = buf
                        if ok is not None:
                            keep, olds = keep + [buf], olds + [torch.zeros_like(buf)]
                    else:
                        buf.mul_(group["momentum"]).add_(g, alpha=1 - group["dampening"])
                    g = g.add(buf, alpha=group["momentum"]) if group["nesterov"] else buf
                p.add_(g, alpha=-group["lr"])
                if ok is not None:
                    self._keep_unless(ok, keep, olds)


class FusedAdam(_ClippedBase):
    """torch.optim.Adam semantics (L2 weight decay; ``amsgrad``), and ``max_grad_norm`` /
    ``skip_nonfinite`` (``_ClippedBase``: the global gradient norm is clipped on the device; under
    DDP it is computed from the averaged gradients, identical on every rank, with no collective).

    A declined step must not advance the step count, and the host cannot know of one without a
    sync: under ``skip_nonfinite`` the count lives in device memory as it does in capturable mode
    (one per param group, advanced by the guarded tick kernel; the set of parameters with
    gradients must not change between steps), and ``state_dict()`` writes it back, so a checkpoint
    holds the number of steps actually taken."""
    decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False,
                 write_bf16_shadow=True, capturable=False, max_grad_norm=0.0, skip_nonfinite=False):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad)
        super().__init__(params, defaults, write_bf16_shadow, capturable, max_grad_norm, skip_nonfinite)

    def state_dict(self):
        """torch's format (with a device step count after ``_write_back_steps()``)."""
        self._write_back_steps()
        return super().state_dict()

    def _native_step(self, work):
        dev_step = self.capturable or self.skip_nonfinite
        bcs = self._adam_moments("FusedAdam", work, dev_step)

        def roles_of(group, params, shadows):
            return {"p": params, "g": _dense_grads(params), "m": [self.state[p]["exp_avg"] for p in params],
                    "v": [self.state[p]["exp_avg_sq"] for p in params],
                    "vm": [self.state[p].get("max_exp_avg_sq") if group["amsgrad"] else None for p in params],
                    "s": shadows}

        glob, launches = self._norm_launches(work, roles_of)
        for k, (gi, group, params, shadows, plan, _) in enumerate(launches):
            b1, b2 = group["betas"]
            bc1, bc2 = bcs[gi]
            dev = self._dev_scalars(gi, group, params[0].device, t0=float(self.state[params[0]]["step"])) \
                if dev_step else None
            args = (plan.chunks.data_ptr(), plan.nchunks, plan.ptr("p"), plan.ptr("g"), plan.ptr("m"),
                    plan.ptr("v"), plan.ptr("vm") if group["amsgrad"] else None,
                    plan.ptr("s") if self.write_bf16_shadow else None, float(group["lr"]), float(b1), float(b2),
                    float(group["eps"]), float(group["weight_decay"]), int(self.decoupled), float(bc1), float(bc2),
                    1.0, dev.data_ptr() if dev is not None else None, int(dev is not None))
            if glob is None:
                _call("adam_step2", *args, self._stream(), what="adam_step")
            else:
                _call("adam_step3", *args, *self._guard_args(glob, k == 0), self._stream(), what="adam_step")
            self._finish(params, shadows)

    def _torch_step(self, work):
        clip, ok = self._torch_guard(work)
        bcs = self._adam_moments("FusedAdam", work, False, ok)
        for gi, group, params in work:
            b1, b2 = group["betas"]
            bc1, bc2 = bcs[gi]
            for p in params:
                st = self.state[p]
                g = p.grad if clip is None else p.grad * clip.to(p.device)
                if ok is not None:
                    keep = [p, st["exp_avg"], st["exp_avg_sq"]] + ([st["max_exp_avg_sq"]] if group["amsgrad"] else [])
                    olds = [t.clone() for t in keep]
                    bc1, bc2 = bc1.to(p.device), bc2.to(p.device)
                if group["weight_decay"] != 0:
                    if self.decoupled:
                        p.mul_(1 - group["lr"] * group["weight_decay"])
                    else:
                        g = g.add(p, alpha=group["weight_decay"])
                st["exp_avg"].mul_(b1).add_(g, alpha=1 - b1)
                st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
                v = st["exp_avg_sq"]
                if group["amsgrad"]:
                    torch.maximum(st["max_exp_avg_sq"], v, out=st["max_exp_avg_sq"])
                    v = st["max_exp_avg_sq"]
                denom = (v.sqrt() / (bc2 ** 0.5)).add_(group["eps"])
                if ok is None:
                    p.addcdiv_(st["exp_avg"], denom, value=-group["lr"] / bc1)
                else:  # (bc1 is a tensor, 0 on a declined first step: what that gives is discarded)
                    p.sub_(st["exp_avg"] / denom * (group["lr"] / bc1).to(p.dtype))
                    self._keep_unless(ok, keep, olds)


class FusedAdamW(FusedAdam):
    """torch.optim.AdamW semantics (decoupled weight decay); ``max_grad_norm`` and
    ``skip_nonfinite`` as in ``FusedAdam`` (under DDP the norm is computed from the averaged
    gradients, identical on every rank, with no collective)."""
    decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False,
                 write_bf16_shadow=True, capturable=False, max_grad_norm=0.0, skip_nonfinite=False):
        super().__init__(params, lr, betas, eps, weight_decay, amsgrad, write_bf16_shadow, capturable,
                         max_grad_norm, skip_nonfinite)


# =============================================================================
# Layer-wise adaptive optimizers (LARS, LAMB) with on-device gradient-norm clipping
# (csrc/optim_layerwise.hip)
# =============================================================================
def multi_tensor_l2norm(tensors):
    """Per-tensor L2 norms (float32 device tensor of ``len(tensors)``) and their global L2 norm
    (0-d device tensor) of fp32 CUDA tensors, contiguous or channels_last-dense: two launches
    for any number of tensors, deterministic (fixed-order sums, no atomics), no host sync."""
    tensors = list(tensors)
    if not tensors:
        raise ValueError("multi_tensor_l2norm: no tensors")
    dev = tensors[0].device
    for t in tensors:
        if not (t.is_cuda and t.device == dev and t.dtype == torch.float32 and (
                t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last)))):
            raise ValueError("multi_tensor_l2norm: fp32 CUDA tensors on one device, contiguous or "
                             f"channels_last-dense (got {tuple(t.shape)} {t.dtype} {t.device} strides {t.stride()})")
    plan = _Plan(tensors, dev)
    plan.update({"a": tensors})
    nt = _norm_tables(plan, tensors, [0] * len(tensors))
    glob = torch.zeros(4, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _call("sumsq_chunks", plan.chunks.data_ptr(), plan.nchunks, plan.ptr("a"), None, nt.partials.data_ptr(), st)
    _call("norm_finalize", nt.partials.data_ptr(), nt.chunk_begin.data_ptr(), nt.n, 1, 0, nt.norms.data_ptr(),
          glob.data_ptr(), 1, 0.0, st)
    return nt.norms[0, :nt.n], glob[2]


class _LayerwiseBase(_FusedBase):
    """Shared by FusedLARS / FusedLAMB: the adapt flags; the global gradient norm, the clip
    coefficient and the norm launches are ``_FusedBase``'s.

    The global norm spans every group, so the native path runs only when every group with
    gradients passes ``_native_ok``; otherwise the whole step runs ``_torch_step``."""
    whole_step_fallback = True

    def __init__(self, params, defaults, max_grad_norm, write_bf16_shadow, capturable):
        super().__init__(params, defaults, write_bf16_shadow, capturable, max_grad_norm)

    def load_state_dict(self, state_dict):
        """torch's; a checkpoint written by ``torch.optim.SGD`` / ``Adam`` has none of the
        layer-wise hyperparameters, so groups take the ones this optimizer was built with."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            for k, v in self.defaults.items():
                group.setdefault(k, v)

    def _step_prologue(self):
        if torch.cuda.is_available():  # (capturable is harmless on a machine without a GPU)
            super()._step_prologue()

    @staticmethod
    def _adapt(group, p):
        return not (group["exclude_1d"] and p.dim() <= 1)


class FusedLARS(_LayerwiseBase):
    """LARS (You et al. 2017): SGD-momentum with a layer-wise trust ratio, for large-batch
    ResNet training. With ``g' = clip g``, ``wn = |w|``, ``gn = clip |g|`` per tensor::

        adapted:   q = trust_coefficient wn / (gn + wd wn + eps)  (1 if wn or gn is 0)
                   d = q (g' + wd w)
        excluded:  d = g'                       (no weight decay, no trust ratio)
        buf = momentum buf + d   (buf = d on a tensor's first step)
        d = d + momentum buf if nesterov else buf
        w -= lr d

    ``exclude_1d`` excludes parameters with ``dim() <= 1`` (biases, BatchNorm / LayerNorm
    affine). ``max_grad_norm > 0`` clips the global gradient norm (every param group's
    gradients; ``clip = min(1, max_grad_norm / (gnorm + 1e-6))``) on the device: under DDP it
    is computed from the averaged gradients, identical on every rank, with no collective.

    Three launches per param group (sum of squares of w and g, finalize, step), none of them
    blocking the host. The state is ``momentum_buffer``: a checkpoint loads into
    ``torch.optim.SGD`` once the extra hyperparameters are dropped, and back.

    ``capturable=True``: the lr is read from device memory (``refresh_scalars()``). Momentum
    buffers are created, zeroed, by the first eager step; a captured step that would have to
    create one raises (the graph would zero the buffer again on every replay) -- capture after
    an eager warm-up step."""

    def __init__(self, params, lr, momentum=0.9, weight_decay=0.0, nesterov=False, trust_coefficient=1e-3,
                 eps=1e-8, exclude_1d=True, max_grad_norm=0.0, write_bf16_shadow=True, capturable=False):
        defaults = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov,
                        trust_coefficient=trust_coefficient, eps=eps, exclude_1d=exclude_1d)
        super().__init__(params, defaults, max_grad_norm, write_bf16_shadow, capturable)

    def _native_step(self, work):
        capturing = torch.cuda.is_current_stream_capturing()
        for _, group, params in work:
            if group["momentum"] == 0:
                continue
            for p in params:
                st = self.state[p]
                if st.get("momentum_buffer") is None:
                    if capturing:
                        raise RuntimeError(
                            "FusedLARS: this step would create a momentum buffer, which cannot happen inside "
                            "a graph capture (its zero fill would replay); run an eager step first")
                    st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        glob = self._global(work[0][2][0].device)
        launches = []
        for k, (gi, group, params) in enumerate(work):
            mom = group["momentum"] != 0
            shadows = [self._shadow(p) for p in params]
            roles = {"p": params, "g": _dense_grads(params),
                     "b": [self.state[p]["momentum_buffer"] if mom else None for p in params], "s": shadows}
            plan, nt = self._tables(gi, group, params, roles)
            self._sumsq(plan, nt, "p", "g")
            self._finalize(nt, 2, 1, glob, k == 0)
            # (roles: a densified gradient is a temporary that must live until its step is enqueued)
            launches.append((gi, group, params, shadows, plan, nt, mom, roles))
        # every group's finalize has run: glob holds the norm over all of them
        for gi, group, params, shadows, plan, nt, mom, _ in launches:
            dev = self._dev_scalars(gi, group, params[0].device) if self.capturable else None
            _call("lars_step", plan.chunks.data_ptr(), plan.nchunks, plan.ptr("p"), plan.ptr("g"),
                  plan.ptr("b") if mom else None, plan.ptr("s") if self.write_bf16_shadow else None,
                  nt.flags.data_ptr(), nt.norms.data_ptr(), nt.n, glob.data_ptr(), float(group["lr"]),
                  float(group["momentum"]), float(group["weight_decay"]), int(group["nesterov"]),
                  float(group["trust_coefficient"]), float(group["eps"]),
                  dev.data_ptr() if dev is not None else None, self._stream())
            self._finish(params, shadows)

    def _torch_step(self, work):
        clip = self._torch_clip(work)
        for _, group, params in work:
            wd, mom = group["weight_decay"], group["momentum"]
            for p in params:
                g = p.grad if clip is None else p.grad * clip.to(p.device)
                if self._adapt(group, p):
                    wn, gn = p.double().norm(), g.double().norm()
                    q = torch.where((wn > 0) & (gn > 0),
                                    group["trust_coefficient"] * wn / (gn + wd * wn + group["eps"]),
                                    torch.ones_like(wn)).to(p.dtype)
                    d = g.add(p, alpha=wd).mul_(q)
                else:
                    d = g
                if mom != 0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = st["momentum_buffer"] = torch.clone(d).detach()
                    else:
                        buf.mul_(mom).add_(d)
                    d = d.add(buf, alpha=mom) if group["nesterov"] else buf
                p.add_(d, alpha=-group["lr"])


class FusedLAMB(_LayerwiseBase):
    """LAMB (You et al. 2020): Adam moments with a layer-wise trust ratio, for large-batch
    transformer training. With ``g' = clip g``::

        m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2
        u = (m / bc1) / (sqrt(v / bc2) + eps) + wd w          (wd = 0 on excluded tensors)
        r = |w| / |u| on adapted tensors with |w| > 0 and |u| > 0, else 1
        w -= lr r u

    ``exclude_1d`` and ``max_grad_norm`` as in ``FusedLARS``. Per param group: stage 1 (moments
    and the partial sums of |u|^2, |w|^2), finalize, stage 2 (u recomputed from the moments: no
    scratch tensor) -- 3 launches, 5 with clipping (a sum-of-squares pass over g and its
    finalize first). The state is ``step`` / ``exp_avg`` / ``exp_avg_sq``: a checkpoint loads
    into ``torch.optim.Adam`` once the extra hyperparameters are dropped, and back.

    ``capturable=True`` as in ``FusedAdam``: lr and the step count live in device memory, the
    count (and the bias corrections for it) advance on the device ahead of stage 1,
    ``state_dict()`` writes the count back into ``step``, and the set of parameters with
    gradients must not change between steps."""
    dev_width = 4  # [lr, t, bc1, bc2] (bc1 / bc2 are written by the tick kernel)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, exclude_1d=True,
                 max_grad_norm=0.0, write_bf16_shadow=True, capturable=False):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, exclude_1d=exclude_1d)
        super().__init__(params, defaults, max_grad_norm, write_bf16_shadow, capturable)

    def state_dict(self):
        """torch's format (in capturable mode after ``_write_back_steps()``), as ``FusedAdam``'s."""
        self._write_back_steps()
        return super().state_dict()

    def _native_step(self, work):
        dev_step = self.capturable
        bcs = self._adam_moments("FusedLAMB", work, dev_step)
        clipping = self.max_grad_norm > 0
        glob = self._global(work[0][2][0].device) if clipping else None
        launches = []
        for k, (gi, group, params) in enumerate(work):
            shadows = [self._shadow(p) for p in params]
            roles = {"p": params, "g": _dense_grads(params), "m": [self.state[p]["exp_avg"] for p in params],
                     "v": [self.state[p]["exp_avg_sq"] for p in params], "s": shadows}
            plan, nt = self._tables(gi, group, params, roles)
            if clipping:
                self._sumsq(plan, nt, "g", None)
                self._finalize(nt, 1, 0, glob, k == 0)
            launches.append((gi, group, params, shadows, plan, nt, roles))  # (roles: as in FusedLARS)
        for gi, group, params, shadows, plan, nt, _ in launches:
            b1, b2 = group["betas"]
            bc1, bc2 = bcs[gi]
            dev = self._dev_scalars(gi, group, params[0].device, t0=float(self.state[params[0]]["step"])) \
                if dev_step else None
            devp = dev.data_ptr() if dev is not None else None
            st = self._stream()
            if dev is not None:
                _call("lamb_tick", devp, float(b1), float(b2), st)
            _call("lamb_stage1", plan.chunks.data_ptr(), plan.nchunks, plan.ptr("p"), plan.ptr("g"), plan.ptr("m"),
                  plan.ptr("v"), nt.flags.data_ptr(), nt.partials.data_ptr(),
                  glob.data_ptr() if glob is not None else None, float(b1), float(b2), float(1 - b1), float(1 - b2),
                  float(group["eps"]), float(group["weight_decay"]), float(bc1), float(bc2), devp, st)
            self._finalize(nt, 2, -1, None, False)
            _call("lamb_stage2", plan.chunks.data_ptr(), plan.nchunks, plan.ptr("p"), plan.ptr("m"), plan.ptr("v"),
                  plan.ptr("s") if self.write_bf16_shadow else None, nt.flags.data_ptr(), nt.norms.data_ptr(), nt.n,
                  float(group["lr"]), float(group["eps"]), float(group["weight_decay"]), float(bc1), float(bc2),
                  devp, st)
            self._finish(params, shadows)

    def _torch_step(self, work):
        bcs = self._adam_moments("FusedLAMB", work, False)
        clip = self._torch_clip(work)
        for gi, group, params in work:
            b1, b2 = group["betas"]
            bc1, bc2 = bcs[gi]
            for p in params:
                st = self.state[p]
                g = p.grad if clip is None else p.grad * clip.to(p.device)
                st["exp_avg"].mul_(b1).add_(g, alpha=1 - b1)
                st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
                u = (st["exp_avg"] / bc1).div_((st["exp_avg_sq"] / bc2).sqrt_().add_(group["eps"]))
                if self._adapt(group, p):
                    u.add_(p, alpha=group["weight_decay"])
                    wn, un = p.double().norm(), u.double().norm()
                    u.mul_(torch.where((wn > 0) & (un > 0), wn / un, torch.ones_like(wn)).to(p.dtype))
                p.add_(u, alpha=-group["lr"])
