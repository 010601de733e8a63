"""Concrete Trainer: the training hot loop and distributed validation.

Reference: ``/root/reference/trainer/trainer.py:11-123``.

Same semantics: per batch ``zero_grad -> forward -> criterion -> backward ->
step``; epoch log ``{'loss', 'val_loss', 'val_<metric>'...}``; per-epoch
LR-scheduler step; iteration-based epochs via ``len_epoch`` + ``inf_loop``;
DEBUG progress line ``'Train Epoch: {} {} Loss: {:.6f}'`` every
``int(sqrt(batch_size))`` iterations; validation predictions gathered to rank 0
and scored there.

MI355X-first changes to the hot loop:
  * the loss is accumulated ON DEVICE; the cross-rank mean is taken once per
    epoch (and at DEBUG log points) instead of a ``dist.reduce`` + ``.item()``
    host sync every iteration. mean_iters(mean_ranks) == mean_ranks(mean_iters),
    so the logged epoch loss is unchanged;
  * input batches are moved with ``non_blocking=True`` (device-resident
    synthetic loaders make this a no-op);
  * image-grid logging is opt-in (``trainer.log_images``);
  * ``len_epoch`` is honoured exactly (the reference ran ``len_epoch+1`` steps);
  * validation computes a real ``val_loss`` (the reference's was always 0 -- Q1)
    and gathers *unpadded* per-rank predictions as fixed-shape tensors;
  * throughput (images/sec, whole job) is measured per epoch with device syncs;
  * ``trainer.hip_graph``: after ``GRAPH_WARMUP`` eager steps (DDP samples its runtime
    stats over the first 10 iterations) the whole step -- zero_grad, forward, loss,
    backward with DDP's RCCL all-reduces, the fused optimizer -- is captured once as a
    HIP graph and replayed for every later full-size batch (copied into the graph's
    static input buffers -- the images and the target, which is the labels or, for a mixed
    batch, the three tensors of a ``MixedTarget``); the optimizer is capturable, so replays use the scheduler's
    current lr and Adam's current step. Partial batches and validation run eagerly;
  * ``trainer.ema`` (``{decay, warmup, validate}``, ``optim.ModelEMA`` built by
    ``runtime.build_ema``): the weight average is updated right after ``optimizer.step()``, in
    the eager loop and in the captured step alike (one more launch in the graph; the warm-up
    steps build its tables). ``validate``: ``"both"`` (default) reports ``val_*`` for the trained
    weights and ``val_ema_*`` for the averaged ones, ``"ema"`` / ``"model"`` only one of them;
    ``monitor`` may name ``val_ema_<metric>``. Absent or null, nothing changes;
  * ``trainer.log_grad_norm`` (default false; needs an optimizer with ``grad_norm()``, i.e.
    ``optim.Fused*`` with ``max_grad_norm`` or ``skip_nonfinite``): the global gradient norm of
    every step, eager or replayed, is accumulated on the device the way the loss is -- no
    per-iteration sync -- and the epoch log gets ``grad_norm`` (the mean of the finite norms,
    before clipping) and, where the optimizer counts them, ``skipped_steps`` (the steps
    ``skip_nonfinite`` declined in the epoch);
  * ``trainer.lr_step``: ``"epoch"`` (default, the reference's) or ``"iteration"`` -- the
    scheduler steps after every optimizer step, graph replays included (the host value; a
    capturable optimizer's ``refresh_scalars()`` carries it to the device before each replay);
  * ``trainer.eval_mode``: ``"gather"`` (default: the validation described above) or ``"stream"``
    (``trainer/streaming.py``): every batch's logits are scored on the device in one pass
    (``csrc/eval_stats.hip``) that adds the loss sum and the top-k correct counts into a few device
    scalars; a validation pass ends with one small all-reduce, keeps no logits, gathers nothing
    and never waits for a batch. Needs a loss and metrics with a row-wise form
    (``models.loss.EVAL_FORMS``, ``models.metric.COUNT_FORMS``); the log keys are the same.
"""
from __future__ import annotations

import math
import time

import torch

from ..base.base_trainer import BaseTrainer
from ..utils import MetricTracker, inf_loop
from ..utils import dist as pdist
from ..utils.profiling import PhaseTimer
from .streaming import StreamingEval, eval_mode


GRAPH_WARMUP = 11  # eager steps before the capture (DDP's runtime statistics cover iterations 1..10)


def _map_target(fn, target):
    """``fn`` over a target: one tensor (labels), or a tuple of tensors (a mixed batch's
    ``MixedTarget``), which keeps its type."""
    if torch.is_tensor(target):
        return fn(target)
    vals = [fn(t) for t in target]
    return type(target)(*vals) if hasattr(target, "_fields") else type(target)(vals)


def _target_shapes(target):
    return [target.shape] if torch.is_tensor(target) else [t.shape for t in target]


class _LossCurve:
    """The per-iteration ``loss/train`` scalar of the reference (``trainer.py:60-62`` ->
    ``MetricTracker.update`` -> ``writer.add_scalar``) without its per-iteration host sync:
    every ``log_step`` iterations the rank-mean loss is copied device -> pinned host
    (non-blocking, behind the step's kernels) and written once that copy has landed --
    checked at the next log point, flushed at the end of the epoch. On CPU it is written
    at once (no device to wait for)."""

    def __init__(self, writer, device, enabled):
        self.writer = writer
        self.device = device
        self.enabled = bool(enabled)  # the same on every rank (it gates a collective)
        self._pending = []  # (global step, pinned host scalar, event)

    def push(self, step, loss):
        if not self.enabled:
            return
        mean = pdist.all_reduce_mean(loss.detach().float().reshape(1))  # collective: every rank
        if not pdist.is_main_process() or getattr(self.writer, "writer", None) is None:
            return
        if self.device.type != "cuda":
            self._write(step, float(mean.item()))
            return
        host = torch.empty(1, dtype=torch.float32, pin_memory=True)
        host.copy_(mean, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._pending.append((step, host, ev))
        self.drain(block=False)

    def drain(self, block=False):
        while self._pending:
            step, host, ev = self._pending[0]
            if not block and not ev.query():
                return
            ev.synchronize()
            self._write(step, float(host[0]))
            self._pending.pop(0)

    def _write(self, step, value):
        w = self.writer
        saved = (w.step, w.mode)
        w.step, w.mode = step, "train"
        w.add_scalar("loss", value)
        w.step, w.mode = saved



class Trainer(BaseTrainer):
    def __init__(self, model, criterion, metric_ftns, optimizer, config, device,
                 data_loader, valid_data_loader=None, lr_scheduler=None, len_epoch=None,
                 autocast_dtype=None, channels_last=False, ema=None):
        super().__init__(model, criterion, metric_ftns, optimizer, config, lr_scheduler=lr_scheduler, ema=ema)
        self.device = device
        self.data_loader = data_loader
        self._base_loader = data_loader
        if len_epoch is None:
            self.len_epoch = len(self.data_loader)
        else:
            self.data_loader = inf_loop(data_loader)
            self.len_epoch = len_epoch
        self.valid_data_loader = valid_data_loader
        self.do_validation = self.valid_data_loader is not None
        self.log_step = max(1, int(math.sqrt(data_loader.batch_size)))
        self.log_images = bool(config["trainer"].get("log_images", False))
        self.autocast_dtype = autocast_dtype
        self.channels_last = channels_last

        self.train_metrics = MetricTracker("loss", writer=self.writer)
        self.loss_curve = _LossCurve(self.writer, device, config["trainer"].get("tensorboard", False))
        self.valid_metrics = MetricTracker("loss", *[m.__name__ for m in self.metric_ftns], writer=self.writer)
        self.valid_ema_metrics = None
        self.ema_validate = "model"
        if self.ema is not None:
            self.ema_validate = getattr(self.ema, "validate", "both")  # (checked by runtime.build_ema)
            self.valid_ema_metrics = MetricTracker("ema_loss", *["ema_" + m.__name__ for m in self.metric_ftns],
                                                   writer=self.writer)
        # "gather": logits of the whole set to rank 0; "stream": device accumulators (one per tracker)
        self.eval_mode = eval_mode(config)
        self._stream_evals = {}
        if self.eval_mode == "stream":
            self._stream_evals[""] = StreamingEval(criterion, self.metric_ftns, device)
            if self.ema is not None:
                self._stream_evals["ema_"] = StreamingEval(criterion, self.metric_ftns, device)
        self.lr_step = config["trainer"].get("lr_step", "epoch")
        if self.lr_step not in ("epoch", "iteration"):
            raise ValueError(f'trainer.lr_step must be "epoch" or "iteration", got {self.lr_step!r}')
        # the optimizer's global gradient norm in the epoch log (trainer.log_grad_norm)
        self.log_grad_norm = bool(config["trainer"].get("log_grad_norm", False)) and hasattr(optimizer, "grad_norm")
        self.last_throughput = None
        # optional per-phase device timing (HIP events + ROCTx ranges): trainer.profile_phases
        self.phase_timer = PhaseTimer(enabled=bool(config["trainer"].get("profile_phases", False))
                                      and device.type == "cuda")
        # HIP-graph step (trainer.hip_graph): needs a capturable fused optimizer
        self.hip_graph = bool(config["trainer"].get("hip_graph", False)) and device.type == "cuda"
        if self.hip_graph and not getattr(optimizer, "capturable", False):
            self.logger.warning("trainer.hip_graph needs a capturable fused optimizer (optim.Fused*, "
                                "trainer.fused_optimizer); training eagerly")
            self.hip_graph = False
        self._graph = None
        self._graph_io = None  # (static data, static target, static loss)
        self._graph_eager_steps = 0
        # whose weights graph replays have rewritten since their last eager forward (see _valid_epoch)
        self._replayed = {"model": False, "ema": False}
        # the capture side stream: the one DDP was built on (runtime.builder.wrap_model), if any
        self._side = (getattr(model, "_pdt_capture_stream", None) or torch.cuda.Stream(device=device)) \
            if self.hip_graph else None

    # ------------------------------------------------------------------ helpers
    def _on_epoch_start(self, epoch):
        for loader in (self._base_loader, self.valid_data_loader):
            if loader is not None and hasattr(loader, "set_epoch"):
                loader.set_epoch(epoch)

    def _to_device(self, data, target):
        data = data.to(self.device, non_blocking=True)
        # a loader's NHWC-padded batch (``pdt_nhwc_pad``) is already in the layout the
        # native stem reads in place: re-laying it out would copy it and drop the tag
        if self.channels_last and data.dim() == 4 and getattr(data, "pdt_nhwc_pad", None) is None:
            data = data.contiguous(memory_format=torch.channels_last)
        return data, _map_target(lambda t: t.to(self.device, non_blocking=True), target)

    def _autocast(self):
        if self.autocast_dtype is None:
            return torch.autocast(device_type=self.device.type, enabled=False)
        return torch.autocast(device_type=self.device.type, dtype=self.autocast_dtype)

    def _sync(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------ train
    def _train_epoch(self, epoch):
        self.model.train()
        self.train_metrics.reset()
        loss_sum = torch.zeros((), dtype=torch.float32, device=self.device)
        if self.log_grad_norm:
            gnorm_sum = torch.zeros((), dtype=torch.float32, device=self.device)
            gnorm_n = torch.zeros((), dtype=torch.float32, device=self.device)
            skipped = getattr(self.optimizer, "skipped_steps", None)
            skipped_at_start = skipped().clone() if skipped is not None else None
        n_iter = 0
        n_images = 0
        warm = min(2, max(0, self.len_epoch - 1))
        t_start = None

        for batch_idx, (data, target) in enumerate(self.data_loader):
            if batch_idx == warm:
                self._sync()
                t_start = time.perf_counter()
                n_images = 0
            data, target = self._to_device(data, target)

            if self.hip_graph:
                loss = self._graph_step(data, target)
            else:
                pt = self.phase_timer
                self.optimizer.zero_grad(set_to_none=True)
                with pt.phase("forward"), self._autocast():
                    output = self.model(data)
                    loss = self.criterion(output, target)
                with pt.phase("backward"):
                    loss.backward()
                with pt.phase("optimizer"):
                    self.optimizer.step()
                if self.ema is not None:
                    with pt.phase("ema"):
                        self.ema.update(self.model)
            if self.lr_scheduler is not None and self.lr_step == "iteration":
                self.lr_scheduler.step()

            loss_sum += loss.detach().float()
            if self.log_grad_norm:
                # (a replay rewrites the norm in place: read it behind the step, like the loss)
                gnorm = self.optimizer.grad_norm()
                if gnorm is not None:
                    finite = torch.isfinite(gnorm)
                    gnorm_sum += torch.where(finite, gnorm, torch.zeros_like(gnorm)).to(self.device)
                    gnorm_n += finite.to(self.device)
            n_iter += 1
            n_images += data.shape[0]

            gstep = (epoch - 1) * self.len_epoch + batch_idx
            if pdist.is_main_process():
                self.writer.set_step(gstep)
            if batch_idx % self.log_step == 0:
                self.loss_curve.push(gstep, loss)
            if batch_idx % self.log_step == 0 and self.logger.isEnabledFor(10):  # DEBUG
                loss_reduced = self.reduce_loss(loss)
                if pdist.is_main_process():
                    self.logger.debug("Train Epoch: {} {} Loss: {:.6f}".format(
                        epoch, self._progress(batch_idx + 1), loss_reduced.item()))
                    if self.log_images:
                        from ..utils.image import make_grid
                        self.writer.add_image("input", make_grid(data.detach().float().cpu(), nrow=8,
                                                                 normalize=True))

            if batch_idx + 1 >= self.len_epoch:
                break

        self._sync()
        if t_start is not None and n_iter > warm:
            dt = time.perf_counter() - t_start
            self.last_throughput = n_images * pdist.get_world_size() / max(dt, 1e-9)

        self.loss_curve.drain(block=True)
        if self.device.type == "cuda":
            from ..ops.native_ops import check_targets_pending
            check_targets_pending()  # the epoch's last NLL target checks (native loss)
        mean_loss = pdist.all_reduce_mean(loss_sum / max(n_iter, 1))
        # the TB curve got its per-log-step points above: the epoch mean is not written again
        self.train_metrics.update("loss", mean_loss.item(), n=1, write=False)
        log = self.train_metrics.result()
        if self.log_grad_norm:
            # the norm is taken from the averaged gradients: the same on every rank
            log["grad_norm"] = (gnorm_sum / gnorm_n).item() if gnorm_n.item() > 0 else float("nan")
            if skipped_at_start is not None:
                log["skipped_steps"] = int((self.optimizer.skipped_steps() - skipped_at_start).item())
        if self.last_throughput is not None:
            log["images_per_sec"] = round(self.last_throughput, 2)
        if self.phase_timer.enabled:
            log.update({f"ms_{k}": round(v, 3) for k, v in self.phase_timer.summary().items()})

        if self.do_validation:
            if self.ema_validate != "ema":
                val_log = self._valid_epoch(epoch)
                if pdist.is_main_process():
                    log.update(**{"val_" + k: v for k, v in val_log.items()})
            if self.ema is not None and self.ema_validate != "model":
                val_log = self._valid_epoch(epoch, model=self.ema.module, prefix="ema_")
                if pdist.is_main_process():
                    log.update(**{"val_" + k: v for k, v in val_log.items()})

        if self.lr_scheduler is not None and self.lr_step == "epoch":
            self.lr_scheduler.step()
        return log

    # ------------------------------------------------------------------ HIP graph
    def _step_body(self, data, target):
        # the captured kernels must write fixed addresses: under the framework's reducer every
        # gradient lives in a fixed bucket slot anyway, so the gradients are dropped and the
        # native kernels write the slots directly (no zero fill, no accumulate add); otherwise
        # they stay allocated (set_to_none=False) and are zeroed in place
        self.optimizer.zero_grad(set_to_none=bool(getattr(self.model, "static_grad_slots", False)))
        with self._autocast():
            output = self.model(data)
            loss = self.criterion(output, target)
        loss.backward()
        self.optimizer.step()
        if self.ema is not None:
            self.ema.update(self.model)
        return loss

    def _graph_step(self, data, target):
        """One training step in ``trainer.hip_graph`` mode: eager (on the capture side
        stream) during the warm-up and for batches whose shape differs from the captured
        one; the capture right after the warm-up (it records the step without running it:
        the batch is then replayed like every later one); a replay otherwise."""
        cur = torch.cuda.current_stream(self.device)
        side = self._side
        # capture only a FULL batch (the loader's batch_size): a partial last batch captured
        # here would fix the graph to the short shape and every later full batch would run
        # eagerly; a partial batch arriving after the warm-up runs eagerly and the capture
        # waits for the next full one
        full = data.shape[0] == getattr(self._base_loader, "batch_size", data.shape[0])
        if self._graph is None and self._graph_eager_steps >= GRAPH_WARMUP and full:
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                self._capture(data, target)
            cur.wait_stream(side)
        io = self._graph_io
        if self._graph is not None and io[0].shape == data.shape \
                and type(io[1]) is type(target) and _target_shapes(io[1]) == _target_shapes(target):
            io[0].copy_(data)
            if torch.is_tensor(target):
                io[1].copy_(target)
            else:  # a mixed batch: every target tensor is a static graph input
                for static, t in zip(io[1], target):
                    static.copy_(t)
            self.optimizer.refresh_scalars()  # the scheduler's lr (written outside the graph)
            self._graph.replay()
            self._replayed["model"] = self._replayed["ema"] = True
            return io[2]
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            loss = self._step_body(data, target)
        cur.wait_stream(side)
        self._graph_eager_steps += 1
        return loss

    def _capture(self, data, target):
        from ..ops.native_ops import nhwc_padded_view
        gx = data.clone()
        if getattr(data, "pdt_nhwc_pad", None):  # keep the padded-NHWC view the native stem reads in place
            cp = data.pdt_nhwc_pad
            buf = nhwc_padded_view(data, cp).clone(memory_format=torch.channels_last)
            gx = buf[:, :data.shape[1]]
            gx.pdt_nhwc_pad = cp
        gy = _map_target(torch.clone, target)
        self.optimizer.refresh_scalars()
        # the eager warm-up's cached activation blocks go back first (the graph gets a private
        # pool: both reserved at once would double the activation memory)
        torch.cuda.synchronize(self.device)
        torch.cuda.empty_cache()
        pdist.quiesce_for_capture(self.device)  # the RCCL watchdog retires the warm-up's collectives first
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self._side):
            gloss = self._step_body(gx, gy)
        self._graph, self._graph_io = graph, (gx, gy, gloss)
        self.logger.info("captured the training step as a HIP graph after {} eager steps".format(
            self._graph_eager_steps))

    # ------------------------------------------------------------------ validate
    @torch.no_grad()
    def _valid_epoch(self, epoch, model=None, prefix=""):
        """Validate ``model`` (default: the trained one); the averaged weights' pass (``prefix``
        ``"ema_"``) keeps its own tracker, so its keys are ``ema_loss`` / ``ema_<metric>``."""
        model = self.model if model is None else model
        tracker = self.valid_metrics if not prefix else self.valid_ema_metrics
        # graph replays rewrite weights (and their bf16 shadows) on the device without a host-side
        # version bump: without one this eager forward would read the weight copies the kernel
        # layer cached per version at the previous validation (stem, padded, fp8, transposed)
        who = "model" if model is self.model else "ema" if self.ema is not None and model is self.ema.module else None
        if who is not None and self._replayed[who]:
            owner = self.optimizer if who == "model" else self.ema
            if hasattr(owner, "mark_updated"):
                owner.mark_updated()
            self._replayed[who] = False
        model.eval()
        tracker.reset()
        if self.eval_mode == "stream":
            acc = self._stream_evals[prefix]
            acc.reset()
            for data, target in self.valid_data_loader:
                data, target = self._to_device(data, target)
                with self._autocast():
                    output = model(data)
                acc.update(output, target)
            scores = acc.result(prefix)  # (one all-reduce: every rank)
            result = {}
            if pdist.is_main_process():
                for key, value in scores.items():
                    tracker.update(key, value)
                result = tracker.result()
            if model is self.model:
                model.train()
            return result
        outputs, targets = [], []
        loss_sum = torch.zeros((), dtype=torch.float64, device=self.device)
        n = 0
        for data, target in self.valid_data_loader:
            data, target = self._to_device(data, target)
            with self._autocast():
                output = model(data)
                loss = self.criterion(output, target)
            loss_sum += loss.double() * data.shape[0]
            n += data.shape[0]
            outputs.append(output.float())
            targets.append(target)

        C = outputs[0].shape[1] if outputs else 1
        out = torch.cat(outputs) if outputs else torch.zeros((0, C), device=self.device)
        tgt = torch.cat(targets) if targets else torch.zeros((0,), dtype=torch.long, device=self.device)
        stats = torch.stack([loss_sum, torch.tensor(float(n), dtype=torch.float64, device=self.device)])
        if pdist.get_world_size() > 1:
            torch.distributed.all_reduce(stats)

        out_all = self._accumulate_predictions_from_multiple_gpus(out)
        tgt_all = self._accumulate_predictions_from_multiple_gpus(tgt)
        result = {}
        if pdist.is_main_process():
            out_all = torch.cat(out_all)
            tgt_all = torch.cat(tgt_all)
            tracker.update(prefix + "loss", float(stats[0] / max(stats[1], 1)))
            for met in self.metric_ftns:
                tracker.update(prefix + met.__name__, met(out_all, tgt_all))
            result = tracker.result()
        if model is self.model:
            model.train()
        return result

    def _progress(self, batch_idx):
        base = "[{}/{} ({:.0f}%)]"
        if hasattr(self._base_loader, "n_samples"):
            current = batch_idx * self._base_loader.batch_size
            total = self._base_loader.n_samples
        else:
            current = batch_idx
            total = self.len_epoch
        return base.format(current, total, 100.0 * current / max(total, 1))
