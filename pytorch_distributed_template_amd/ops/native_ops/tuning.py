"""The autotune names the wrappers use, and distributed pre-tuning"""
from __future__ import annotations

import os
import weakref

import torch
import torch.nn as nn

from .. import autotune

# Tile-variant autotuner: table, policy, timing and the selection protocol live in
# ``ops/autotune.py`` (``autotune.choose``); a site here gives it a key, a launch and a default.
_tuned, _tune_allowed, _capturing = autotune.tuned, autotune.tune_allowed, autotune.capturing
NOT_APPLICABLE, AX_UNFUSED = autotune.NOT_APPLICABLE, autotune.AX_UNFUSED


def pretune_distributed(run_step) -> None:
    """Agree on kernel variants across ranks before DDP training starts.

    ``run_step()`` runs one forward+backward on this rank's model (not yet
    DDP-wrapped). Rank 0 runs it with tuning enabled, then broadcasts its table;
    every rank adopts it and tuning is frozen (untuned shapes later fall back to
    the deterministic heuristic on every rank alike)."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return
    obj = [None]
    if dist.get_rank() == 0:
        err = None
        if os.environ.get("PDT_AUTOTUNE", "1") != "0" and os.environ.get("PDT_DETERMINISTIC", "0") != "1":
            # the step must leave no trace on rank 0 that the other ranks do not share:
            # RNG streams are restored (DataLoader seeds, dropout), the fp8 scaling
            # histories it created or rolled are dropped (``_snapshot_fp8_meta``)
            cpu_rng = torch.get_rng_state()
            cuda_rng = torch.cuda.get_rng_state() if torch.cuda.is_available() else None
            fp8_before = _snapshot_fp8_meta()
            try:
                with autotune.forced_tuning():
                    run_step()
                    if torch.cuda.is_available():
                        torch.cuda.synchronize()
            except Exception as e:  # tell the other ranks instead of leaving them in the broadcast
                err = f"{type(e).__name__}: {e}"
            finally:
                torch.set_rng_state(cpu_rng)
                if cuda_rng is not None:
                    torch.cuda.set_rng_state(cuda_rng)
                _restore_fp8_meta(fp8_before)
        obj = [{"error": err} if err is not None else dict(_tuned())]
    dist.broadcast_object_list(obj, src=0)
    if isinstance(obj[0], dict) and set(obj[0]) == {"error"}:
        raise RuntimeError(f"kernel pre-tuning step failed on rank 0: {obj[0]['error']}")
    autotune.adopt(obj[0])


_FP8_META_ATTRS = ("_pdt_fp8_meta", "_pdt_fp8_gmeta")


def _snapshot_fp8_meta():
    """{module: {attr: clone}} of every live fp8 delayed-scaling state (nn.Linear owners)."""
    import gc
    snap = {}
    for obj in gc.get_objects():
        if isinstance(obj, nn.Module):
            st = {a: getattr(obj, a).clone() for a in _FP8_META_ATTRS if getattr(obj, a, None) is not None}
            snap[id(obj)] = (weakref.ref(obj), st)
    return snap


def _restore_fp8_meta(snap):
    """Undo what a step did to the fp8 scaling states: states it created are removed,
    states it rolled get their previous values back."""
    import gc
    for obj in gc.get_objects():
        if not isinstance(obj, nn.Module):
            continue
        ent = snap.get(id(obj))
        before = ent[1] if ent is not None and ent[0]() is obj else {}
        for a in _FP8_META_ATTRS:
            if getattr(obj, a, None) is None:
                continue
            if a in before:
                getattr(obj, a).copy_(before[a])
            else:
                delattr(obj, a)
