"""The kernel library handle: where ``libpdt_hip.so`` is, the ctypes signatures read from
``csrc/pdt_api.h``, the loader and the op timer, and the helpers every wrapper uses (stream and
pointer accessors, return-code checks, gradient buffers, the fallback policy, NHWC helpers).
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
import threading
from pathlib import Path

import torch

from ..build import CSRC
from .tuning import NOT_APPLICABLE, _capturing

_LIB_PATH = Path(os.environ.get("PDT_LIB_PATH", "") or
                 Path(__file__).resolve().parents[2] / "_lib" / "libpdt_hip.so")  # override: A/B builds
_lib = None
_lock = threading.Lock()

c_int, c_long, c_float, c_double, c_void_p, c_uint = (ctypes.c_int, ctypes.c_long, ctypes.c_float,
                                                      ctypes.c_double, ctypes.c_void_p, ctypes.c_uint)

# The library's C ABI is declared once, in ``csrc/pdt_api.h`` (the compiler checks every
# definition against it); the ctypes signatures are read from that same file.
_API_HEADER = CSRC / "pdt_api.h"
_SCALARS = {"int": c_int, "long": c_long, "unsigned": c_uint, "float": c_float, "double": c_double,
            "hipStream_t": c_void_p}
_POINTEES = ("void", "float", "double", "int", "long", "int64_t")
_DECL = re.compile(r"^PDT_API\s+([^;()]*?)(\w+)\s*\(([^;()]*)\)\s*;", re.M)


def _ctype(text: str, decl: str):
    """ctypes type of a C return type or parameter written ``[const] T [*] [name]``."""
    tok = [t for t in text.replace("*", " * ").split() if t != "const"]
    pointer = tok[1:2] == ["*"]
    name = tok[2:] if pointer else tok[1:]  # nothing, or the parameter's name
    if tok and len(name) <= 1 and not set(name) & {"*", *_SCALARS, *_POINTEES}:
        if pointer and tok[0] in _POINTEES:
            return c_void_p
        if not pointer and tok[0] in _SCALARS:
            return _SCALARS[tok[0]]
    raise TypeError(f"{_API_HEADER.name}: the type in {text.strip()!r} (declaration of {decl}) is outside the "
                    "ABI's closed set")


def parse_api(text: str) -> dict:
    """``{name: (restype, [argtypes])}`` of every ``PDT_API <ret> name(<params>);`` in ``text``."""
    sigs = {}
    for ret, name, params in _DECL.findall(text):
        if name in sigs:
            raise ValueError(f"{_API_HEADER.name}: {name} is declared twice")
        sigs[name] = (_ctype(ret, name), [_ctype(p, name) for p in params.split(",")] if params.strip() else [])
    return sigs


@functools.lru_cache(maxsize=None)
def signatures() -> dict:
    """The signature table of this tree's ``csrc/pdt_api.h`` (read once per process)."""
    return parse_api(_API_HEADER.read_text())


def bind(lib, names=None):
    """Set ``restype`` / ``argtypes`` of the library's entry points (all of them, or ``names``) on
    a ``ctypes.CDLL`` from the header; an entry point the library lacks is an AttributeError."""
    sigs = signatures()
    for name in sigs if names is None else names:
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = sigs[name]
    return lib


def lib_path() -> Path:
    return _LIB_PATH


class OpTimer:
    """``PDT_OP_TIMING=1``: every launching entry point of the kernel library is bracketed
    by HIP events, and its device time attributed to (entry point, integer arguments) --
    the per-op, per-shape breakdown of a training step (scripts/op_profile.py). Query
    entry points (plans, row counts, workspace sizes) pass through untimed."""
    _QUERY = ("_rows", "_variants", "_plan", "_plan2", "_workspace", "_size", "_blocks", "_kind", "_resolve_variant",
              "_part", "_words", "_grad_row", "_set_bwd_single", "_set_tiled")

    def __init__(self, lib):
        self._lib = lib
        self.records = []
        self.enabled = False

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("pdt_") or name.endswith(self._QUERY):
            return fn
        ints = [i for i, t in enumerate(signatures().get(name, (None, []))[1]) if t in (c_int, c_long, c_uint)]

        def call(*args):
            if not self.enabled or _capturing():
                return fn(*args)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*args)
            e1.record()
            self.records.append((name, tuple(args[i] for i in ints if i < len(args)), e0, e1))
            return rc
        return call

    def summary(self, top=60):
        """[(ms, calls, name, int-args)] sorted by total time (synchronises)."""
        torch.cuda.synchronize()
        agg = {}
        for name, key, e0, e1 in self.records:
            ms = e0.elapsed_time(e1)
            ent = agg.setdefault((name, key), [0.0, 0])
            ent[0] += ms
            ent[1] += 1
        rows = sorted(((v[0], v[1], k[0], k[1]) for k, v in agg.items()), key=lambda r: -r[0])
        return rows[:top]


def _load():
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not _LIB_PATH.exists():
                raise RuntimeError(f"native kernel library missing: {_LIB_PATH} -- run "
                                   "`python -m pytorch_distributed_template_amd.ops.build`")
            lib = bind(ctypes.CDLL(str(_LIB_PATH)))
            _lib = OpTimer(lib) if os.environ.get("PDT_OP_TIMING", "0") == "1" else lib
    return _lib


def available() -> bool:
    if os.environ.get("PDT_DISABLE_NATIVE") == "1":
        return False
    return _LIB_PATH.exists() and torch.cuda.is_available()


def require():
    if not torch.cuda.is_available():
        raise RuntimeError("native HIP ops need a GPU")
    _load()


_raw_stream = torch._C._cuda_getCurrentRawStream
_cur_device = torch._C._cuda_getDevice


def _s():
    """The current HIP stream handle (the raw accessor: ~20x cheaper than
    ``torch.cuda.current_stream().cuda_stream``, which builds a Stream object per call)."""
    return _raw_stream(_cur_device())


def _p(t):
    return None if t is None else t.data_ptr()


def _chk(rc, name):
    if rc != 0:
        raise RuntimeError(f"{name} failed with code {rc}")


class NotApplicable(RuntimeError):
    """An explicitly requested kernel variant cannot run this geometry / epilogue."""


def _chk_v(rc, name):
    if rc == NOT_APPLICABLE:
        raise NotApplicable(f"{name}: variant not applicable")
    _chk(rc, name)


def multi_tensor_l2norm(tensors):
    """``(per_tensor_norms, global_norm)`` of fp32 CUDA tensors (contiguous or channels_last-dense):
    a float32 device tensor of ``len(tensors)`` and a 0-d device tensor, from two launches whatever
    the number of tensors, with fixed-order sums (bitwise repeatable) and no host sync -- e.g. to
    log a gradient norm. The kernels are the ones FusedLARS / FusedLAMB step with
    (``csrc/optim_layerwise.hip``); the work list is built by ``optim/fused.py``."""
    from ...optim.fused import multi_tensor_l2norm as impl
    return impl(tensors)


def _grad_buf(param, shape, memory_format=None, device=None):
    """fp32 output buffer for ``param``'s gradient: its slot in the data-parallel reducer's
    bucket when it has one (``parallel/reducer.py``: the kernel then writes the gradient where
    the all-reduce reads it, and autograd adopts that view as ``param.grad`` with no copy),
    else a new tensor of ``shape``."""
    if param is not None and getattr(param, "_pdt_grad_slot", None) is not None:
        from ...parallel.reducer import grad_out
        return grad_out(param, *shape, memory_format=memory_format)
    # no parameter (e.g. a bias gradient asked for without its bias tensor): the current GPU --
    # device=None would allocate on the HOST, and the kernel that fills the buffer would then
    # write through a host pointer (the illegal access of round 5's r5z variant sweep)
    dev = param.device if param is not None else device if device is not None else (
        torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None)
    if memory_format is not None:
        return torch.empty(shape, dtype=torch.float32, device=dev, memory_format=memory_format)
    return torch.empty(shape, dtype=torch.float32, device=dev)


_FALLBACK_WARNED: set = set()


def fallback(what: str, reason: str) -> None:
    """Called where a native op cannot run its input and the stock PyTorch path would.
    Under backend ``native`` that is an error -- a run that asked for the HIP kernels
    never silently measures MIOpen / SDPA instead; under ``auto`` it warns once per op."""
    from .. import fused
    if fused.get_backend() == "native":
        raise NotImplementedError(f"backend 'native': no HIP kernel path for {what} ({reason}); "
                                  "select backend 'auto' to allow the stock PyTorch op for it")
    if what not in _FALLBACK_WARNED:
        _FALLBACK_WARNED.add(what)
        import warnings
        warnings.warn(f"[pdt] {what}: {reason} -> stock PyTorch op", stacklevel=3)


def _cl(t: torch.Tensor) -> torch.Tensor:
    """channels_last-contiguous view/copy (NHWC storage)."""
    if t.dim() == 4 and not t.is_contiguous(memory_format=torch.channels_last):
        t = t.contiguous(memory_format=torch.channels_last)
    return t


def _empty_cl(n, c, h, w, dtype, device):
    return torch.empty((n, c, h, w), dtype=dtype, device=device, memory_format=torch.channels_last)
