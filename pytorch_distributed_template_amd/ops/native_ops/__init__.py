"""ctypes bindings to ``libpdt_hip.so`` and the autograd Functions built on them.

Every op checks shapes / dtypes / memory formats on the host before a kernel
is launched (a mis-shaped launch on MI355X can fault the whole node) and
raises loudly if the library is missing on a GPU run -- there is no silent
fallback inside this package. ``ops/fused.py`` decides native vs torch.

Tensor conventions: activations are bf16 ``channels_last`` (NHWC storage);
parameters stay fp32 (master weights) and are cast to bf16 shadows that the
kernels read; gradients of parameters are produced in fp32.

One module per kernel family, each importing the names it calls from the ones below it:
``tuning`` and ``lib`` (the library handle and the helpers every wrapper uses) at the bottom, then
``shadows``, ``gemm`` and ``data``, then ``conv`` -> ``bn_unit`` -> ``bottleneck`` / ``stem_pool`` (ResNet),
``fp8`` -> ``linear`` / ``layernorm`` / ``attention`` and ``embed`` (ViT), ``loss`` and ``lenet``.
This file only re-exports every name of every module, private ones included, so that
an attribute of ``native_ops`` reaches what it always did (``linear``, ``attention``, ``bottleneck`` and
``stem_pool`` are the functions, not the modules of the same name). State lives in its module: the dictionaries and singletons are mutated in place,
so the references here stay valid; the library handle ``lib._lib`` is rebound by ``_load()`` and is
read through ``_load()`` alone. To replace a function under test, patch it in its own module,
where its callers look it up.
"""
import importlib
import pkgutil

for _m in pkgutil.iter_modules(__path__):
    globals().update((k, v) for k, v in vars(importlib.import_module(f"{__name__}.{_m.name}")).items()
                     if not k.startswith("__"))
del importlib, pkgutil, _m
