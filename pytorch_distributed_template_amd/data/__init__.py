"""Data loader registry (``*_loader.type`` in config).

Reference: ``/root/reference/data_loader/data_loaders.py`` (MnistDataLoader).
"""
from .mnist import MnistDataLoader, MnistDataset, read_idx, synthetic_mnist  # noqa: F401
from .packed import (MixedTarget, PackedImageLoader, PackedImageSet, center_crop_boxes, erase_keys,  # noqa: F401
                     mix_params, open_packed, random_erasing_rects, random_resized_crop_boxes, validate_erase,
                     validate_mix)
from .samplers import EvalShardSampler, shard_bounds  # noqa: F401
from .synthetic import (SyntheticImageDataset, SyntheticImageLoader, SyntheticImageNet,  # noqa: F401
                        SyntheticImageNetLoader)
