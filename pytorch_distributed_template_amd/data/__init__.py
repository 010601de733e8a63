"""Data loader registry (``*_loader.type`` in config).

Reference: ``/root/reference/data_loader/data_loaders.py`` (MnistDataLoader).
"""
from .mnist import MnistDataLoader, MnistDataset, read_idx, synthetic_mnist  # noqa: F401
from .packed import (PackedImageLoader, PackedImageSet, center_crop_boxes, open_packed,  # noqa: F401
                     random_resized_crop_boxes)
from .samplers import EvalShardSampler, shard_bounds  # noqa: F401
from .synthetic import (SyntheticImageDataset, SyntheticImageLoader, SyntheticImageNet,  # noqa: F401
                        SyntheticImageNetLoader)
