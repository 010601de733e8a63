"""The packed loader's pinned parameter block (data/packed.py: _param_layout): the word layout the
loader has uploaded since Mixup / CutMix and Random Erasing went in, written out here as numbers."""
import pytest
import torch

from pytorch_distributed_template_amd.data.packed import _block_views, _param_layout

# (offset, words) of every field in units of B int32 words, as the uploads were hand-numbered:
# host[:2B] kidx, host[2B:4B] labels, host[4B:9B] box; mixed: four int64 vectors in host[:8B], then
# host[8B:13B] box, [13B:18B] pbox, [18B:22B] rect, [22B:23B] w_own, [23B:24B] lam
PLAIN = {"kidx": (0, 2), "labels": (2, 2), "box": (4, 5)}
MIXED = {"kidx": (0, 2), "labels": (2, 2), "pidx": (4, 2), "plabels": (6, 2), "box": (8, 5), "pbox": (13, 5),
         "rect": (18, 4), "w_own": (22, 1), "lam": (23, 1)}
INT64 = ("kidx", "labels", "pidx", "plabels")


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("mixing", [False, True])
@pytest.mark.parametrize("R", [0, 1, 8])
def test_param_layout(B, mixing, R):
    lay = _param_layout(B, mixing, R)
    base = 24 * B if mixing else 9 * B
    want = {k: (o * B, n * B) for k, (o, n) in (MIXED if mixing else PLAIN).items()}
    if R:  # the rectangles, then one key per sample, behind everything else
        want["erect"] = (base, 4 * R * B)
        want["ekey"] = (base + 4 * R * B, B)
    assert {k: v[:2] for k, v in lay.items()} == want
    total = max(o + n for o, n, _, _ in lay.values())
    assert total == base + ((4 * R + 1) * B if R else 0)
    words = sorted((o, o + n) for o, n, _, _ in lay.values())
    assert words[0][0] == 0 and all(a[1] == b[0] for a, b in zip(words, words[1:]))  # no overlap, no hole
    for name, (off, n, dtype, shape) in lay.items():
        assert (dtype == torch.int64) == (name in INT64)
        if dtype == torch.int64:
            assert off % 2 == 0 and n == 2 * B and shape == (B,)
    assert lay["box"][2:] == (torch.int32, (B, 5))
    if mixing:
        assert lay["pbox"][2:] == (torch.int32, (B, 5)) and lay["rect"][2:] == (torch.int32, (B, 4))
        assert lay["w_own"][2:] == (torch.float32, (B,)) and lay["lam"][2:] == (torch.float32, (B,))
    if R:
        assert lay["erect"][2:] == (torch.int32, (B, R, 4)) and lay["ekey"][2:] == (torch.int32, (B,))


def test_block_views_alias_the_words():
    lay = _param_layout(3, True, 2)
    buf = torch.arange(24 * 3 + 9 * 3, dtype=torch.int32)
    v = _block_views(buf, lay)
    assert v["rect"].shape == (3, 4) and v["rect"][0, 0] == 18 * 3
    assert v["erect"].shape == (3, 2, 4) and v["erect"][0, 0, 0] == 24 * 3 and v["ekey"][0] == 24 * 3 + 8 * 3
    assert v["pidx"].dtype == torch.int64 and v["pidx"].data_ptr() == buf.data_ptr() + 4 * 4 * 3
