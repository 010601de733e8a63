"""Float64 reference for Mixup / CutMix in the packed-image pipeline, built on
packed_ref.reference. Nothing here touches the code under test.

mixed(): the own view and the partner's view (its own image, box and flip), both in float64;
outside the rectangle w_own * own + (1 - w_own) * partner with the float32 value of w_own,
inside it the partner's pixel. The blend commutes with the normalization (the weights sum to 1),
so it is formed on the normalized views.
"""
import numpy as np
import torch

import packed_ref as R


def inside(rect, S):
    """bool [B, 1, S, S]: output pixels inside rect rows (y0, x0, y1, x1), half-open."""
    r = torch.as_tensor(np.asarray(rect), dtype=torch.int64).reshape(-1, 4)
    B = r.shape[0]
    yy = torch.arange(S).view(1, S, 1)
    xx = torch.arange(S).view(1, 1, S)
    m = ((yy >= r[:, 0].view(B, 1, 1)) & (yy < r[:, 2].view(B, 1, 1))
         & (xx >= r[:, 1].view(B, 1, 1)) & (xx < r[:, 3].view(B, 1, 1)))
    return m[:, None]


def mixed(images, idx, box, pidx, pbox, rect, w_own, S, mean=R.MEAN, std=R.STD):
    """float64 [B, 3, S, S]: output b mixes the view (idx[b], box[b]) with (pidx[b], pbox[b])."""
    own = R.reference(images, idx, box, S, mean, std)
    par = R.reference(images, pidx, pbox, S, mean, std)
    w = torch.as_tensor(np.asarray(w_own, dtype=np.float32)).to(torch.float64).view(-1, 1, 1, 1)
    return torch.where(inside(rect, S), par, w * own + (1.0 - w) * par)


def mixed_batch(images, indices, box, partner, rect, w_own, S, mean=R.MEAN, std=R.STD):
    """A loader batch: sample b is global image indices[b] with box[b]; its partner is sample
    partner[b] of the same batch (that sample's image and box)."""
    indices = [int(i) for i in indices]
    partner = [int(p) for p in partner]
    box = torch.as_tensor(np.asarray(box))
    return mixed(images, indices, box, [indices[p] for p in partner], box[partner], rect, w_own, S, mean, std)


def soft_targets(label_a, label_b, lam, V, eps=0.0):
    """float64 [B, V]: (1 - eps) (lam onehot(a) + (1 - lam) onehot(b)) + eps / V."""
    a = torch.as_tensor(label_a).cpu().view(-1, 1)
    b = torch.as_tensor(label_b).cpu().view(-1, 1)
    lam = torch.as_tensor(lam).cpu().to(torch.float64).view(-1, 1)
    t = torch.zeros(a.shape[0], V, dtype=torch.float64)
    t.scatter_add_(1, a, lam)
    t.scatter_add_(1, b, 1.0 - lam)
    return (1.0 - eps) * t + eps / V
