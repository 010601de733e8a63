"""MnistModel (the reference template's LeNet, ``model/model.py``) as two
whole-network kernels (csrc/lenet.hip: one workgroup per image, all layers in
LDS, fp32 like the reference); its NLL loss (``model/loss.py``) is in ``loss.py``.
"""
from __future__ import annotations

import torch

from .lib import _chk, _load, _p, _s


def lenet_supported(model, x) -> bool:
    c1, c2, f1, f2 = model.conv1, model.conv2, model.fc1, model.fc2
    return (x.is_cuda and x.dim() == 4 and tuple(x.shape[1:]) == (1, 28, 28)
            and (c1.in_channels, c1.out_channels, c1.kernel_size, c1.stride, c1.padding) == (1, 10, (5, 5), (1, 1), (0, 0))
            and (c2.in_channels, c2.out_channels, c2.kernel_size, c2.stride, c2.padding) == (10, 20, (5, 5), (1, 1), (0, 0))
            and (f1.in_features, f1.out_features) == (320, 50) and f2.in_features == 50 and f2.out_features <= 64
            and all(t is not None for t in (c1.bias, c2.bias, f1.bias, f2.bias)))


def _lenet_params(model):
    return [t.detach().float().contiguous() for t in (model.conv1.weight, model.conv1.bias, model.conv2.weight,
                                                      model.conv2.bias, model.fc1.weight, model.fc1.bias,
                                                      model.fc2.weight, model.fc2.bias)]


class _LeNet(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, wf1, bf1, wf2, bf2, training, p2, p1, seed, masks):
        x = x.float().contiguous()
        ps = [t.float().contiguous() for t in (w1, b1, w2, b2, wf1, bf1, wf2, bf2)]
        B, NC = x.shape[0], wf2.shape[0]
        logp = torch.empty((B, NC), dtype=torch.float32, device=x.device)
        m2, m1 = (masks if masks is not None else (None, None))
        _chk(_load().pdt_lenet_fwd(*[_p(t) for t in [x] + ps], B, NC, int(training), float(p2), float(p1),
                                   seed & 0xFFFFFFFF, _p(logp), _p(m2), _p(m1), _s()), "lenet_fwd")
        ctx.save_for_backward(x, *ps)
        ctx.meta = (B, NC, int(training), float(p2), float(p1), seed & 0xFFFFFFFF)
        return logp

    @staticmethod
    def backward(ctx, g):
        x, *ps = ctx.saved_tensors
        B, NC, training, p2, p1, seed = ctx.meta
        lib = _load()
        row = lib.pdt_lenet_grad_row(NC)
        part = torch.empty(B * row, dtype=torch.float32, device=x.device)
        flat = torch.empty(row, dtype=torch.float32, device=x.device)
        g = g.float().contiguous()
        _chk(lib.pdt_lenet_bwd(*[_p(t) for t in [x] + ps], B, NC, training, p2, p1, seed, _p(g), _p(part), _p(flat),
                               _s()), "lenet_bwd")
        grads, off = [], 0
        for t in ps:  # flat layout = parameter order (csrc/lenet.hip O_*)
            grads.append(flat[off:off + t.numel()].view(t.shape))
            off += t.numel()
        assert off == row
        if ctx.needs_input_grad[0]:
            raise NotImplementedError("native LeNet does not produce an input gradient")
        return (None, *grads, None, None, None, None, None)


def lenet_forward(model, x, masks=None, seed=None):
    """log-probabilities of MnistModel on x [B, 1, 28, 28] (Dropout2d / dropout active in training)."""
    p2 = model.conv2_drop.p if model.training else 0.0
    p1 = 0.5 if model.training else 0.0
    if seed is None:
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item()) if model.training else 0  # host RNG: no device sync
    return _LeNet.apply(x, model.conv1.weight, model.conv1.bias, model.conv2.weight, model.conv2.bias,
                        model.fc1.weight, model.fc1.bias, model.fc2.weight, model.fc2.bias, model.training, p2, p1,
                        seed, masks)
