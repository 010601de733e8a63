"""float64 references for FusedLARS / FusedLAMB, written from their definitions (shared by
tests/test_optim_layerwise_cpu.py and tests/test_optim_layerwise_gpu.py; no test lives here).

Parameters are held in float64 across all steps and rounded to fp32 only for the comparison.
``groups`` is a list of dicts {"w": [float64 tensors], "adapt": [bool], "weight_decay": float};
``grads`` passed to ``step`` mirrors that nesting."""
import math

import torch


def clip_coef(grads, max_grad_norm):
    if max_grad_norm <= 0:
        return 1.0
    gnorm = math.sqrt(sum(float((g * g).sum()) for gs in grads for g in gs))
    return min(1.0, max_grad_norm / (gnorm + 1e-6))


class RefLARS:
    def __init__(self, groups, momentum, nesterov, trust_coefficient, eps, max_grad_norm):
        self.groups = groups
        self.momentum, self.nesterov, self.tc, self.eps = momentum, nesterov, trust_coefficient, eps
        self.max_grad_norm = max_grad_norm
        self.bufs = [[None] * len(g["w"]) for g in groups]

    def step(self, grads, lr):
        clip = clip_coef(grads, self.max_grad_norm)
        for gi, group in enumerate(self.groups):
            wd = group["weight_decay"]
            for i, w in enumerate(group["w"]):
                g = grads[gi][i] * clip
                if group["adapt"][i]:
                    wn, gn = float(w.norm()), float(g.norm())
                    q = self.tc * wn / (gn + wd * wn + self.eps) if (wn > 0 and gn > 0) else 1.0
                    d = q * (g + wd * w)
                else:
                    d = g
                if self.momentum != 0:
                    buf = self.bufs[gi][i]
                    buf = d.clone() if buf is None else self.momentum * buf + d
                    self.bufs[gi][i] = buf
                    d = d + self.momentum * buf if self.nesterov else buf
                group["w"][i] = w - lr * d


class RefLAMB:
    def __init__(self, groups, betas, eps, max_grad_norm):
        self.groups = groups
        self.b1, self.b2 = betas
        self.eps, self.max_grad_norm = eps, max_grad_norm
        self.t = 0
        self.m = [[torch.zeros_like(w) for w in g["w"]] for g in groups]
        self.v = [[torch.zeros_like(w) for w in g["w"]] for g in groups]

    def step(self, grads, lr):
        clip = clip_coef(grads, self.max_grad_norm)
        self.t += 1
        bc1, bc2 = 1 - self.b1 ** self.t, 1 - self.b2 ** self.t
        for gi, group in enumerate(self.groups):
            for i, w in enumerate(group["w"]):
                g = grads[gi][i] * clip
                adapt = group["adapt"][i]
                m = self.m[gi][i] = self.b1 * self.m[gi][i] + (1 - self.b1) * g
                v = self.v[gi][i] = self.b2 * self.v[gi][i] + (1 - self.b2) * g * g
                u = (m / bc1) / ((v / bc2).sqrt() + self.eps) + (group["weight_decay"] if adapt else 0.0) * w
                wn, un = float(w.norm()), float(u.norm())
                r = wn / un if (adapt and wn > 0 and un > 0) else 1.0
                group["w"][i] = w - lr * r * u


# role of the two extra tensors every case carries
ZERO_GRAD, ZERO_WEIGHT = "zero_grad", "zero_weight"


def make_case(shapes, extra_shapes, device, seed, unaligned=False):
    """fp32 leaf parameters for ``shapes`` plus one tensor whose gradient is always zero and one
    whose weight starts at zero (both 2-D, so they are adapted: the q = 1 / r = 1 branches), in two
    groups. 4-D tensors are channels_last. ``unaligned``: every parameter is a view into one flat
    buffer starting at element 1 (4-byte aligned only: the kernels' scalar path).
    Returns (params, kinds, group index of each parameter)."""
    gen = torch.Generator().manual_seed(seed)
    all_shapes = list(shapes) + list(extra_shapes)
    kinds = [None] * len(shapes) + [ZERO_GRAD, ZERO_WEIGHT]
    total = sum(math.prod(s) for s in all_shapes)
    flat = torch.zeros(total + 1, device=device) if unaligned else None
    off, params = 1, []
    for s, kind in zip(all_shapes, kinds):
        t = torch.zeros(s) if kind == ZERO_WEIGHT else torch.randn(s, generator=gen)
        if len(s) == 4:
            t = t.contiguous(memory_format=torch.channels_last)
        if unaligned:
            n = t.numel()
            if len(s) == 4:
                view = flat[off:off + n].view(s[0], s[2], s[3], s[1]).permute(0, 3, 1, 2)
            else:
                view = flat[off:off + n].view(s)
            view.copy_(t)
            off += n
            t = view
        else:
            t = t.to(device)
        params.append(t.requires_grad_(True))
    # group 0: even positions, group 1: odd positions (each gets adapted and excluded tensors)
    group_of = [i % 2 for i in range(len(params))]
    return params, kinds, group_of


def make_grads(params, kinds, gen, steps):
    """``steps`` lists of fp32 CPU gradients, laid out like the parameters."""
    out = []
    for _ in range(steps):
        gs = []
        for p, kind in zip(params, kinds):
            g = torch.zeros(p.shape) if kind == ZERO_GRAD else torch.randn(p.shape, generator=gen)
            if p.dim() == 4:
                g = g.contiguous(memory_format=torch.channels_last)
            gs.append(g)
        out.append(gs)
    return out


def split(items, group_of):
    return [[x for x, g in zip(items, group_of) if g == gi] for gi in (0, 1)]


def ref_groups(params, group_of, weight_decays, exclude_1d):
    ps = split(params, group_of)
    return [{"w": [p.detach().cpu().double() for p in ps[gi]],
             "adapt": [not (exclude_1d and p.dim() <= 1) for p in ps[gi]],
             "weight_decay": weight_decays[gi]} for gi in (0, 1)]


def set_grads(params, grads):
    for p, g in zip(params, grads):
        g = g.to(p.device)
        if p.grad is None:
            p.grad = torch.empty_like(p)  # (a view parameter gets a dense gradient of its own layout)
        p.grad.copy_(g)


def assert_matches(params, group_of, ref, rtol=1e-5, atol=1e-6):
    for gi, ps in enumerate(split(params, group_of)):
        for i, p in enumerate(ps):
            want = ref.groups[gi]["w"][i].to(torch.float32)
            got = p.detach().cpu()
            assert torch.allclose(got, want, rtol=rtol, atol=atol), \
                (gi, i, tuple(p.shape), float((got - want).abs().max()))
