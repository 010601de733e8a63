"""References for the weight-EMA kernel (csrc/ema.hip) and ``optim.ModelEMA``: the recurrence in
float64, the tick in numpy fp32, and the bound on what fp32 arithmetic may add.

The recurrence, per element, with this update's weight ``w`` (and ``d = 1 - w``)::

    e_n = e_{n-1} + w (p_n - e_{n-1})

``tick()`` mirrors ``ema_tick_kernel`` operation for operation in numpy fp32, so ``t``, ``d`` and
``w`` are reproduced bit for bit; ``ref_update()`` is the recurrence in float64 with ``w`` taken
as the fp32 value the kernel uses -- its own rounding error (2^-53 relative) is 2^-29 of the
bound below and is ignored.

Error bound. With u = 2^-24 (fp32 unit roundoff) the kernel rounds three times per update:

    s = fl(p - e)        |s - (p - e)|  <= u |p - e|
    m = fl(w s)          |m - w s|      <= u |w s|      (fused into the add: this rounding vanishes)
    r = fl(e + m)        |r - (e + m)|  <= u |e + m|

so, given the same inputs, |r - (e + w (p - e))| <= u (2 w |p - e| + |r|) (1 + 2u): the first two
roundings are each at most u w |p - e| (1 + u), the last u |e + m| with |e + m| <= |r| (1 + u).
An error err_{n-1} already in e enters r as (1 - w) err_{n-1} = d err_{n-1} (e appears as
(1 - w) e in the exact result; the rounding terms change by O(u err), absorbed in the margin):

    err_n <= d_n err_{n-1} + step_n,   step_n = 1.01 u (2 w_n |p_n - e_{n-1}| + |e_n|)

with the reference's values on the right-hand side; the factor 1.01 covers every second-order
term (each is below 4u ~ 2.4e-7 relative). ``Bound`` carries err_n per element.

torch's ``lerp_`` evaluates the same form for w < 0.5 and ``p - (p - e) (1 - w)`` for w >= 0.5:
that one rounds (1 - w), the subtract, the multiply and the final subtract, |error| <=
u (3 (1 - w) |p - e| + |r|), inside step_n where w >= 0.6 and by at most a factor 1.5 / (2 w)
outside for 0.5 <= w < 0.6 in the worst case only -- tests/test_ema_cpu.py shows that the actual
error stays inside the bound over the general family's warm-up, which crosses that range.
"""
import numpy as np
import torch

U = 2.0 ** -24
MARGIN = 1.01


def tick(t, decay, warmup):
    """``(t, decay, warmup) -> (t + 1, d, w)`` as numpy fp32, as the tick kernel computes them."""
    f = np.float32
    t = f(t)
    d = f(decay)
    if warmup:
        d = min(d, f((f(1) + t) / (f(10) + t)))
    return f(t + f(1)), f(d), f(f(1) - d)


def schedule(n, decay, warmup, t0=0):
    """The first ``n`` ticks from ``t0``: a list of ``(t_after, d, w)``."""
    out, t = [], np.float32(t0)
    for _ in range(n):
        t, d, w = tick(t, decay, warmup)
        out.append((t, d, w))
    return out


def ref_update(e64, p, w):
    """One update in float64; ``p`` any float tensor, ``w`` the kernel's fp32 weight."""
    return e64 + float(w) * (p.double() - e64)


class Bound:
    """err_n per element, carried along a float64 reference run."""

    def __init__(self, e0):
        self.e = e0.double().clone()
        self.err = torch.zeros_like(self.e)

    def update(self, p, w):
        w = float(w)
        p = p.double()
        new = self.e + w * (p - self.e)
        step = MARGIN * U * (2.0 * w * (p - self.e).abs() + new.abs())
        self.err = (1.0 - w) * self.err + step
        self.e = new
        return new

    def ratio(self, got):
        """The worst |got - reference| / bound over the elements (0 where both are 0)."""
        diff = (got.double() - self.e).abs()
        r = torch.where(self.err > 0, diff / self.err.clamp_min(1e-300), torch.where(diff > 0, torch.inf, 0.0))
        return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------- input families
SIZES = [1, 3, 1023, 1024, 1025, 4 * 1024 + 5]
CL_SHAPE = (16, 8, 3, 3)


def exact_values(shape, gen):
    """Integer multiples of 2^8 with magnitude <= 2^15: with w in {1, 0.5, 0.25} and 4 updates
    every intermediate (p - e: multiples of 2^4 .. 2^8 below 2^17; w s; e + m) fits 24 bits."""
    return (torch.randint(-128, 129, tuple(shape), generator=gen) * 256).float()


def bf16_trunc(x):
    """The seeded shadow fault: fp32 -> bf16 by dropping the low 16 bits."""
    return (x.contiguous().view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)
