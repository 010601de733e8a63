"""Float64 reference and input families for the streaming evaluation statistics
(csrc/eval_stats.hip, ``ops.fused.eval_stats_update``). A plain module like kernel_ref.py, which
it builds on: no fixtures, no pytest settings.

Definition (per row, target t, V columns)
-----------------------------------------
* rank = #{j : x[j] > x[t]} + #{j < t : x[j] == x[t]}: t's position in a stable descending sort.
  rank == 0 exactly when ``torch.argmax`` returns t (first maximum; -0 == +0). A row holding a NaN
  gets rank V; so does a target outside [0, V), whose loss is 0 and which is counted out of range.
* a row is correct at k iff rank < min(k, V): a row of rank V is never correct, so k >= V counts
  exactly the rows with a target in range and no NaN.
* loss: "ce"  lse(x) - (1 - eps) x[t] - eps mean(x)   (``kernel_ref.xent_ref``'s formula)
        "nll" -x[t]
* accumulators: sum of the row losses (float64) and int64 [rows, out of range, correct at each k].

``fault`` seeds one wrong rule into the reference (tests/test_eval_stream_cpu.py shows that each is
caught by a named check): "ge" (>= where > belongs), "ties_after" (equal values counted behind the
target instead of before it), "nan_correct" (no NaN rule), "drop_last" (the last column unread).
"""
import torch

import kernel_ref as kr

FAULTS = ("ge", "ties_after", "nan_correct", "drop_last")
FAMILIES = ("xent", "ties", "zeros", "nan", "oor")


def eval_ref(logits, target, kind="ce", eps=0.0, ks=(1,), fault=None):
    assert fault is None or fault in FAULTS
    x = kr.f64(logits)
    B, V = x.shape
    t = target.to(torch.long)
    valid = (t >= 0) & (t < V)
    tc = t.clamp(0, V - 1).unsqueeze(1)
    xt = x.gather(1, tc)
    cols = torch.arange(V, device=x.device).unsqueeze(0)
    seen = cols < V - 1 if fault == "drop_last" else cols < V
    gt = (x >= xt) if fault == "ge" else (x > xt)
    tie = (x == xt) & ((cols > tc) if fault == "ties_after" else (cols < tc))
    above = ((gt | tie) & seen).sum(1)
    nan = torch.isnan(x).any(1)
    ok = valid if fault == "nan_correct" else valid & ~nan
    rank = torch.where(ok, above, torch.full_like(above, V))
    if kind == "nll":
        rows, rows_abs = -xt[:, 0], xt[:, 0].abs()
    else:
        m = x.max(1, keepdim=True).values
        lse = (m + torch.log(torch.exp(x - m).sum(1, keepdim=True)))[:, 0]
        lse = torch.where(nan, torch.full_like(lse, float("nan")), lse)  # (max() is not required to propagate)
        rows = lse - (1 - eps) * xt[:, 0] - eps * x.mean(1)
        rows_abs = lse.abs() + ((1 - eps) * xt[:, 0]).abs() + eps * x.abs().mean(1)
    rows = torch.where(valid, rows, torch.zeros_like(rows))
    rows_abs = torch.where(valid, rows_abs, torch.zeros_like(rows_abs))
    counts = [B, int((~valid).sum())] + [int((rank < min(k, V)).sum()) for k in ks]
    return dict(rank=rank, loss_rows=rows, loss_rows_abs=rows_abs, loss_sum=rows.sum(), valid=valid, nan=nan,
                counts=torch.tensor(counts, dtype=torch.int64))


# ---------------------------------------------------------------------------- input families
def _xent(B, V, dtype, g):
    """tests/test_row_kernels_gpu.py's cross-entropy input: the maximum in the first column, in the
    last column, an all-equal row and a +-80 row."""
    x = kr.normal((B, V), g, dtype, std=3.0)
    t = torch.randint(0, V, (B,), generator=g, device=g.device)
    x[0, 0], t[0] = 20.0, 0
    if B > 1:
        x[1, V - 1], t[1] = 20.0, V - 1
    if B > 2:
        x[2] = 1.5
    if B > 3:
        x[3] = (torch.randint(0, 2, (V,), generator=g, device=g.device).to(x.dtype) * 2 - 1) * 80
    return x, t


def family(name, B, V, dtype, g):
    """(x [B, V] ``dtype``, t int64 [B]) of one family (the NLL kind reads the same values: it scores
    -x[t] whatever the row sums to)."""
    assert name in FAMILIES
    x, t = _xent(B, V, dtype, g)
    if name == "ties":
        # the target's value duplicated just before it, just after it, at column 0 and at column
        # V-1 (row r takes variant r % 4); every other row raises the target so the ties lead
        r = torch.arange(B, device=g.device)
        x[r[::2], t[::2]] = 10.0
        j = torch.stack([t - 1, t + 1, torch.zeros_like(t), torch.full_like(t, V - 1)])[r % 4, r]
        ok = (j >= 0) & (j < V)
        x[r[ok], j[ok]] = x[r[ok], t[ok]]
    elif name == "zeros":
        # +0 / -0 everywhere (rank = t: every earlier column ties), or among negative values
        sign = torch.randint(0, 2, (B, V), generator=g, device=g.device).to(dtype) * 2 - 1
        zeros = torch.zeros((B, V), dtype=dtype, device=g.device) * sign
        keep = torch.randint(0, 2, (B, V), generator=g, device=g.device).bool()
        keep[::2] = False
        x = torch.where(keep, -x.abs() - 1, zeros)
        x[torch.arange(B, device=g.device), t] = zeros[torch.arange(B, device=g.device), t]
    elif name == "nan":
        x[0, int(t[0])] = float("nan")  # at the target itself
        if B > 1 and V > 1:
            x[1, (int(t[1]) + 1) % V] = float("nan")  # elsewhere in the row
    elif name == "oor":
        t[0] = -1
        if B > 1:
            t[B - 1] = V
    return x, t


def strided(x, pad):
    """``x`` as a view with row stride V + pad; the pad columns hold NaN, so a read past a row's end
    turns that row's rank into V and its loss into NaN."""
    if pad == 0:
        return x.contiguous()
    B, V = x.shape
    full = torch.full((B, V + pad), float("nan"), dtype=x.dtype, device=x.device)
    full[:, :V] = x
    return full[:, :V]
