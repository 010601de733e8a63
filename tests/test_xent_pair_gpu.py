"""The paired-target cross-entropy kernels (csrc/xent.hip: pdt_xent_pair_fwd / _bwd) against a
float64 reference, with the allowance scheme of tests/test_row_kernels_gpu.py: nothing is fixed
in advance. E_ref is the largest error of PyTorch's own fp32 GPU ops on the same inputs
(torch.logsumexp; F.cross_entropy with the dense soft-target matrix, and its autograd) against
float64; the kernel is allowed 4 x E_ref, floored at one fp32 unit roundoff of the case's largest
|reference|, plus the bf16 half-ulp on dlogits and the propagation of the stored lse's own error
(the reason is in test_xent's docstring there). Outputs and lse are guard-banded; each case prints
a ``MEASURED`` line."""
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_ref as kr
import mix_ref as M

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402

DEV = torch.device("cuda")
BF, F32 = torch.bfloat16, torch.float32
LAMS = [0.0, 1.0, 0.5, 0.3]


def G(shape, dtype):
    return kr.guarded(shape, dtype, DEV)


def done(what):
    torch.cuda.synchronize()
    kr.check_guards(what)


def emax(a, ref64):
    return (kr.f64(a) - ref64).abs().max().item()


def allowance(e_ref, ref64):
    return 4 * max(e_ref, kr.U * ref64.abs().max().item())


def xent_inputs(B, V, bf16, g):
    """The logits of test_row_kernels_gpu.xent_inputs: the maximum in the first column, in the last
    column, an all-equal row, a +-80 row."""
    x = kr.normal((B, V), g, BF if bf16 else F32, std=3.0)
    t = torch.randint(0, V, (B,), generator=g, device=DEV)
    x[0, 0], t[0] = 20.0, 0
    if B > 1:
        x[1, V - 1], t[1] = 20.0, V - 1
    if B > 2:
        x[2] = 1.5
    if B > 3:
        x[3] = (torch.randint(0, 2, (V,), generator=g, device=DEV).to(x.dtype) * 2 - 1) * 80
    return x, t


def pair_targets(B, V, ta, g):
    """tb and lam for the rows: ta at column 0 with tb at column V-1 (row 0), ta == tb (row 1), lam
    cycling through {0, 1, 0.5, float32(0.3)}, random elsewhere."""
    tb = torch.randint(0, V, (B,), generator=g, device=DEV)
    lam = torch.rand((B,), generator=g, device=DEV, dtype=F32)
    for r in range(min(B, 8)):
        lam[r] = LAMS[r % 4]
    tb[0] = V - 1            # row 0: ta = 0 (xent_inputs), tb = V - 1, lam = 0: all the weight on tb
    if B > 1:
        tb[1] = ta[1]        # ta == tb
    if B > 4:
        ta[4], tb[4] = 0, V - 1  # the same two columns with a blended weight
        lam[4] = 0.3
    return tb, lam


def pair_ref(x, ta, tb, lam, eps, gout):
    """float64: loss rows, their mean, lse, softmax, dlogits and the sums of their terms' magnitudes."""
    x = kr.f64(x)
    B, V = x.shape
    m = x.max(1, keepdim=True).values
    lse = (m + torch.log(torch.exp(x - m).sum(1, keepdim=True)))[:, 0]
    lam = kr.f64(lam)
    ta, tb = ta.view(-1, 1), tb.view(-1, 1)  # on the logits' device, like the float64 logits
    xa, xb = x.gather(1, ta)[:, 0], x.gather(1, tb)[:, 0]
    rows = lse - (1 - eps) * (lam * xa + (1 - lam) * xb) - eps * x.mean(1)
    tgt = torch.zeros_like(x).scatter_add_(1, ta, lam[:, None]).scatter_add_(1, tb, (1 - lam)[:, None])
    p = torch.exp(x - lse[:, None])
    return dict(lse=lse, loss_rows=rows, loss=rows.sum() / B, softmax=p,
                loss_rows_abs=lse.abs() + (1 - eps) * ((lam * xa).abs() + ((1 - lam) * xb).abs()) + eps * x.abs().mean(1),
                dlogits=gout / B * (p - (1 - eps) * tgt - eps / V),
                dlogits_abs=abs(gout) / B * (p + (1 - eps) * tgt + eps / V))


@pytest.mark.parametrize("B", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("V", [2, 10, 63, 64, 65, 1000, 1001])
def test_xent_pair(V, B):
    lib = no._load()
    g = kr.gen(2000 * B + V)
    for bf16 in (1, 0):
        for eps in (0.0, 0.1):
            what = f"xent_pair V={V} B={B} bf16={bf16} eps={eps}"
            epsf = float(torch.tensor(eps, dtype=F32))
            x, ta = xent_inputs(B, V, bf16, g)
            tb, lam = pair_targets(B, V, ta, g)
            gout = torch.tensor([1.7], device=DEV)
            lse, rows, loss, dl = G(B, F32), G(B, F32), G(1, F32), G((B, V), BF)
            assert lib.pdt_xent_pair_fwd(no._p(x), bf16, no._p(ta), no._p(tb), no._p(lam), no._p(lse), no._p(rows),
                                         no._p(loss), B, V, epsf, no._s()) == 0, what
            done(what)
            assert lib.pdt_xent_pair_bwd(no._p(x), bf16, no._p(ta), no._p(tb), no._p(lam), no._p(lse), no._p(gout),
                                         no._p(dl), B, V, epsf, no._s()) == 0, what
            done(what + " bwd")
            ref = pair_ref(x, ta, tb, lam, epsf, float(gout.item()))
            # PyTorch's fp32 ops on the same inputs: the dense soft target carries the label smoothing
            xx = x.float().requires_grad_()
            soft = M.soft_targets(ta, tb, lam, V, epsf).to(F32).to(DEV)
            rows_t = F.cross_entropy(xx, soft, reduction="none")
            loss_t = rows_t.mean()
            (loss_t * gout[0]).backward()
            e_lse = emax(torch.logsumexp(x.float(), 1), ref["lse"])
            e_rows, e_loss = emax(rows_t.detach(), ref["loss_rows"]), emax(loss_t.detach(), ref["loss"])
            e_dl = emax(xx.grad, ref["dlogits"])
            a_lse = allowance(e_lse, ref["lse"])
            a_rows = allowance(e_rows, ref["loss_rows_abs"])
            a_dl = allowance(e_dl, ref["dlogits"])
            k_dl = ((kr.f64(dl) - ref["dlogits"]).abs() - kr.BF16_HALF * ref["dlogits"].abs()).clamp_min(0).max().item()
            print(f"MEASURED {what}: lse ref {e_lse:.3e} kernel {emax(lse, ref['lse']):.3e} (allow {a_lse:.3e}); "
                  f"rows ref {e_rows:.3e} kernel {emax(rows, ref['loss_rows']):.3e} (allow {a_rows:.3e}); "
                  f"mean ref {e_loss:.3e} kernel {emax(loss[0], ref['loss']):.3e}; "
                  f"dlogits ref {e_dl:.3e} kernel beyond bf16 half-ulp {k_dl:.3e} (allow {a_dl:.3e})")
            kr.assert_close(lse, ref["lse"], a_lse, what + " lse")
            kr.assert_close(rows, ref["loss_rows"], a_rows, what + " loss rows")
            mabs = ref["loss_rows"].abs().mean().item()
            a_mean = a_rows + allowance(e_loss, ref["loss"]) + 2 * (math.ceil(B / 256) + 10) * kr.U * mabs
            kr.assert_close(loss[0], ref["loss"], a_mean, what + " mean loss")
            prop = abs(gout.item()) / B * ref["softmax"] * (
                a_lse + 4 * kr.U * (kr.f64(x) - ref["lse"][:, None]).abs())
            kr.assert_bf16_close(dl, ref["dlogits"], ref["dlogits_abs"], what + " dlogits", roundings=0,
                                 extra=a_dl + prop)
            # softmax - target distribution sums to 0: each stored entry is off by at most half a bf16
            # ulp of the row's largest entry
            big = kr.f64(dl).abs().max(1).values
            assert bool((kr.f64(dl).sum(1).abs() <= V * 0.5 * kr.ulp_bf16(big) + prop.sum(1)).all()), what + " row sums"
            assert torch.isfinite(lse).all() and torch.isfinite(dl.float()).all() and torch.isfinite(rows).all(), what

            # lam = 1: the plain kernels on ta, within the same allowances (both sides share the lse)
            one = torch.ones(B, device=DEV)
            lse1, rows1, loss1, dl1 = G(B, F32), G(B, F32), G(1, F32), G((B, V), BF)
            lse0, rows0, loss0, dl0 = G(B, F32), G(B, F32), G(1, F32), G((B, V), BF)
            assert lib.pdt_xent_pair_fwd(no._p(x), bf16, no._p(ta), no._p(tb), no._p(one), no._p(lse1), no._p(rows1),
                                         no._p(loss1), B, V, epsf, no._s()) == 0
            assert lib.pdt_xent_pair_bwd(no._p(x), bf16, no._p(ta), no._p(tb), no._p(one), no._p(lse1), no._p(gout),
                                         no._p(dl1), B, V, epsf, no._s()) == 0
            assert lib.pdt_xent_fwd(no._p(x), bf16, no._p(ta), no._p(lse0), no._p(rows0), no._p(loss0), B, V, epsf,
                                    no._s()) == 0
            assert lib.pdt_xent_bwd(no._p(x), bf16, no._p(ta), no._p(lse0), no._p(gout), no._p(dl0), B, V, epsf,
                                    no._s()) == 0
            done(what + " lam=1")
            kr.assert_close(lse1, kr.f64(lse0), a_lse, what + " lam=1 lse")
            kr.assert_close(rows1, kr.f64(rows0), a_rows, what + " lam=1 rows")
            kr.assert_close(loss1[0], kr.f64(loss0[0]), a_mean, what + " lam=1 mean")
            ref0 = kr.xent_ref(x, ta, epsf, gout=float(gout.item()))
            kr.assert_bf16_close(dl1, ref0["dlogits"], ref0["dlogits_abs"], what + " lam=1 dlogits", roundings=0,
                                 extra=a_dl + prop)
            print(f"MEASURED {what} lam=1: bitwise equal to the plain kernels: "
                  f"{torch.equal(rows1, rows0) and torch.equal(dl1.view(torch.int16), dl0.view(torch.int16))}")


@pytest.mark.parametrize("bf16", [1, 0])
def test_out_of_range_label_gives_a_zero_row(bf16):
    lib = no._load()
    B, V = 6, 65
    g = kr.gen(9)
    x, ta = xent_inputs(B, V, bf16, g)
    tb, lam = pair_targets(B, V, ta, g)
    ta[2], tb[3], ta[5], tb[5] = V, -1, -7, V + 3
    bad = [2, 3, 5]
    gout = torch.tensor([1.0], device=DEV)
    lse, rows, loss, dl = G(B, F32), G(B, F32), G(1, F32), G((B, V), BF)
    assert lib.pdt_xent_pair_fwd(no._p(x), bf16, no._p(ta), no._p(tb), no._p(lam), no._p(lse), no._p(rows),
                                 no._p(loss), B, V, 0.1, no._s()) == 0
    assert lib.pdt_xent_pair_bwd(no._p(x), bf16, no._p(ta), no._p(tb), no._p(lam), no._p(lse), no._p(gout),
                                 no._p(dl), B, V, 0.1, no._s()) == 0
    done("out of range")
    assert not rows[bad].any() and not dl[bad].view(torch.int16).any()
    good = [0, 1, 4]
    assert (rows[good] != 0).all() and dl[good].float().abs().sum(1).min() > 0
    assert torch.isfinite(loss).all() and torch.isfinite(lse).all()
    for k in (0, 2, 3, 4, 5, 6, 7):  # null pointers
        args = [no._p(x), bf16, no._p(ta), no._p(tb), no._p(lam), no._p(lse), no._p(rows), no._p(loss), B, V, 0.1,
                no._s()]
        args[k] = None
        assert lib.pdt_xent_pair_fwd(*args) == -1


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_autograd_function_matches_the_torch_path(eps):
    """fused.softmax_cross_entropy with a MixedTarget: the native Function against the torch path
    (bf16 logits; the gradient is bf16: one ulp of its largest entry)."""
    from pytorch_distributed_template_amd.data import MixedTarget
    from pytorch_distributed_template_amd.ops import fused
    g = kr.gen(77)
    B, V = 33, 1000
    x, ta = xent_inputs(B, V, 1, g)
    tb, lam = pair_targets(B, V, ta, g)
    t = MixedTarget(ta, tb, lam)
    out = {}
    try:
        for backend in ("native", "torch"):
            fused.set_backend(backend)
            xx = x.clone().requires_grad_()
            loss = fused.softmax_cross_entropy(xx, t, eps)
            loss.backward()
            out[backend] = (loss.detach().double(), xx.grad.double())
    finally:
        fused.set_backend("auto")
    torch.testing.assert_close(out["native"][0], out["torch"][0], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out["native"][1], out["torch"][1], rtol=2.0 ** -7, atol=1e-6)
