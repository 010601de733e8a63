"""Fused fp8 attention backward (csrc/attention_bwd_f8.hip): dQ, dK, dV of each (batch, head)
in one kernel, every GEMM on e4m3 mfma_scale_f32_32x32x64_f8f6f4.

(1) against an fp32 emulation of the kernel's own quantisation (per-head power-of-two
    scales for Q, K, V, dO; P coded as 256 P; dS with one power-of-two scale per 32 x 32
    tile; e4m3 round-to-nearest): pins the kernel's indexing, lane exchanges and scales;
(2) against exact fp32 attention gradients: the fp8 error budget, next to the bf16
    kernel's error on the same inputs.
Forward output and log-sum-exp come from the bf16 forward kernel in both."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402


def nrmerr(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _pow2(amax):
    e = torch.floor(torch.log2(448.0 / amax.clamp_min(1e-30))).clamp(-100, 100)
    return torch.where(amax > 0, torch.exp2(e), torch.ones_like(amax))


def _q8(x, s):
    return (x * s).to(torch.float8_e4m3fn).float() / s


def _head_q8(x):  # [B, H, T, 64], one scale per (b, h)
    return _q8(x, _pow2(x.abs().amax(dim=(2, 3), keepdim=True)))


def _tile_q8(ds):  # [B, H, T, T], one scale per 32 x 32 tile
    B, H, T, _ = ds.shape
    n = (T + 31) // 32
    x = torch.nn.functional.pad(ds, (0, 32 * n - T, 0, 32 * n - T)).view(B, H, n, 32, n, 32)
    s = _pow2(x.abs().amax(dim=(3, 5), keepdim=True))
    return _q8(x, s).view(B, H, 32 * n, 32 * n)[:, :, :T, :T]


def _bf16_forward(qkv, H):
    B, T, _ = qkv.shape
    out = torch.empty((B, T, H * 64), dtype=torch.bfloat16, device="cuda")
    lse = torch.empty((B * H, T), dtype=torch.float32, device="cuda")
    no._chk(no._load().pdt_attn_fwd(no._p(qkv), no._p(out), no._p(lse), B, T, H, 0.125, no._s()), "fwd")
    return out, lse


# (40, 197, 12) / (8, 64, 40): more heads than CUs -- the persistent kernel's workgroups walk
# several heads each, the next head's operands prefetched across the dQ phase
@pytest.mark.parametrize("B,T,H", [(3, 197, 4), (2, 64, 2), (1, 50, 12), (2, 256, 3), (2, 16, 3), (1, 120, 2),
                                   (40, 197, 12), (8, 64, 40)])
def test_attention_bwd_f8(B, T, H):
    torch.manual_seed(B * 1000 + T)
    lib = no._load()
    qkv = (torch.randn(B, T, 3 * H * 64, device="cuda") * 1.5).to(torch.bfloat16)
    dout = torch.randn(B, T, H * 64, device="cuda").to(torch.bfloat16)
    out, lse = _bf16_forward(qkv, H)
    d8 = torch.full_like(qkv, float("nan"))
    R = 64 * ((T + 63) // 64)
    dbg = torch.zeros(B * H, R, R, device="cuda")
    no._chk(lib.pdt_attn_bwd_f8_debug(no._p(qkv), no._p(out), no._p(dout), no._p(lse), no._p(d8), B, T, H, 0.125,
                                      no._p(dbg), no._s()), "attn_bwd_f8")
    d16 = torch.empty_like(qkv)
    delta = torch.empty_like(lse)
    no._chk(lib.pdt_attn_bwd(no._p(qkv), no._p(out), no._p(dout), no._p(lse), no._p(delta), no._p(d16), B, T, H,
                             0.125, no._s()), "attn_bwd")
    torch.cuda.synchronize()
    assert torch.isfinite(d8.float()).all()

    q, k, v = qkv.float().view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    do = dout.float().view(B, T, H, 64).transpose(1, 2)
    o = out.float().view(B, T, H, 64).transpose(1, 2)
    lse2 = lse.view(B, H, T, 1)
    c = 0.125 / math.log(2.0)
    # (1) the kernel's quantisation model in fp32
    Q8, K8, V8, O8 = _head_q8(q), _head_q8(k), _head_q8(v), _head_q8(do)
    P = torch.exp2(Q8 @ K8.transpose(-1, -2) * c - lse2)
    dS = P * (O8 @ V8.transpose(-1, -2) - (do * o).sum(-1, keepdim=True))
    eds = nrmerr(dbg.view(B, H, R, R)[:, :, :T, :T], dS)
    assert eds < 1e-4, eds  # phase 1's fp32 dS
    P8 = _q8(P, 256.0)
    dS8 = _tile_q8(dS)
    m_dv = P8.transpose(-1, -2) @ O8
    m_dk = 0.125 * dS8.transpose(-1, -2) @ Q8
    m_dq = 0.125 * dS8 @ K8
    # (2) exact attention gradients (fp32 autograd from the same bf16 inputs)
    x = qkv.float().requires_grad_(True)
    qq, kk, vv = x.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    ref = (torch.softmax(qq @ kk.transpose(-1, -2) * 0.125, dim=-1) @ vv).transpose(1, 2).reshape(B, T, H * 64)
    ref.backward(dout.float())
    g8 = d8.float().view(B, T, 3, H, 64)
    g16 = d16.float().view(B, T, 3, H, 64)
    gr = x.grad.view(B, T, 3, H, 64)
    model = {"q": m_dq, "k": m_dk, "v": m_dv}
    errs = {}
    for i, name in enumerate("qkv"):
        em = nrmerr(g8[:, :, i].transpose(1, 2), model[name])
        e8, e16 = nrmerr(g8[:, :, i], gr[:, :, i]), nrmerr(g16[:, :, i], gr[:, :, i])
        emx = nrmerr(model[name], gr[:, :, i].transpose(1, 2))
        print(f"B{B} T{T} H{H} d{name}: vs model {em:.4f}  vs exact fp8 {e8:.4f} bf16 {e16:.4f} (model {emx:.4f})")
        errs[name] = (em, e8)
    for name, (em, e8) in errs.items():
        assert em < 2e-2, (name, em)  # the kernel == its quantisation model
        # fp8 error budget vs exact attention: dominated by the e4m3 score GEMM (an S error of
        # ~0.1 logit moves P by ~10 % at these x1.5 Gaussian inputs; the fp8 forward's own
        # output error is 6.5 %, tests/test_vit_fusion_gpu.py)
        assert e8 < 1.6e-1, (name, e8)


# T = 128 / 129: the last length of two query-tile pairs and the first of three (64, 50: one; 197: four)
@pytest.mark.parametrize("B,T,H", [(3, 197, 4), (40, 197, 12), (2, 64, 2), (1, 50, 12), (2, 128, 2), (2, 129, 2)])
def test_attention_bwd_f8_q8_epilogue(B, T, H):
    """pdt_attn_bwd_f8_q8: the qkv projection's e5m2 output-gradient codes, amax-history roll
    and dequant factor equal the separate delayed cast of the kernel's own bf16 d(qkv) bit for
    bit; the bf16 d(qkv) (when written) equals the plain kernel's; the bias gradient -- q part
    reduced in-kernel, k part 0 and v part sum_q dO (identities of the attention backward) --
    is at least as close to the exact fp32 bias gradient as the column sums of the written
    fp8-path gradient are."""
    torch.manual_seed(B * 7 + T)
    lib = no._load()
    n = 3 * H * 64
    qkv = (torch.randn(B, T, n, device="cuda") * 1.5).to(torch.bfloat16)
    dout = torch.randn(B, T, H * 64, device="cuda").to(torch.bfloat16)
    out, lse = _bf16_forward(qkv, H)
    d8 = torch.empty_like(qkv)
    no._chk(lib.pdt_attn_bwd_f8(no._p(qkv), no._p(out), no._p(dout), no._p(lse), no._p(d8), B, T, H, 0.125,
                                no._s()), "attn_bwd_f8")
    # the delayed-scaling state of a projection that has seen a few gradients
    _, _, meta = no.quantize_fp8_delayed((torch.randn(B * T, n, device="cuda") * 3e-3).to(torch.bfloat16), None,
                                         no.E5M2)
    meta_a, meta_b = meta.clone(), meta.clone()
    # reference: the separate cast with column sums over the bf16 gradient
    nb = lib.pdt_cast_cs_bands(B * T)
    cpart = torch.empty(nb * n + lib.pdt_reduce_rows_work(nb, n), device="cuda")
    q_ref = torch.empty(B * T, n, dtype=torch.uint8, device="cuda")
    dq_ref = torch.empty(1, device="cuda")
    db_ref = torch.empty(n, device="cuda")
    no._chk(lib.pdt_cast_fp8_delayed_cs(no._p(d8), B * T, n, no._p(meta_a), no.E5M2, no._p(q_ref), no._p(dq_ref),
                                        no._p(cpart), no._p(db_ref), no._s()), "cast_cs")
    # fused
    grid = lib.pdt_attn_bwd_f8_grid(B, H)
    part = torch.empty(grid, device="cuda")
    colpart = torch.empty(B * n + lib.pdt_reduce_rows_work(B, n), device="cuda")
    codes = torch.empty(B * T, n, dtype=torch.uint8, device="cuda")
    dq = torch.empty(1, device="cuda")
    db = torch.full((n,), float("nan"), device="cuda")
    d8b = torch.full_like(qkv, float("nan"))
    no._chk(lib.pdt_attn_bwd_f8_q8(no._p(qkv), no._p(out), no._p(dout), no._p(lse), no._p(d8b), B, T, H, 0.125,
                                   no._p(codes), no._p(meta_b), no._p(part), no._p(dq), no._p(colpart), no._p(db),
                                   no._s()), "attn_bwd_f8_q8")
    # without the bf16 output: the same codes
    codes2 = torch.empty_like(codes)
    meta_c = meta.clone()
    no._chk(lib.pdt_attn_bwd_f8_q8(no._p(qkv), no._p(out), no._p(dout), no._p(lse), None, B, T, H, 0.125,
                                   no._p(codes2), no._p(meta_c), no._p(part), no._p(dq), no._p(colpart), no._p(db),
                                   no._s()), "attn_bwd_f8_q8 (codes only)")
    torch.cuda.synchronize()
    assert torch.equal(d8b, d8)
    assert torch.equal(codes, q_ref) and torch.equal(codes2, q_ref)
    assert torch.equal(dq, dq_ref)
    assert torch.equal(meta_b, meta_a) and torch.equal(meta_c, meta_a)
    # exact fp32 bias gradient of the same attention
    qf = qkv.float().requires_grad_(True)
    q, k, v = qf.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4)
    o = torch.softmax((q @ k.transpose(-1, -2)) * 0.125, -1) @ v
    o.transpose(1, 2).reshape(B, T, H * 64).backward(dout.float())
    exact = qf.grad.sum((0, 1))
    hd = H * 64
    assert nrmerr(db[:hd], d8.float().sum((0, 1))[:hd]) < 1e-5  # q: the same sums, another order
    assert db[hd:2 * hd].abs().max().item() == 0.0
    assert nrmerr(db[2 * hd:], exact[2 * hd:]) < 1e-5
    assert nrmerr(db, exact) <= nrmerr(db_ref, exact) + 1e-4, (nrmerr(db, exact), nrmerr(db_ref, exact))
