"""The bf16 attention kernels (csrc/attention.hip, the bf16 instantiation of csrc/attention_f8.hip,
csrc/attention_cls.hip) called entry point by entry point and compared element by element with the
float64 references of tests/kernel_ref.py (section "attention"; every bound is derived in that
module's docstring, none is measured).

Every case has B = 2, H = 3 (so bh / H, bh % H and the [B*H][T] layout of lse and delta matter) and
different data in every (batch, head). Inputs and outputs sit in guard-banded buffers; outputs are
pre-filled with NaN poison. The backward kernels are handed the forward REFERENCE's rounded out
and lse, so a forward fault can neither mask nor fake a backward one. Input families (kr.attn_inputs):
onehot and counting are exact or near exact and catch a dropped, doubled or misaddressed key, query,
head or batch at any bound; negative catches an unmasked padded key; normal is the regime of the
older tests; peaked spreads probabilities over > 2^30 and the row maxima over all tiles (the online
rescale). Sequence lengths: both edges (full last subtile, one valid key in it) of every template
instantiation, T < 16, and T on both sides of every tile boundary of the tiled kernels."""
import functools

import pytest
import torch

import kernel_ref as kr

pytestmark = pytest.mark.gpu

from pytorch_distributed_template_amd.ops import native_ops as no  # noqa: E402

DEV = torch.device("cuda")
BF, F32 = torch.bfloat16, torch.float32
B, H, SCALE = kr.ATTN_B, kr.ATTN_H, kr.ATTN_SCALE
FOUR = ("onehot", "counting", "negative", "normal")
FIVE = kr.ATTN_FAMILIES


_device_error = []  # a launch or synchronize that raised: nothing more is launched after it


def G(shape, dtype, fill=None):
    assert not _device_error, f"an earlier case left a device error: {_device_error[0]}"
    return kr.guarded(shape, dtype, DEV, fill)


def done(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError:
        _device_error.append(what)
        raise
    kr.check_guards(what)


@functools.lru_cache(maxsize=None)
def case(family, T):
    """(inputs, forward reference, its out as bf16, its lse as fp32): computed once per (family, T),
    shared by every test, never modified."""
    inp = kr.attn_inputs(family, B, T, H, kr.attn_seed(family, T), DEV)
    fwd = kr.attn_fwd_ref(inp["qkv"], H, SCALE)
    return inp, fwd, fwd["out"].to(BF), fwd["lse"].to(F32)


@functools.lru_cache(maxsize=None)
def bwd_case(family, T):
    inp, _, out_r, lse_r = case(family, T)
    return kr.attn_bwd_ref(inp["qkv"], out_r, inp["dout"], lse_r, H, SCALE)


class tiled:
    """pdt_attn_set_tiled(on) for the block, 0 after it."""

    def __init__(self, on):
        self.on = int(on)

    def __enter__(self):
        no._load().pdt_attn_set_tiled(self.on)

    def __exit__(self, *exc):
        no._load().pdt_attn_set_tiled(0)


def run_fwd(entry, family, T):
    inp, fwd, _, _ = case(family, T)
    qkv = G(inp["qkv"].shape, BF, inp["qkv"])
    out, lse = G((B, T, H * 64), BF), G((B * H, T), F32)
    what = f"{entry} {family} T={T}"
    no._chk(getattr(no._load(), entry)(no._p(qkv), no._p(out), no._p(lse), B, T, H, SCALE, no._s()), what)
    done(what)
    kr.attn_check_fwd(inp, fwd, out, lse, H, what)


def run_bwd(family, T, with_delta):
    inp, _, out_r, lse_r = case(family, T)
    qkv, dout = G(inp["qkv"].shape, BF, inp["qkv"]), G(inp["dout"].shape, BF, inp["dout"])
    out, lse = G(out_r.shape, BF, out_r), G(lse_r.shape, F32, lse_r)
    delta, dqkv = G((B * H, T), F32), G(inp["qkv"].shape, BF)
    what = f"pdt_attn_bwd {family} T={T}"
    no._chk(no._load().pdt_attn_bwd(no._p(qkv), no._p(out), no._p(dout), no._p(lse), no._p(delta), no._p(dqkv),
                                    B, T, H, SCALE, no._s()), what)
    done(what)
    kr.attn_check_bwd(inp, bwd_case(family, T), dqkv, H, what, delta if with_delta else None)


# ------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("family", FOUR)
@pytest.mark.parametrize("T", kr.ATTN_T_FWD_SEQ)
def test_fwd_whole_sequence(T, family):
    """attn_fwd_seq_kernel<NT>, NT = 1..16, at T = 16 NT and 16 NT - 15, and T = 5, 197. The padded
    subtile of odd NT is forced to -inf; only the last real subtile is masked by key index."""
    run_fwd("pdt_attn_fwd", family, T)


@pytest.mark.parametrize("family", FOUR)
@pytest.mark.parametrize("T", kr.ATTN_T_TILES)
def test_fwd_tiles32(T, family):
    """attn_fwd_f8_kernel<NKT, false> (the default forward), NKT = 1..8 at T = 32 NKT and 32 NKT - 31,
    and T = 197: online softmax over 32-key tiles."""
    run_fwd("pdt_attn_fwd_tiles", family, T)


@pytest.mark.parametrize("family", FIVE)
@pytest.mark.parametrize("T", kr.ATTN_T_TILED)
def test_fwd_tiled_as_dispatched(T, family):
    """attn_fwd_kernel (64-key tiles, online rescale) at the lengths that reach it by themselves."""
    run_fwd("pdt_attn_fwd", family, T)


@pytest.mark.parametrize("family", FIVE)
@pytest.mark.parametrize("T", kr.ATTN_T_TILED_FORCED)
def test_fwd_tiled_forced(T, family):
    """attn_fwd_kernel at small T through pdt_attn_set_tiled(1): one key, one key short of a tile, a
    full tile, one key into the second and the third."""
    with tiled(1):
        run_fwd("pdt_attn_fwd", family, T)


# ------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("family", FIVE)
@pytest.mark.parametrize("T", kr.ATTN_T_BWD_SEQ)
@pytest.mark.parametrize("single", [1, 0])
def test_bwd_whole_sequence(single, T, family):
    """attn_bwd_dkdv_seq_kernel / attn_bwd_dq_seq_kernel <NT, SINGLE> for both stagings (single: the
    row images serve the transposed reads; 0: separate transposed images), NT in {1, 2, 7, 8, 9, 13,
    16} at both edge T (the subtile loops stride by 8 waves: 8 and 9 are the wrap), and T = 5."""
    lib = no._load()
    lib.pdt_attn_set_bwd_single(single)
    try:
        run_bwd(family, T, with_delta=False)
    finally:
        lib.pdt_attn_set_bwd_single(1)


@pytest.mark.parametrize("family", FIVE)
@pytest.mark.parametrize("T", kr.ATTN_T_TILED + kr.ATTN_T_TILED_FORCED)
def test_bwd_tiled(T, family):
    """attn_delta_kernel, attn_bwd_dkdv_kernel and attn_bwd_dq_kernel: d(qkv) and delta."""
    with tiled(T <= 256):
        run_bwd(family, T, with_delta=True)


def test_bwd_q8_refuses_the_tiled_path():
    """pdt_attn_bwd_q8 has whole-sequence kernels only: -1 while the tiled path is forced, before
    anything is launched or written."""
    T = 16
    inp, _, out_r, lse_r = case("normal", T)
    delta, dqkv = G((B * H, T), F32), G(inp["qkv"].shape, BF)
    codes, meta, part, dq = G((B * T, 3 * H * 64), torch.uint8), G(21, F32, 1.0), G(2 * B * H, F32), G(1, F32)
    with tiled(1):
        rc = no._load().pdt_attn_bwd_q8(no._p(inp["qkv"]), no._p(out_r), no._p(inp["dout"]), no._p(lse_r),
                                        no._p(delta), no._p(dqkv), B, T, H, SCALE, no._p(codes), no._p(meta),
                                        no._p(part), no._p(dq), no._s())
    assert rc == -1
    torch.cuda.synchronize()
    assert bool(torch.isnan(dqkv.float()).all()) and bool((codes == kr.POISON_BYTE).all())
    done("pdt_attn_bwd_q8 tiled")


# --------------------------------------------------------------------------- class token
@pytest.mark.parametrize("family", ("onehot", "onehot0") + FOUR[1:])
@pytest.mark.parametrize("T", kr.ATTN_T_CLS)
def test_cls_attention(T, family):
    """pdt_cls_attn_fwd / pdt_cls_attn_bwd at the edges of the 32-token pass. onehot: query 0 selects
    key T - 1, onehot0: key 0. dq of every token but 0 must be exactly 0 and written."""
    lib = no._load()
    inp = kr.attn_inputs(family, B, T, H, kr.attn_seed(family, T), DEV)
    ref = kr.attn_cls_ref(inp["qkv"], H)
    what = f"cls {family} T={T}"
    qkv = G(inp["qkv"].shape, BF, inp["qkv"])
    out, lse = G((B, H * 64), BF), G(B * H, F32)
    no._chk(lib.pdt_cls_attn_fwd(no._p(qkv), no._p(out), no._p(lse), B, T, H, no._s()), what)
    done(what)
    kr.attn_check_cls_fwd(inp, ref, out, lse, H, what)
    o_r, lse_r = ref["out"].to(BF), ref["lse"].to(F32)
    do = inp["dout"][:, 0].contiguous()
    bref = kr.attn_cls_ref(inp["qkv"], H, do, o_r, lse_r)
    o_g, lse_g, do_g = G(o_r.shape, BF, o_r), G(lse_r.shape, F32, lse_r), G(do.shape, BF, do)
    dqkv = G(inp["qkv"].shape, BF)
    no._chk(lib.pdt_cls_attn_bwd(no._p(qkv), no._p(o_g), no._p(do_g), no._p(lse_g), no._p(dqkv), B, T, H, no._s()),
            what + " bwd")
    done(what + " bwd")
    kr.attn_check_cls_bwd(inp, bref, dqkv, H, what + " bwd")


# ---------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("T", [197, 257])
def test_qkv_attention_autograd(T):
    """no.qkv_attention(...).backward, one case per path (T = 197: the 32-key-tile forward and the
    whole-sequence backward; 257: the tiled kernels): the forward within the forward bounds, the
    backward against attn_bwd_ref evaluated on the kernel's OWN out and lse -- the autograd wrapper
    hands the kernels what they expect."""
    assert not _device_error, f"an earlier case left a device error: {_device_error[0]}"
    inp, fwd, _, _ = case("normal", T)
    x = inp["qkv"].clone().requires_grad_(True)
    out = no.qkv_attention(x, H)
    saved = out.grad_fn.saved_tensors
    lse = saved[2]
    assert lse.shape == (B * H, T) and lse.dtype == F32
    out.backward(inp["dout"])
    torch.cuda.synchronize()
    kr.attn_check_fwd(inp, fwd, out.detach(), lse, H, f"qkv_attention T={T}")
    bref = kr.attn_bwd_ref(inp["qkv"], out.detach(), inp["dout"], lse, H, SCALE)
    kr.attn_check_bwd(inp, bref, x.grad, H, f"qkv_attention.backward T={T}")
