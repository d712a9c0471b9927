"""Flash forward with ONE row-major LDS image of V per tile, read transposed
in hardware, and K / V in a two-deep ring with one barrier per tile (needs
MI355X).

`out` and `lse` elementwise against the float64 reference and the derived
bounds of attn_refs.py (check_attention(..., backward=False)), inputs from
make_inputs with its +-64 sentinels. Nothing here is tuned. What the cases
straddle:
  * the ring shorter than, equal to and longer than its depth: 1, 2, 3, 4 and
    5 kv tiles of 64 inside one 256-row q block;
  * image rows past S - 1, which now hold a copy of row S - 1 (V = +-64
    there) instead of zeros: one such row (S 127, 191) and 63 (S 65, 193).
    Their P is exactly 0, so `out` and `lse` must not see them;
  * nothing past q, k, v is read: the tensors are prefixes of allocations
    whose tails are NaN for more than a 64-row tile;
  * several q blocks (the ring restarts per block; any dispatch order);
  * kv masks that empty whole tiles of the ring;
  * no state between calls: the same bits from two calls, and from a call
    right after a large one;
  * the training path: rope_flash_attention through autograd, and the fused
    backward routes on the forward's out / lse, one case per head dim.
"""
import pytest
import torch

from attn_refs import (_c, attention_ref, case_id, case_scale,
                       check_attention, make_inputs, make_rope_tables)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
DIMS = (128, 64)

RING_CASES = [_c(S, D, H, causal)
              for D in DIMS for H in ((4, 4), (6, 2))
              for S in (33, 65, 129, 193, 257) for causal in (True, False)]
CLAMP_CASES = [_c(S, D, (6, 2), causal)
               for D in DIMS for S in (127, 65, 193, 191)
               for causal in (True, False)]
POISON_CASES = [_c(S, D, (6, 2), True) for D in DIMS for S in (65, 127)]
BLOCK_CASES = [_c(S, D, H, True)
               for S in (513, 577) for D, H in ((128, (4, 1)), (64, (6, 2)))]
MASK_CASES = [c for D, H in ((128, (6, 2)), (64, (4, 1))) for c in (
    _c(193, D, H, False, mask="left", arg=130),
    _c(193, D, H, True, mask="tail", arg=64),
    _c(129, D, H, True, mask="full"),
    _c(257, D, H, False, mask="min_left", arg=64))]


def _fwd(c, inputs):
    q, k, v, _, mask = inputs
    return get_ext(required=True).flash_attn_fwd(q, k, v, c["causal"],
                                                 case_scale(c), mask)


def _check(c, inputs=None):
    inputs = make_inputs(c, DEV) if inputs is None else inputs
    q, k, v, _, mask = inputs
    ref = attention_ref(q, k, v, c["causal"], case_scale(c), mask)
    out, lse = _fwd(c, inputs)
    assert not torch.isnan(out.float()).any(), "out: NaN"
    check_attention(dict(out=out, lse=lse), ref, case_id(c), backward=False)
    return out, lse


@pytest.mark.parametrize("c", RING_CASES, ids=case_id)
def test_ring_shorter_than_equal_to_and_longer_than_its_depth(c):
    _check(c)


@pytest.mark.parametrize("c", CLAMP_CASES, ids=case_id)
def test_rows_past_the_end_hold_the_last_row_unseen(c):
    S = c["S"]
    inputs = make_inputs(c, DEV)
    # the sentinel the clamped rows would carry into out is there
    assert inputs[2][:, S - 1].abs().min().item() == 64.0
    _check(c, inputs)


def _prefix_of_poisoned(t, tail_rows):
    """t [B,S,H,D] as the contiguous prefix of one allocation whose tail,
    tail_rows more [H,D] rows, is NaN."""
    B, S, H, D = t.shape
    buf = torch.full(((B * S + tail_rows) * H * D,), float("nan"),
                     device=t.device, dtype=t.dtype)
    view = buf[:t.numel()].view(B, S, H, D)
    view.copy_(t)
    return view, buf


@pytest.mark.parametrize("c", POISON_CASES, ids=case_id)
def test_nothing_past_the_tensors_is_read(c):
    q, k, v, do, mask = make_inputs(c, DEV)
    keep = []
    views = []
    for t in (q, k, v):
        view, buf = _prefix_of_poisoned(t, 64 + 8)   # more than one kv tile
        assert torch.isnan(buf[t.numel():].float()).all()
        views.append(view)
        keep.append(buf)
    # the last batch row is the one whose over-read would land in the NaNs
    out, lse = _check(c, (views[0], views[1], views[2], do, mask))
    assert not torch.isnan(out[-1].float()).any()
    assert not torch.isnan(lse[-1]).any()


@pytest.mark.parametrize("c", BLOCK_CASES, ids=case_id)
def test_several_q_blocks(c):
    _check(c)


@pytest.mark.parametrize("c", MASK_CASES, ids=case_id)
def test_masks_across_the_ring(c):
    out, _ = _check(c)
    if c["mask"] == "full":     # batch row 0 has no admissible column
        assert out[0].float().abs().max().item() == 0.0


@pytest.mark.parametrize("D", DIMS)
def test_same_bits_twice_and_after_a_large_call(D):
    small = _c(129, D, (6, 2), True)
    large = _c(513, D, (6, 2), True)
    s_in = make_inputs(small, DEV)
    alone = _fwd(small, s_in)
    again = _fwd(small, s_in)
    for x, y in zip(alone, again):
        assert torch.equal(x, y)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    l_in = make_inputs(large, DEV)
    # NaN-free but huge values everywhere a stale read could land
    big = _fwd(large, tuple(t if i == 4 or t is None else t * 64
                            for i, t in enumerate(l_in)))
    del big
    after = _fwd(small, s_in)
    for x, y in zip(alone, after):
        assert torch.equal(x, y)


@pytest.mark.parametrize("c", [_c(161, 128, (6, 2), True),
                               _c(97, 64, (8, 4), True)], ids=case_id)
def test_training_path(c):
    from deepspeed_amd.ops.attention import rope_flash_attention
    from test_flash_bwd_rope_gpu import _check_routes
    ext = get_ext(required=True)
    inputs = make_inputs(c, DEV)
    cos, sin = make_rope_tables(c["S"], c["D"], 3, device=DEV)
    # the backward routes consume this forward's out and lse
    _check_routes(c, inputs, cos, sin, case_id(c))

    # rope_flash_attention through autograd: the forward it runs is held to
    # the reference on the rotated q, k it attends over
    q, k, v, do, _ = inputs
    cos_s, sin_s = cos[:c["S"]].contiguous(), sin[:c["S"]].contiguous()
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = rope_flash_attention(ql, kl, vl, cos_s, sin_s, causal=True)
    assert out is not None
    qr, kr = ext.rope_qk(q, k, cos_s, sin_s)
    ref = attention_ref(qr, kr, v, True, case_scale(c))
    o2, lse = ext.flash_attn_fwd(qr, kr, v, True, case_scale(c), None)
    assert torch.equal(out.detach(), o2)
    check_attention(dict(out=out.detach(), lse=lse), ref, case_id(c),
                    backward=False)
    out.backward(do)
    for g in (ql.grad, kl.grad, vl.grad):
        assert g is not None and not torch.isnan(g.float()).any()
