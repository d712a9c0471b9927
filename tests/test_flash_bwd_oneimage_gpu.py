"""Flash backward with ONE row-major LDS image per tile, read transposed in
hardware, and pass 1's three-deep ring (needs MI355X).

Comparison and bounds as in test_attention_bwd_tiles_gpu.py: elementwise
against the float64 reference of attn_refs.py, inputs with the +-64 sentinels
of make_tile_inputs. What the cases straddle:
  * the ring shorter than, and exactly, its depth: pass 1 runs G * nq steps
    per workgroup (G = Hq / Hk q heads, nq = ceil(S / 32) steps each), here
    1, 2, 3, 4 in one head and 2 across a head seam;
  * a head seam inside the ring: the last step of head g and the first of
    g + 1 in flight together;
  * rows past S - 1 of a step's image, which now hold a copy of row S - 1
    (dO = +-64 there) instead of zeros: one such row (S 127, 383) and 31
    (S 97). dk and dv must not see them;
  * no scratch besides the row constants: the same bits from two calls, and
    from a call right after a large one;
  * the ROPE instantiations, one causal case per head dim.
"""
import pytest
import torch

from attn_bwd_tile_cases import make_tile_inputs
from attn_refs import (_c, attention_ref, case_id, case_scale,
                       check_attention, make_inputs, make_rope_tables)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"

RING_CASES = [_c(S, D, (4, 4), False)
              for D in (128, 64) for S in (31, 33, 65, 97)]
RING_CASES += [_c(31, D, (8, 4), False) for D in (128, 64)]
SEAM_CASES = [_c(129, D, (6, 2), True) for D in (128, 64)]
CLAMP_CASES = [_c(S, D, (6, 2), causal)
               for D in (128, 64)
               for S, causal in ((127, True), (383, True), (97, False),
                                 (97, True))]


def _fwd_bwd(c, inputs):
    q, k, v, do, mask = inputs
    scale = case_scale(c)
    e = get_ext(required=True)
    out, lse = e.flash_attn_fwd(q, k, v, c["causal"], scale, mask)
    dq, dk, dv = e.flash_attn_bwd(q, k, v, do, out, lse, c["causal"], scale,
                                  mask)
    return out, lse, dq, dk, dv


def _check(c):
    inputs = make_tile_inputs(c, DEV)
    q, k, v, do, mask = inputs
    ref = attention_ref(q, k, v, c["causal"], case_scale(c), mask, do)
    out, lse, dq, dk, dv = _fwd_bwd(c, inputs)
    check_attention(dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv), ref,
                    case_id(c))


@pytest.mark.parametrize("c", RING_CASES, ids=case_id)
def test_ring_shorter_than_and_exactly_its_depth(c):
    _check(c)


@pytest.mark.parametrize("c", SEAM_CASES, ids=case_id)
def test_head_seam_inside_the_ring(c):
    _check(c)


@pytest.mark.parametrize("c", CLAMP_CASES, ids=case_id)
def test_rows_past_the_end_repeat_the_last_row_unseen(c):
    S = c["S"]
    inputs = make_tile_inputs(c, DEV)
    # the sentinels the clamped rows would carry into dV / dK are there
    assert inputs[3][:, S - 1].abs().min().item() == 64.0
    assert inputs[2][:, S - 1].abs().min().item() == 64.0
    _check(c)


@pytest.mark.parametrize("D", (128, 64))
def test_same_bits_twice_and_after_a_large_call(D):
    small = _c(129, D, (6, 2), True)
    large = _c(513, D, (6, 2), True)
    s_in = make_tile_inputs(small, DEV)
    alone = _fwd_bwd(small, s_in)
    again = _fwd_bwd(small, s_in)
    for x, y in zip(alone[2:], again[2:]):
        assert torch.equal(x, y)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    l_in = make_inputs(large, DEV)
    # NaN-free but huge values everywhere a stale read could land
    big = _fwd_bwd(large, tuple(t if i == 4 or t is None else t * 64
                                for i, t in enumerate(l_in)))
    del big
    after = _fwd_bwd(small, s_in)
    for x, y in zip(alone[2:], after[2:]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("c", [_c(161, 128, (6, 2), True),
                               _c(97, 64, (8, 4), True)], ids=case_id)
def test_rope_instantiations(c):
    from test_flash_bwd_rope_gpu import _check_routes
    cos, sin = make_rope_tables(c["S"], c["D"], 3, device=DEV)
    _check_routes(c, make_tile_inputs(c, DEV), cos, sin, case_id(c))
