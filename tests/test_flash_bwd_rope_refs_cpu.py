"""The bound of attn_refs.py for the un-rotated dq / dk (flash backward given
cos / sin tables) is VALID and SHARP on every case of the GPU test
test_flash_bwd_rope_gpu.py: the emulated fused route (the fp32 accumulators
of test_attention_refs_cpu.emulate_attention, un-rotated in fp32, rounded to
bf16 once) stays inside it, and the same route with one edge of the
un-rotation broken does not. Runs without a GPU."""
import pytest
import torch

from attn_bwd_tile_cases import TILE_CASES, make_tile_inputs
from attn_refs import (ATTN_CASES, attention_ref, case_id, case_scale,
                       make_inputs, make_rope_tables, unrotated_grads)
from edge_refs import assert_within
from test_attention_refs_cpu import emulate_attention

BF = torch.bfloat16
EXTRA = 3

# (case, how its inputs are made): the cases of the GPU test, in its order
ROPE_BWD_CASES = [(c, make_inputs) for c in ATTN_CASES] + \
    [(c, make_tile_inputs) for c in TILE_CASES]
IDS = [("tile-" if mk is make_tile_inputs else "") + case_id(c)
       for c, mk in ROPE_BWD_CASES]


def emulate_unrotate(d32, cos, sin, mut=None, round_first=False):
    """The epilogue in plain torch: d32 [B,S,H,D] fp32 accumulators, fp32
    table, fp32 products and sum, ONE bf16 rounding. round_first: the unfused
    route instead (bf16 gradient, then the rope kernel: two roundings)."""
    S, D = d32.shape[1], d32.shape[3]
    half = D // 2
    if round_first:
        d32 = d32.to(BF).float()
    if mut == "skipped":
        return d32.to(BF)
    r0 = 1 if mut == "row_plus_1" else 0
    c, s = cos[r0:r0 + S], sin[r0:r0 + S]
    if mut == "column_plus_4":          # one lane's l4 group of 4 columns
        c, s = c.roll(-4, 1), s.roll(-4, 1)
    if mut == "forward":
        s = -s
    c, s = c.reshape(1, S, 1, half), s.reshape(1, S, 1, half)
    d1, d2 = d32[..., :half], d32[..., half:]
    return torch.cat([d1 * c + d2 * s, d2 * c - d1 * s], -1).to(BF)


MUTANTS = ["forward", "row_plus_1", "column_plus_4", "skipped"]

_CACHE = {}


def _case(i):
    """Inputs, the emulation's fp32 dq / dk, the un-rotated reference, and
    the table without its NaN rows (the row_plus_1 mutant reads row S)."""
    if i not in _CACHE:
        c, mk = ROPE_BWD_CASES[i]
        q, k, v, do, mask = mk(c)
        scale = case_scale(c)
        ref = attention_ref(q, k, v, c["causal"], scale, mask, do)
        cos, sin = make_rope_tables(c["S"], c["D"], EXTRA, poison=False)
        un = unrotated_grads(ref, cos, sin)
        emu = emulate_attention(q, k, v, c["causal"], scale, mask, do,
                                fp32_grads=True)
        _CACHE[i] = (emu["dq32"], emu["dk32"], un, cos, sin)
    return _CACHE[i]


def test_poisoned_and_plain_tables_agree_below_S():
    a = make_rope_tables(33, 64, EXTRA, poison=True)
    b = make_rope_tables(33, 64, EXTRA, poison=False)
    for x, y in zip(a, b):
        assert x.shape == (36, 32) and x.dtype == torch.float32
        assert x.is_contiguous() and torch.equal(x[:33], y[:33])
        assert torch.isnan(x[33:]).all() and not torch.isnan(y).any()
    # cos^2 + sin^2 = 1 to fp32 rounding: the pair is one angle's
    assert ((b[0].double() ** 2 + b[1].double() ** 2 - 1).abs() < 1e-6).all()


@pytest.mark.parametrize("i", range(len(ROPE_BWD_CASES)), ids=IDS)
def test_emulated_fused_route_within_bound(i):
    dq32, dk32, un, cos, sin = _case(i)
    for name, d32 in (("dq", dq32), ("dk", dk32)):
        assert not torch.isnan(un[name]).any()
        got = emulate_unrotate(d32, cos, sin)
        assert_within(got, un[name], un[name + "_tol"], f"{IDS[i]} {name}")
        # the unfused route (two roundings) is inside the bound as well
        two = emulate_unrotate(d32, cos, sin, round_first=True)
        assert_within(two, un[name], un[name + "_tol"],
                      f"{IDS[i]} {name} unfused")


def test_peak_share_of_the_bound():
    """How far inside the bound the faithful emulation sits (printed)."""
    peak = 0.0
    for i in range(len(ROPE_BWD_CASES)):
        dq32, dk32, un, cos, sin = _case(i)
        for name, d32 in (("dq", dq32), ("dk", dk32)):
            err = (emulate_unrotate(d32, cos, sin).double() - un[name]).abs()
            tol = un[name + "_tol"]
            peak = max(peak, (err[tol > 0] / tol[tol > 0]).max().item()
                       if (tol > 0).any() else 0.0)
    print(f"faithful emulation peaks at {peak:.3f} of the bound")
    assert peak <= 1.0


def test_every_present_unrotate_mutant_is_caught():
    """Accounting of test_every_present_mutant_is_caught: a (case, mutant)
    pair whose dq and dk equal the unmutated emulation's has no such edge
    (S = 1: the gradients are exactly 0); fewer than 1 pair in 20 may be
    skipped that way. On every other pair both dq and dk must be rejected."""
    pairs = skipped = 0
    missed = []
    for i in range(len(ROPE_BWD_CASES)):
        dq32, dk32, un, cos, sin = _case(i)
        base = {n: emulate_unrotate(d, cos, sin)
                for n, d in (("dq", dq32), ("dk", dk32))}
        for mut in MUTANTS:
            pairs += 1
            got = {n: emulate_unrotate(d, cos, sin, mut=mut)
                   for n, d in (("dq", dq32), ("dk", dk32))}
            if all(torch.equal(got[n], base[n]) for n in got):
                skipped += 1            # the broken edge is not in this case
                continue
            for n in got:
                try:
                    assert_within(got[n], un[n], un[n + "_tol"],
                                  f"{IDS[i]} {mut} {n}")
                except AssertionError:
                    continue
                missed.append(f"{IDS[i]}: {mut} {n}")
    print(f"un-rotation mutants: {pairs} (case, mutant) pairs, {skipped} "
          f"skipped as 'edge not present' ({100.0 * skipped / pairs:.1f} %)")
    assert not missed, "mutants inside the bound:\n" + "\n".join(missed)
    assert skipped * 20 < pairs
