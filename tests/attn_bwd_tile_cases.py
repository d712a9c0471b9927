"""Cases and sentinels for the tile geometry of the pipelined flash backward
(attention_bwd.hip), shared by the GPU test and its CPU 'teeth' test.

Geometry straddled: both passes give a workgroup 128 rows (4 waves x 32) of
the outer index and stream the other index in steps of 32; the transposed
scratch images are padded to a multiple of 128 rows and written by a
pre-pass in 64-row tiles. So with KB = 128 and QS = 32 the lengths are
KB-1, KB, KB+1, 2*KB+1, 3*KB+1, QS-1, QS+1, KB+QS+1, and 127 / 383, which
leave exactly one row in the padded scratch tail.
"""
import torch

from attn_refs import F32_MIN, SENT, _c, make_inputs

KB = 128      # keys (pass 1) / q rows (pass 2) per workgroup; scratch padding
QS = 32       # rows per streamed step, and per wave

TILE_CASES = [
    _c(31, 128, (4, 4), True), _c(33, 64, (6, 2), False),
    _c(127, 128, (6, 2), True), _c(127, 64, (4, 4), False, True),
    _c(128, 64, (8, 1), True, True), _c(128, 128, (4, 4), False),
    _c(129, 128, (8, 1), True), _c(129, 64, (6, 2), False),
    _c(161, 128, (6, 2), True, True),
    _c(257, 128, (4, 4), True), _c(257, 64, (8, 1), False),
    _c(383, 128, (6, 2), True), _c(385, 64, (8, 1), False, True),
    _c(385, 64, (4, 4), True),
    # masks ending on the new boundaries; one fully masked batch row
    _c(257, 128, (6, 2), False, mask="left", arg=128),
    _c(385, 64, (4, 4), True, mask="left", arg=129),
    _c(257, 64, (8, 1), True, mask="tail", arg=128),
    _c(385, 128, (4, 4), False, mask="tail", arg=160),
    _c(129, 128, (6, 2), True, mask="full"),
]


def boundary_points(S):
    """Both sides of every 32-row boundary below S, and the last row."""
    pts = {S - 1}
    for m in range(QS, S, QS):
        pts.update((m - 1, m))
    return sorted(p for p in pts if 0 <= p < S)


def make_tile_inputs(case, device="cpu"):
    """make_inputs plus +-64 sentinels in V (admissible keys only) and dO on
    both sides of every boundary of the backward's tiles."""
    q, k, v, do, mask = make_inputs(case, "cpu")
    S = case["S"]
    for n, j in enumerate(boundary_points(S)):
        sign = SENT * (1 - 2 * (n % 2))
        do[:, j] = sign
        for b in range(v.shape[0]):
            if mask is None or mask[b, j] > F32_MIN:
                v[b, j] = -sign
    mv = lambda t: None if t is None else t.to(device)      # noqa: E731
    return mv(q), mv(k), mv(v), mv(do), mv(mask)


def boundary_key(case, mask):
    """The highest tile-boundary key that some batch row admits and that a
    later q row still sees."""
    S = case["S"]
    for j in reversed(boundary_points(S)):
        if j == S - 1 and S > 1:
            continue
        if mask is None or bool((mask[:, j] > F32_MIN).any()):
            return j
    return S - 1


def boundary_row(case):
    """The first row of the last 32-row step; the last row where that step
    is the first one (causal row 0 sees one key, so its dS is exactly 0)."""
    S = case["S"]
    r = QS * ((S - 1) // QS)
    return r if r else S - 1
