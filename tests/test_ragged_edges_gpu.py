"""Ragged decode HIP kernel at its split-KV, length and contract edges (needs
MI355X). Elementwise against attn_refs.ragged_ref (float64, derived bound).
Both pools are NaN at every position >= len and in every slot `rows` does
not name, so any read past a length fails the comparison; V carries the
sentinel 64 at position len - 1, so a dropped last position does too."""
import pytest
import torch

from attn_refs import (RAGGED_CHUNKS, RAGGED_DUP, RAGGED_LENS_A,
                       RAGGED_LENS_B, RAGGED_SHAPES, make_ragged, ragged_ref)
from edge_refs import assert_within

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF = torch.bfloat16
N_SLOTS, SMAX = 14, 300


def _ext():
    return get_ext(required=True)


@pytest.mark.parametrize("G,D,Hk", RAGGED_SHAPES)
def test_ragged_decode_vs_float64(G, D, Hk):
    """chunk = 4 with lens <= 37 gives multi-chunk rows, empty chunks and
    NS = 10; adding a 257 caps NS at 64 (eff_chunk 8); 512 is one chunk."""
    for lens in (RAGGED_LENS_A, RAGGED_LENS_B):
        q, kp, vp, rows, ln = make_ragged(lens, RAGGED_DUP, G, D, Hk,
                                          N_SLOTS, SMAX, DEV)
        assert rows[RAGGED_DUP[0]] == rows[RAGGED_DUP[1]]
        ref = ragged_ref(q, kp, vp, rows, ln)
        for chunk in RAGGED_CHUNKS:
            out = _ext().ragged_decode(q, kp, vp, rows, ln, chunk)
            assert_within(out, ref["out"], ref["tol"],
                          f"n={len(lens)} chunk={chunk}")


@pytest.mark.parametrize("chunk", RAGGED_CHUNKS)
def test_ragged_decode_empty_row_is_zero(chunk):
    lens = [0, 9, 0, 37, 5]
    q, kp, vp, rows, ln = make_ragged(lens, (4, 1), 4, 128, 2, N_SLOTS,
                                      SMAX, DEV)
    ref = ragged_ref(q, kp, vp, rows, ln)
    out = _ext().ragged_decode(q, kp, vp, rows, ln, chunk)
    assert_within(out, ref["out"], ref["tol"], f"chunk={chunk}")
    for i in (0, 2):
        assert torch.count_nonzero(out[i].float()) == 0


def test_ragged_decode_rejects_bad_arguments():
    """Pools are leading views of larger buffers and every bad tensor is at
    least as large as the good one: indexing would stay in allocated memory
    even without the checks."""
    e = _ext()
    n, Hk, G, D, B, Smax = 3, 2, 2, 64, 4, 16
    Hq = Hk * G
    kbuf = torch.zeros(B + 2, Smax, Hk, D, device=DEV, dtype=BF)
    vbuf = torch.zeros(B + 2, Smax, Hk, D, device=DEV, dtype=BF)
    kp, vp = kbuf[:B], vbuf[:B]
    assert kp.is_contiguous()
    q = torch.zeros(n, 1, Hq, D, device=DEV, dtype=BF)
    rows = torch.tensor([2, 0, 1], device=DEV)
    lens = torch.tensor([5, 16, 1], device=DEV)
    e.ragged_decode(q, kp, vp, rows, lens, 4)               # the good call
    q3 = torch.zeros(n, 1, 3, D, device=DEV, dtype=BF)
    k1 = torch.zeros(B + 2, Smax, 1, 3 * D, device=DEV, dtype=BF)[:B]
    bad = {
        "lens.max() == 0": lambda: e.ragged_decode(
            q, kp, vp, rows, torch.zeros_like(lens), 4),
        "lens.max() > Smax": lambda: e.ragged_decode(
            q, kp, vp, rows, torch.tensor([5, Smax + 1, 1], device=DEV), 4),
        "chunk 0": lambda: e.ragged_decode(q, kp, vp, rows, lens, 0),
        "chunk -4": lambda: e.ragged_decode(q, kp, vp, rows, lens, -4),
        "G = 3": lambda: e.ragged_decode(q3, k1[..., :D].contiguous(),
                                         k1[..., :D].contiguous(), rows,
                                         lens, 4),
        "vpool shape": lambda: e.ragged_decode(q, kp, vbuf, rows, lens, 4),
        "pool head_dim": lambda: e.ragged_decode(
            q, torch.zeros(B, Smax, Hk, 2 * D, device=DEV, dtype=BF),
            torch.zeros(B, Smax, Hk, 2 * D, device=DEV, dtype=BF), rows,
            lens, 4),
        "kpool dtype": lambda: e.ragged_decode(q, kp.float(), vp, rows,
                                               lens, 4),
        "vpool dtype": lambda: e.ragged_decode(q, kp, vp.float(), rows,
                                               lens, 4),
        "rows int32": lambda: e.ragged_decode(q, kp, vp, rows.int(), lens, 4),
        "lens int32": lambda: e.ragged_decode(q, kp, vp, rows, lens.int(), 4),
        "lens length": lambda: e.ragged_decode(
            q, kp, vp, rows, torch.tensor([5, 16, 1, 1], device=DEV), 4),
        "rows length": lambda: e.ragged_decode(
            q, kp, vp, torch.tensor([2, 0, 1, 1], device=DEV), lens, 4),
        "rows strided": lambda: e.ragged_decode(
            q, kp, vp, torch.zeros(2 * n, dtype=torch.long,
                                   device=DEV)[::2], lens, 4),
        "rows device": lambda: e.ragged_decode(q, kp, vp, rows.cpu(), lens,
                                               4),
        "lens device": lambda: e.ragged_decode(q, kp, vp, rows, lens.cpu(),
                                               4),
    }
    for name, call in bad.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"'{name}' did not raise")
