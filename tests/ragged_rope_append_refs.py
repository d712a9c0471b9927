"""float64 reference, batches and checks shared by the ragged_rope_append
tests (CPU fallback and HIP kernel).

Reference, per (d, d + D/2) pair of a token at table row p:
    r1 = a*c - b*s,  r2 = b*c + a*s
with a, b the STORED input values and c, s the fp32 table entries, all widened
to float64. An fp32 evaluation is two product roundings plus one sum rounding
(or one FMA and one product), so it is off by at most
    3 * U24 * (|a*c| + |b*s|)       (resp. |b*c| + |a*s|);
a bf16 result adds one RNE rounding, BF16_ULP * |ref| (edge_refs.bf16_tol).
V is a copy and must be bit-exact.
"""
import torch

from edge_refs import BF16_ULP, U24, assert_within

# (slot, q_start, q_len, kv_len) per total token count T; q_start order and
# list order are both shuffled, slot 0 / slot B-1 and position 0 / Smax-1 are
# used, and multi-token chunks sit next to single-token decode rows.
POOL = {1: (4, 16, 32), 7: (4, 16, 32), 300: (8, 64, 64)}   # T -> B, Smax, P
SEQS = {
    7: [(2, 5, 2, 9), (3, 0, 1, 16), (0, 1, 3, 3), (1, 4, 1, 5)],
    300: [(3, 114, 60, 60), (0, 0, 64, 64), (5, 174, 1, 33),
          (7, 64, 50, 64), (2, 299, 1, 1), (6, 236, 63, 63),
          (1, 175, 61, 62)],
}
# T = 1 cannot touch both ends at once: two single-token batches
SEQS_T1 = [[(3, 0, 1, 16)], [(0, 0, 1, 1)]]

# skip rule: B = 6, Smax = 16, P = 32, T = 12; `SKIP_EDITS` overwrite one
# index of one token each with an out-of-range value
SKIP_POOL = (6, 16, 32)
SKIP_SEQS = [(3, 0, 1, 16), (0, 1, 3, 3), (1, 4, 1, 5), (2, 5, 3, 9),
             (4, 8, 3, 6), (5, 11, 1, 10)]
SKIP_EDITS = [("slot", 0, -1), ("pos", 2, -1), ("slot", 4, 6),
              ("pos", 7, 16), ("pos", 8, 32)]
SKIP_BAD = [0, 2, 4, 7, 8]
# slots whose last token is still valid: 0 (t=3), 4 (t=10), 5 (t=11)
SKIP_LENS = {0: 3, 4: 6, 5: 10}


def pattern(shape, dtype, device, salt=0):
    """Non-constant, NaN-free fill; every value is exact in bf16."""
    n = 1
    for s in shape:
        n *= s
    v = ((torch.arange(n, dtype=torch.float32) * 7 + salt) % 251 - 125) / 8
    return v.reshape(shape).to(dtype).to(device)


def make_inputs(T, Hq, Hk, D, P, dtype, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn(T, Hq, D, generator=g) * 2).to(dtype).to(device)
    k = (torch.randn(T, Hk, D, generator=g) * 2).to(dtype).to(device)
    v = (torch.randn(T, Hk, D, generator=g) * 2).to(dtype).to(device)
    # any fp32 values serve as a table; a real one keeps |c|,|s| <= 1
    ang = torch.rand(P, D // 2, generator=g) * 6.2831853
    return q, k, v, ang.cos().to(device), ang.sin().to(device)


def rope_ref(x, cos, sin, pos):
    """x [T,H,D], pos [T] (in range) -> float64 (ref, slack) [T,H,D]."""
    half = x.shape[-1] // 2
    x = x.double().cpu()
    c = cos.double().cpu()[pos.cpu()].unsqueeze(1)
    s = sin.double().cpu()[pos.cpu()].unsqueeze(1)
    a, b = x[..., :half], x[..., half:]
    ref = torch.cat([a * c - b * s, b * c + a * s], dim=-1)
    slack = 3 * U24 * torch.cat([(a * c).abs() + (b * s).abs(),
                                 (b * c).abs() + (a * s).abs()], dim=-1)
    return ref, slack


def bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def check_call(q_rot, q, k, v, cos, sin, tok_slot, tok_pos, kpool, vpool,
               kpool0, vpool0, lens, lens0, what):
    """Everything one ragged_rope_append call promises, for any index
    content: `kpool0`/`vpool0`/`lens0` are copies from before the call."""
    B, Smax = kpool.shape[0], kpool.shape[1]
    P = cos.shape[0]
    slot, pos = tok_slot.cpu(), tok_pos.cpu()
    T = slot.numel()
    ok = (slot >= 0) & (slot < B) & (pos >= 0) & (pos < min(Smax, P))
    keep = ok.nonzero().squeeze(1)
    ulp = BF16_ULP if q.dtype == torch.bfloat16 else 0.0
    assert q_rot.shape == q.shape and q_rot.dtype == q.dtype

    ref, slack = rope_ref(q.cpu()[keep], cos, sin, pos[keep])
    assert_within(q_rot.cpu()[keep], ref, ulp * ref.abs() + slack,
                  f"{what} q_rot")
    assert not q_rot.cpu()[~ok].double().abs().any(), \
        f"{what}: q_rot rows of skipped tokens are not zero"

    ref, slack = rope_ref(k.cpu()[keep], cos, sin, pos[keep])
    assert_within(kpool.cpu()[slot[keep], pos[keep]], ref,
                  ulp * ref.abs() + slack, f"{what} kpool rows")
    assert torch.equal(bits(vpool.cpu()[slot[keep], pos[keep]]),
                       bits(v.cpu()[keep])), f"{what}: V rows not bit-exact"

    named = torch.zeros(B, Smax, dtype=torch.bool)
    named[slot[keep], pos[keep]] = True
    for name, got, before in (("kpool", kpool, kpool0),
                              ("vpool", vpool, vpool0)):
        assert torch.equal(bits(got.cpu()[~named]),
                           bits(before.cpu()[~named])), \
            f"{what}: {name} changed outside the rows the batch names"

    if lens is not None:
        # last token of its sequence: followed by another slot or by nothing
        last = torch.ones(T, dtype=torch.bool)
        last[:-1] = slot[1:] != slot[:-1]
        sel = ok & last
        want = lens0.cpu().clone()
        want[slot[sel]] = pos[sel] + 1
        assert torch.equal(lens.cpu(), want), \
            f"{what}: lens {lens.tolist()} want {want.tolist()}"
