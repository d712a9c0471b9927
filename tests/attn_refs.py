"""float64 references, derived bounds and shared cases for the attention and
ragged-decode edge tests (conventions of edge_refs.py: nothing here is tuned).

Definitions
-----------
A kv column j is ADMISSIBLE for q row i unless the causal rule (j > i)
excludes it or its additive mask value is <= finfo(float32).min. The kernels
add mask * log2(e) in fp32, where finfo.min overflows to -inf, so the HF
"min" convention and -inf mean the same thing. A row with no admissible
column is DEFINED as out = 0, dq = 0, no contribution to dk / dv, lse = -inf
(torch's softmax gives NaN there); its lse is excluded from comparison.

Bounds (unit roundoffs: fp32 U24 = 2^-24; bf16 RNE half ulp <= 2^-8 relative)
------------------------------------------------------------------------------
score  s_ij = scale * sum_d q k + mask is an fp32 sum of D exact bf16
       products, then scaled, masked, shifted by the running max and fed to a
       hardware exp. In units of U24 its absolute error is at most
         ds_ij = (D + EPI) * (scale * sum_d |q||k| + |mask_j|)
                 + 2 * (|s_ij - m_i| + 8)
       (the last term: one rounding of the subtraction and of the log2(e)
       rescaling; +8 because the deferred max may lag the true row max by 8).
row    p_ij = exp(s_ij - lse_i) inherits ds_ij and the error of the row sum
       relatively: eta_i = 2 * max_j ds_ij + (S + EPI) * U24.
out    P is rounded to bf16 before P @ V (2^-8), accumulated in fp32 over S
       keys (S * U24; D, EPI for the normalisation), so before the final bf16
       rounding (bf16_tol) it is off by at most
         (2^-8 + eta_i + (S + D + EPI) * U24) * (P @ |V|).
lse    max_j ds_ij + U24 * ((S + EPI) + C_LOG * (|lse - m| + 8)
       + 4 * (|lse| + |m|)): relative error of the sum is absolute in its
       log; native log2 and the ln 2 / log2 e conversions of m and lse.
bwd P  recomputed as exp(s - lse) from the SAVED fp32 lse:
         etab_ij = ds_ij + lse_tol_i + 4 * U24   (relative).
dV     sum over the G*S (head, q) pairs of bf16(P) * dO:
         (2^-8 + (G*S + EPI) * U24) * P^T|dO| + (etab o P)^T |dO|.
dS     = P o (dP - Drow) * scale. dP is an fp32 sum of D products
       (D * U24 * sum_d |dO||V|). Drow = sum_d dO * O uses the bf16 O the
       forward WROTE, which is off from the exact O by the forward slack plus
       its own rounding (2^-8 |O|):
         eD_i = sum_d |dO| (2^-8 |O| + slack_out) + (D + EPI) U24 sum|dO||O|.
       So  e_ij = scale * P_ij * (etab_ij |dP_ij - Drow_i| + D U24 dPabs_ij
                  + eD_i) + 3 U24 |dS_ij|,
       and after rounding dS to bf16  E_ij = (1 + 2^-8) e_ij + 2^-8 |dS_ij|.
dQ     E @ |K| + (S + EPI) * U24 * (|dS| @ |K|).
dK     sum over the group of E^T @ |Q| + (G*S + EPI) * U24 * (|dS|^T @ |Q|).
ragged fp32 throughout: with L keys, eta as above (S -> L, no +8) and
       4 * (L + D + EPI) * U24 for the accumulation (L), the chain of at most
       L online rescales (a multiply and an exp, 3 units each) and the
       split-KV combine -- all times P @ |V|, plus the final bf16 rounding.

Un-rotated dQ / dK (flash backward given cos / sin tables)
----------------------------------------------------------
q and k are then the RoPE-rotated tensors, and the epilogues return the
gradient with respect to the un-rotated ones: the inverse rotate-half
rotation at table row s, applied to the fp32 accumulators BEFORE their single
bf16 rounding. With (d1, d2) the exact gradient pair at columns (j, j + D/2),
c = cos[s, j] and s = sin[s, j] (the fp32 table values, taken to float64
exactly: kernel and reference read the same table), the reference is
         d1' = d1 c + d2 s,     d2' = d2 c - d1 s.
The kernel holds d1, d2 off by at most e1, e2 (dq_slack / dk_slack above: the
pre-rounding slack of dQ / dK) and forms both expressions in fp32: two
products and one sum, 3 roundings of at most U24 each relative to
|c||d1| + |s||d2| (a fused multiply-add only drops one of them). So before the
final rounding
         slack1' = |c| e1 + |s| e2 + 3 U24 (|c||d1| + |s||d2|)
         slack2' = |c| e2 + |s| e1 + 3 U24 (|c||d2| + |s||d1|)
and tol' = bf16_tol(ref', slack'). Nothing here is tuned. The unfused route
(bf16 dQ, then the rope kernel: two roundings) is NOT a mutant of this bound:
its extra rounding (2^-8 |d1|, 2^-8 |d2| before the rotation) is of the order
of the allowance 2^-7 |ref'| for the final one, and the emulated unfused
route lies inside on every shared case (test_flash_bwd_rope_refs_cpu.py
checks that too), so no test asserts that it falls outside.
"""
import math

import torch

from edge_refs import BF16_ULP, C_LOG, EPI, U24, assert_within, bf16_tol

HALF_BF16 = 2.0 ** -8     # RNE: half a bf16 ulp, relative
F32_MIN = torch.finfo(torch.float32).min
SENT = 64.0               # V / dO sentinel magnitude
MASKED_V = 1000.0         # V on every inadmissible (-inf / min masked) column


# ------------------------------------------------------------- reference
def _heads(t):            # [B,S,H,D] -> [B,H,S,D] float64
    return t.double().permute(0, 2, 1, 3)


def attention_ref(q, k, v, causal, scale, kvmask=None, dout=None):
    """All float64, closed form. q [B,S,Hq,D], k/v [B,S,Hk,D], kvmask [B,S]
    additive or None, dout [B,S,Hq,D] or None. Returns a dict of references
    in the kernels' layouts (out/dq [B,S,Hq,D], dk/dv [B,S,Hk,D],
    lse [B,Hq,S]), the condition terms and the tolerances derived above;
    dq_slack / dk_slack are the pre-rounding parts of dq_tol / dk_tol."""
    B, S, Hq, D = q.shape
    Hk = k.shape[2]
    G = Hq // Hk
    dev = q.device
    hmap = torch.arange(Hq, device=dev) // G
    qd, kd, vd = _heads(q), _heads(k)[:, hmap], _heads(v)[:, hmap]
    s = qd @ kd.transpose(-1, -2) * scale
    s_abs = qd.abs() @ kd.abs().transpose(-1, -2) * scale   # sum|q||k|*scale
    adm = torch.ones(B, 1, S, S, dtype=torch.bool, device=dev)
    if causal:
        adm = adm & torch.tril(torch.ones(S, S, dtype=torch.bool, device=dev))
    if kvmask is not None:
        md = kvmask.double().view(B, 1, 1, S)
        adm = adm & (md > F32_MIN)
        mfin = torch.where(md > F32_MIN, md, torch.zeros_like(md))
        s = s + mfin
        s_abs = s_abs + mfin.abs()
    adm = adm.expand(B, Hq, S, S)
    ninf = torch.full_like(s, float("-inf"))
    s = torch.where(adm, s, ninf)
    has = adm.any(-1)                                       # [B,Hq,S]
    m = torch.where(has, s.max(-1).values, torch.zeros_like(s[..., 0]))
    e = torch.exp(s - m.unsqueeze(-1))                      # 0 where -inf
    l = e.sum(-1)
    p = e / torch.where(has, l, torch.ones_like(l)).unsqueeze(-1)
    lse = torch.where(has, m + torch.log(torch.where(has, l,
                                                     torch.ones_like(l))),
                      ninf[..., 0])
    out = p @ vd
    pv_abs = p @ vd.abs()

    zero = torch.zeros_like(s)
    gap = torch.where(adm, (s - m.unsqueeze(-1)).abs(), zero)
    ds_err = U24 * ((D + EPI) * torch.where(adm, s_abs, zero) +
                    2.0 * (gap + 8.0))
    ds_err = torch.where(adm, ds_err, zero)
    ds_max = ds_err.max(-1).values
    eta = 2.0 * ds_max + (S + EPI) * U24
    out_slack = (HALF_BF16 + eta + (S + D + EPI) * U24).unsqueeze(-1) * pv_abs
    lse_fin = torch.where(has, lse, torch.zeros_like(lse))
    lse_tol = ds_max + U24 * ((S + EPI) + C_LOG * ((lse_fin - m).abs() + 8.0)
                              + 4.0 * (lse_fin.abs() + m.abs()))
    r = dict(out=out.permute(0, 2, 1, 3), lse=lse, has=has, pv_abs=pv_abs,
             s_abs=s_abs, lse_tol=lse_tol,
             out_tol=bf16_tol(out, out_slack).permute(0, 2, 1, 3))
    if dout is None:
        return r

    do = _heads(dout)
    drow = (do * out).sum(-1)
    do_o_abs = (do.abs() * out.abs()).sum(-1)               # sum|dO||O|
    dp = do @ vd.transpose(-1, -2)
    dp_abs = do.abs() @ vd.abs().transpose(-1, -2)
    dmd = dp - drow.unsqueeze(-1)
    ds = p * dmd * scale
    dq = ds @ kd
    dq_terms = ds.abs() @ kd.abs()                          # |dS| @ |K|
    pt_do_abs = p.transpose(-1, -2) @ do.abs()              # P^T @ |dO|
    dst_q_abs = ds.abs().transpose(-1, -2) @ qd.abs()       # |dS|^T @ |Q|

    def group(t):         # [B,Hq,S,D] -> [B,S,Hk,D], summed over the group
        return t.reshape(B, Hk, G, S, D).sum(2).permute(0, 2, 1, 3)

    etab = ds_err + (lse_tol + 4.0 * U24).unsqueeze(-1)
    e_drow = (do.abs() * (HALF_BF16 * out.abs() + out_slack)).sum(-1) + \
        (D + EPI) * U24 * do_o_abs
    e_ds = scale * p * (etab * dmd.abs() + D * U24 * dp_abs +
                        e_drow.unsqueeze(-1)) + 3.0 * U24 * ds.abs()
    E = (1.0 + HALF_BF16) * e_ds + HALF_BF16 * ds.abs()
    dq_slack = E @ kd.abs() + (S + EPI) * U24 * dq_terms
    dk_slack = group(E.transpose(-1, -2) @ qd.abs()) + \
        (G * S + EPI) * U24 * group(dst_q_abs)
    dv_slack = (HALF_BF16 + (G * S + EPI) * U24) * group(pt_do_abs) + \
        group((etab * p).transpose(-1, -2) @ do.abs())
    dk = group(ds.transpose(-1, -2) @ qd)
    dv = group(p.transpose(-1, -2) @ do)
    dq = dq.permute(0, 2, 1, 3)
    dq_slack = dq_slack.permute(0, 2, 1, 3)
    r.update(dq=dq, dk=dk, dv=dv, do_o_abs=do_o_abs, dq_terms=dq_terms,
             pt_do_abs=pt_do_abs, dst_q_abs=dst_q_abs,
             dq_slack=dq_slack, dk_slack=dk_slack,
             dq_tol=bf16_tol(dq, dq_slack),
             dk_tol=bf16_tol(dk, dk_slack), dv_tol=bf16_tol(dv, dv_slack))
    return r


def unrotate_ref(d, slack, cos, sin):
    """Inverse rotate-half rotation at table row s of a float64 gradient
    d [B,S,H,D] that the kernel holds to within `slack` before rounding.
    cos / sin: fp32 [>= S, D/2], rows 0..S-1 used. Returns (reference,
    elementwise tolerance), derived in the module docstring."""
    S, D = d.shape[1], d.shape[3]
    half = D // 2
    c = cos[:S].to(d.device).double().reshape(1, S, 1, half)
    s = sin[:S].to(d.device).double().reshape(1, S, 1, half)
    d1, d2 = d[..., :half], d[..., half:]
    e1, e2 = slack[..., :half], slack[..., half:]
    ca, sa = c.abs(), s.abs()
    ref = torch.cat([d1 * c + d2 * s, d2 * c - d1 * s], -1)
    sl = torch.cat([ca * e1 + sa * e2 + 3.0 * U24 * (ca * d1.abs() +
                                                      sa * d2.abs()),
                    ca * e2 + sa * e1 + 3.0 * U24 * (ca * d2.abs() +
                                                      sa * d1.abs())], -1)
    return ref, bf16_tol(ref, sl)


def unrotated_grads(r, cos, sin):
    """dq, dk of attention_ref's dict `r` with respect to the un-rotated q and
    k, and their tolerances."""
    dq, dq_tol = unrotate_ref(r["dq"], r["dq_slack"], cos, sin)
    dk, dk_tol = unrotate_ref(r["dk"], r["dk_slack"], cos, sin)
    return dict(dq=dq, dq_tol=dq_tol, dk=dk, dk_tol=dk_tol)


def make_rope_tables(S, D, extra=3, device="cpu", seed=0, poison=True):
    """cos, sin [S + extra, D/2], fp32, contiguous: one angle per (row,
    column), uniform in [0, 2 pi), so every entry is distinct and of order 1
    and a wrong row, column or sign shows in every column. The kernels only
    read the table, so it need not be a RoPE table. poison: rows S.. are NaN
    (no kernel may read them); otherwise they hold angles like the rest."""
    g = torch.Generator().manual_seed(seed + 104729 * S + D)
    ang = torch.rand(S + extra, D // 2, generator=g,
                     dtype=torch.float64) * (2.0 * math.pi)
    cos, sin = ang.cos().float(), ang.sin().float()
    if poison:
        cos[S:] = float("nan")
        sin[S:] = float("nan")
    return cos.contiguous().to(device), sin.contiguous().to(device)


def check_attention(got, r, what, backward=True):
    """got: dict with out, lse (and dq, dk, dv). Elementwise against the
    reference dict `r`; lse only on rows that have an admissible column."""
    assert_within(got["out"], r["out"], r["out_tol"], f"{what} out")
    lse = got["lse"].detach().double().cpu()
    assert not torch.isnan(lse).any(), f"{what} lse: NaN"
    has = r["has"].cpu()
    zero = torch.zeros_like(lse)
    assert_within(torch.where(has, lse, zero),
                  torch.where(has, r["lse"].cpu(), zero), r["lse_tol"],
                  f"{what} lse")
    if backward:
        for name in ("dq", "dk", "dv"):
            assert_within(got[name], r[name], r[name + "_tol"],
                          f"{what} {name}")


# ---------------------------------------------------------------- inputs
def make_mask(kind, arg, B, S, device):
    """[B,S] additive fp32 mask: batch row 0 carries the mask under test,
    the other row a different one (a 3-column tail pad) or none."""
    if kind is None:
        return None
    m = torch.zeros(B, S, device=device)
    ninf = float("-inf")
    if kind == "tail":            # keys arg.. padded
        m[0, arg:] = ninf
    elif kind == "left":          # keys 0..arg-1 padded (HF left padding)
        m[0, :arg] = ninf
        if S > 3:
            m[1, S - 3:] = ninf
    elif kind == "bias":          # finite bias on the second half
        m[0, S // 2:] = -5.0
    elif kind == "min_left":
        m[0, :arg] = F32_MIN
    elif kind == "min_tail":
        m[0, arg:] = F32_MIN
        m[1, :1] = F32_MIN
    elif kind == "full":          # one fully masked batch row
        m[0, :] = ninf
    else:
        raise ValueError(kind)
    return m


def sentinel_keys(L):
    """Last valid key, both sides of the 64 and 256 boundaries, and the
    first key of the last 64-tile."""
    return sorted({j for j in (L - 1, 63, 64, 255, 256, 64 * ((L - 1) // 64))
                   if 0 <= j < L})


def make_inputs(case, device="cpu", seed=0):
    """bf16 q, k, v, dout and the mask for one case. q ~ 0.5 N(0,1) keeps the
    softmax flat, so every key carries ~1/S of the weight; heads and batches
    get distinct offsets; V and dO carry +-64 sentinels at the edges that a
    tile loop can drop; inadmissible columns carry V = 1000."""
    S, D, Hq, Hk = case["S"], case["D"], case["Hq"], case["Hk"]
    B = 2
    g = torch.Generator().manual_seed(seed + 7919 * S + 31 * Hq + D)

    def rn(*shape):
        return torch.randn(*shape, generator=g)

    hq = torch.arange(Hq).view(1, 1, Hq, 1)
    hk = torch.arange(Hk).view(1, 1, Hk, 1)
    bb = torch.arange(B).view(B, 1, 1, 1)
    q = 0.5 * rn(B, S, Hq, D) + 0.05 * (hq + 1) - 0.1 * bb
    k = rn(B, S, Hk, D) + 0.25 * (hk + 1) * (1 - 2 * bb)
    v = rn(B, S, Hk, D) + 0.75 * (hk + 1) + 2.0 * bb
    do = rn(B, S, Hq, D) + 0.5 * (hq + 1) - 1.0 * bb
    mask = make_mask(case.get("mask"), case.get("arg"), B, S, "cpu")
    for b in range(B):
        if mask is None:
            valid = torch.ones(S, dtype=torch.bool)
        else:
            valid = mask[b] > F32_MIN
            v[b, ~valid] = MASKED_V
        idx = torch.nonzero(valid).flatten()
        if idx.numel():
            L = int(idx[-1]) + 1
            for n, j in enumerate(sentinel_keys(L)):
                if valid[j]:
                    v[b, j] = SENT * (1 - 2 * (n % 2))
    for n, i in enumerate(sentinel_keys(S)):
        do[:, i] = SENT * (1 - 2 * (n % 2))
    bf = torch.bfloat16
    to = dict(device=device, dtype=bf)
    return (q.to(**to), k.to(**to), v.to(**to), do.to(**to),
            None if mask is None else mask.to(device))


def case_scale(case):
    return 0.25 if case.get("custom") else 1.0 / math.sqrt(case["D"])


def case_id(c):
    s = f"S{c['S']}-D{c['D']}-H{c['Hq']}x{c['Hk']}-" \
        f"{'causal' if c['causal'] else 'full'}"
    if c.get("custom"):
        s += "-scale.25"
    if c.get("mask"):
        s += f"-{c['mask']}{c.get('arg', '')}"
    return s


def _c(S, D, H, causal, custom=False, mask=None, arg=None):
    return dict(S=S, D=D, Hq=H[0], Hk=H[1], causal=causal, custom=custom,
                mask=mask, arg=arg)


# Tile sizes straddled: forward 256 rows/block, 32/wave, 64 kv/tile. The
# backward (128-row workgroups of 4 waves x 32 rows in both passes, 32-row
# streamed steps, scratch padded to 128 and written in 64-row tiles) has its
# own cases in attn_bwd_tile_cases.py.
ATTN_CASES = [
    # unmasked: every S, causal and not, both D, every head layout
    _c(1, 64, (1, 1), True), _c(1, 128, (4, 1), False, True),
    _c(31, 128, (6, 2), True, True), _c(31, 64, (8, 1), False),
    _c(33, 64, (4, 4), True), _c(33, 128, (1, 1), False, True),
    _c(64, 128, (4, 1), True), _c(64, 64, (6, 2), False, True),
    _c(65, 64, (8, 1), True, True), _c(65, 128, (4, 4), False),
    _c(255, 128, (6, 2), True), _c(255, 64, (4, 1), False, True),
    _c(256, 64, (4, 4), True, True), _c(256, 128, (8, 1), False),
    _c(257, 128, (1, 1), True), _c(257, 64, (6, 2), False),
    _c(321, 64, (6, 2), True, True), _c(321, 128, (4, 1), False),
    _c(321, 128, (8, 1), True), _c(257, 128, (6, 2), False, True),
    # masks: batch row 0 masked, row 1 different; forward and backward
    _c(65, 64, (4, 1), False, mask="tail", arg=1),
    _c(65, 128, (1, 1), True, mask="tail", arg=1),
    _c(257, 128, (4, 1), False, mask="tail", arg=64),
    _c(257, 64, (6, 2), True, mask="tail", arg=64),
    _c(321, 64, (4, 4), False, True, mask="tail", arg=320),
    _c(33, 128, (8, 1), True, mask="tail", arg=32),
    _c(65, 128, (4, 4), False, mask="left", arg=1),
    _c(65, 64, (1, 1), True, True, mask="left", arg=1),
    _c(257, 64, (4, 1), False, mask="left", arg=63),
    _c(257, 128, (6, 2), False, mask="left", arg=64),
    _c(257, 64, (8, 1), True, mask="left", arg=64),
    _c(321, 128, (4, 1), True, True, mask="left", arg=65),
    _c(321, 64, (6, 2), False, mask="left", arg=130),
    _c(257, 128, (4, 4), True, mask="left", arg=130),
    _c(255, 64, (6, 2), False, mask="bias"),
    _c(255, 128, (4, 1), True, mask="bias"),
    _c(256, 128, (1, 1), False, mask="min_left", arg=64),
    _c(256, 64, (4, 1), True, mask="min_left", arg=64),
    _c(321, 128, (6, 2), True, mask="min_tail", arg=64),
    _c(65, 64, (6, 2), False, mask="full"),
    _c(257, 128, (4, 1), True, mask="full"),
]


# ------------------------------------------------------------ ragged decode
def ragged_ref(q, kpool, vpool, rows, lens):
    """float64 decode attention of each q row over the first lens[i] positions
    of slot rows[i]; scale 1/sqrt(D). q [n,1,Hq,D], pools [B,Smax,Hk,D].
    Returns out [n,1,Hq,D], terms = P @ |V| and the tolerance derived in the
    module docstring. A row of length 0 is defined as exactly 0."""
    n, _, Hq, D = q.shape
    Hk = kpool.shape[2]
    G = Hq // Hk
    scale = 1.0 / math.sqrt(D)
    hmap = torch.arange(Hq, device=q.device) // G
    outs, terms, tols = [], [], []
    for i in range(n):
        L, slot = int(lens[i]), int(rows[i])
        qi = q[i, 0].double()                               # [Hq,D]
        if L == 0:
            z = torch.zeros_like(qi)
            outs.append(z), terms.append(z), tols.append(z)
            continue
        kk = kpool[slot, :L].double()[:, hmap]              # [L,Hq,D]
        vv = vpool[slot, :L].double()[:, hmap]
        s = torch.einsum("hd,lhd->hl", qi, kk) * scale
        s_abs = torch.einsum("hd,lhd->hl", qi.abs(), kk.abs()) * scale
        m = s.max(-1, keepdim=True).values
        p = torch.softmax(s, -1)
        o = torch.einsum("hl,lhd->hd", p, vv)
        t = torch.einsum("hl,lhd->hd", p, vv.abs())
        ds = U24 * ((D + EPI) * s_abs + 2.0 * (s - m).abs())
        eta = 2.0 * ds.max(-1, keepdim=True).values + (L + EPI) * U24
        outs.append(o), terms.append(t)
        tols.append(bf16_tol(o, (eta + 4.0 * (L + D + EPI) * U24) * t))
    st = lambda ts: torch.stack(ts).unsqueeze(1)            # noqa: E731
    return dict(out=st(outs), terms=st(terms), tol=st(tols))


def make_ragged(lens, dup, G, D, Hk, n_slots, Smax, device="cpu", seed=0):
    """Pools poisoned with NaN at every position >= len and in every slot
    that `rows` does not name; V sentinel 64 at position len - 1. `rows` is a
    permutation of slots; row `dup[0]` names the same slot as row `dup[1]`
    (with its own, shorter or equal, length)."""
    g = torch.Generator().manual_seed(seed + 13 * G + D + Hk)
    n = len(lens)
    Hq = G * Hk
    rows = torch.randperm(n_slots, generator=g)[:n].clone()
    rows[dup[0]] = rows[dup[1]]
    assert lens[dup[0]] <= lens[dup[1]]
    hk = torch.arange(Hk).view(1, 1, Hk, 1)
    kpool = torch.randn(n_slots, Smax, Hk, D, generator=g) + 0.25 * (hk + 1)
    vpool = torch.randn(n_slots, Smax, Hk, D, generator=g) + 0.75 * (hk + 1)
    q = 0.5 * torch.randn(n, 1, Hq, D, generator=g)
    fill = torch.zeros(n_slots, dtype=torch.long)
    for i in range(n):
        fill[rows[i]] = max(int(fill[rows[i]]), lens[i])
        if lens[i]:
            vpool[rows[i], lens[i] - 1] = SENT
    for s in range(n_slots):
        kpool[s, int(fill[s]):] = float("nan")
        vpool[s, int(fill[s]):] = float("nan")
    to = dict(device=device, dtype=torch.bfloat16)
    return (q.to(**to), kpool.to(**to), vpool.to(**to), rows.to(device),
            torch.tensor(lens, dtype=torch.long, device=device))


RAGGED_LENS_A = [1, 2, 3, 4, 5, 7, 8, 9, 37, 5]     # last row: duplicate slot
RAGGED_LENS_B = RAGGED_LENS_A + [257]              # NS = 64, eff_chunk = 8
RAGGED_DUP = (9, 6)                                 # row 9 shares row 6's slot
RAGGED_CHUNKS = [4, 8, 512]
RAGGED_SHAPES = [(G, D, Hk) for G in (1, 2, 4, 8) for D in (64, 128)
                 for Hk in (1, 2)]
