"""float64 closed-form attention over an explicit admissibility matrix, for the
banded causal kernels (window=, segment_ids=). Keys and derivation are those
of attn_refs.attention_ref (its docstring), so attn_refs.check_attention
applies unchanged. One difference: a masked score adds an exact 0 to every
sum the kernels form, so each "S terms accumulated" of those bounds is the
size of the admissible set summed: n_i keys for row i (eta, out, lse, dQ),
G * c_j (q head, row) pairs for key j (dK, dV). Nothing is tuned; every row
admits key i, so no lse is exempt; out_slack is the one extra key."""
import torch

from attn_refs import C_LOG, EPI, HALF_BF16, U24, bf16_tol


def band_lo(S, window, starts):
    """Brute force: first admissible key of each row, a Python list."""
    return [max(0 if window is None else max(0, i - window + 1),
                max(s for s in (starts or [0]) if s <= i)) for i in range(S)]


def band_adm(S, bands, device):
    """bool [B,S,S] from one (window, segment starts) per batch row."""
    idx = torch.arange(S)
    return torch.stack([(idx[None] >= torch.tensor(band_lo(S, w, st))[:, None])
                        & (idx[None] <= idx[:, None])
                        for w, st in bands]).to(device)


def segment_ids(S, bands, device):
    """int64 [B,S], non-decreasing with gaps: the segment's first index."""
    return torch.tensor([band_lo(S, None, st) for _, st in bands]).to(device)


def band_attention_ref(q, k, v, adm, scale, dout=None):
    B, S, Hq, D = q.shape
    Hk = k.shape[2]
    G = Hq // Hk
    hmap = torch.arange(Hq, device=q.device) // G
    hd = lambda t: t.double().permute(0, 2, 1, 3)           # noqa: E731
    qd, kd, vd = hd(q), hd(k)[:, hmap], hd(v)[:, hmap]
    n = adm.sum(-1).double()[:, None]                       # [B,1,S] keys/row
    c = (G * adm.sum(-2).double())[:, :, None, None]        # [B,S,1,1]
    adm = adm[:, None].expand(B, Hq, S, S)
    zero = torch.zeros((), dtype=torch.float64, device=q.device)
    s = torch.where(adm, qd @ kd.mT * scale, zero - float("inf"))
    s_abs = torch.where(adm, qd.abs() @ kd.abs().mT * scale, zero)
    m = s.max(-1).values
    e = torch.exp(s - m[..., None])
    p = e / e.sum(-1, keepdim=True)
    lse = m + torch.log(e.sum(-1))
    out, pv_abs = p @ vd, p @ vd.abs()
    gap = torch.where(adm, (s - m[..., None]).abs(), zero)
    ds_err = torch.where(adm, U24 * ((D + EPI) * s_abs + 2 * (gap + 8)), zero)
    ds_max = ds_err.max(-1).values
    eta = 2.0 * ds_max + (n + EPI) * U24
    out_slack = (HALF_BF16 + eta + (n + D + EPI) * U24)[..., None] * pv_abs
    lse_tol = ds_max + U24 * ((n + EPI) + C_LOG * ((lse - m).abs() + 8.0)
                              + 4.0 * (lse.abs() + m.abs()))
    r = dict(out=out.permute(0, 2, 1, 3), lse=lse, has=adm.any(-1),
             pv_abs=pv_abs, s_abs=s_abs, lse_tol=lse_tol, out_slack=out_slack,
             out_tol=bf16_tol(out, out_slack).permute(0, 2, 1, 3))
    if dout is None:
        return r
    do = hd(dout)
    do_o_abs = (do.abs() * out.abs()).sum(-1)
    dp, dp_abs = do @ vd.mT, do.abs() @ vd.abs().mT
    dmd = dp - (do * out).sum(-1)[..., None]
    ds = p * dmd * scale
    dq_terms, pt_do_abs = ds.abs() @ kd.abs(), p.mT @ do.abs()
    dst_q_abs = ds.abs().mT @ qd.abs()
    group = lambda t: t.reshape(B, Hk, G, S, D).sum(2) \
        .permute(0, 2, 1, 3)                                # noqa: E731
    etab = ds_err + (lse_tol + 4.0 * U24)[..., None]
    e_drow = (do.abs() * (HALF_BF16 * out.abs() + out_slack)).sum(-1) + \
        (D + EPI) * U24 * do_o_abs
    e_ds = scale * p * (etab * dmd.abs() + D * U24 * dp_abs +
                        e_drow[..., None]) + 3.0 * U24 * ds.abs()
    E = (1.0 + HALF_BF16) * e_ds + HALF_BF16 * ds.abs()
    dq_slack = (E @ kd.abs() +
                (n + EPI)[..., None] * U24 * dq_terms).permute(0, 2, 1, 3)
    dk_slack = group(E.mT @ qd.abs()) + (c + EPI) * U24 * group(dst_q_abs)
    dv_slack = (HALF_BF16 + (c + EPI) * U24) * group(pt_do_abs) + \
        group((etab * p).mT @ do.abs())
    dq = (ds @ kd).permute(0, 2, 1, 3)
    dk, dv = group(ds.mT @ qd), group(p.mT @ do)
    r.update(dq=dq, dk=dk, dv=dv, do_o_abs=do_o_abs, dq_terms=dq_terms,
             pt_do_abs=pt_do_abs, dst_q_abs=dst_q_abs, dq_slack=dq_slack,
             dk_slack=dk_slack, dq_tol=bf16_tol(dq, dq_slack),
             dk_tol=bf16_tol(dk, dk_slack), dv_tol=bf16_tol(dv, dv_slack))
    return r
