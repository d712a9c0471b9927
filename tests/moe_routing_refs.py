"""Plain float64 references, bounds and inputs for the MoE routing tests.

Gate bound, derived the way `edge_refs.py` derives its own (units of
2^-24 = U24, all relative to the gate g_e = exp(t_e) / sum exp(t), t = x - m):
  * exp(t_e): rounding the argument x - m moves exp by |t_e| relative, an
    exp2-based evaluation by as much again: 2 |t_e|;
  * the sum has E positive terms (condition 1): E for the additions, plus the
    terms' own argument errors, 2 E_p[|t|] on the sum;
  * EPI = 8 fixed roundings: exp at <= 1 ulp (2 units) in numerator and sum,
    one division, and margin for the renormalisation's own division.
So rel(g_e) = U24 * (E + EPI + 2 |t_e| + 2 E_p[|t|]).
  * weights = g_j / sum of <= k kept gates: numerator and denominator each
    carry at most the row's largest rel, the sum k roundings, the division
    one: rel(w) = 2 max_e rel(g_e) + (k + EPI) U24.
  * l_aux = E*E/k sum_e me_e ce_e: ce_e (a count / S) is exact up to fixed
    roundings; me_e is an S-term fp32 sum of gates, each off by its own
    bound: tol = E*E/k sum_e ce_e mean_s(rel * g)[e] + (S + E + EPI) U24 l_aux.
  * dlogits = g_e (dg_e - sum g dg): g, the renormalisation's denominator,
    its weights and the dot's gates carry the row's largest rel each (4), the
    sums have E + k terms, plus 2 EPI fixed roundings, all on
    g_e (|dg_e| + sum g |dg|) with |dg| built from absolute values.
"""
import torch

from edge_refs import BF16_ULP, EPI, U24


def make_logits(S, E, seed):
    """fp32 logits on a jittered grid: every row is a permutation of E grid
    points `step` apart (jitter +-0.1 step), expert 0 pushed up and expert 1
    down by E/2 + 1/3 steps, so queue 0 overflows, queue 1 stays short, and
    two gates of a row never come closer than 0.13 step relative."""
    g = torch.Generator().manual_seed(seed)
    base = torch.argsort(torch.rand(S, E, generator=g), dim=1).double()
    base[:, 0] += E // 2 + 1.0 / 3
    base[:, 1] -= E // 2 + 1.0 / 3
    jitter = (torch.rand(S, E, generator=g, dtype=torch.float64) - 0.5) * 0.2
    return ((base + jitter) * (4.0 / E)).float()


def gate_ref(logits, k, capacity, drop_tokens):
    """float64 gate: softmax, stable sort by (value descending, index
    ascending), running counts in token order. Returns a dict with the seven
    outputs, the capacity used, the gates and the tolerances."""
    x = logits.double().cpu()
    S, E = x.shape
    t = x - x.max(dim=1, keepdim=True).values
    gates = torch.softmax(x, dim=1)
    idx = torch.sort(gates, dim=1, descending=True, stable=True).indices[:, :k]
    mask = torch.zeros(S, E, dtype=torch.float64).scatter_(1, idx, 1.0)
    counts = mask.sum(0).long()
    loc = (torch.cumsum(mask, 0) - 1).gather(1, idx).long()
    if drop_tokens:
        keep = loc < capacity
    else:
        capacity = max(capacity, int(counts.max()) if S else 1)
        keep = torch.ones_like(loc, dtype=torch.bool)
    vals = gates.gather(1, idx) * keep
    den = vals.sum(1, keepdim=True).clamp(min=1e-9)
    weights = vals / den
    l_aux = (gates.mean(0) * mask.mean(0)).sum() * E * E / k
    slot_token = torch.full((E * capacity,), -1, dtype=torch.long)
    slot_token[(idx * capacity + loc)[keep]] = \
        torch.arange(S * k).view(S, k)[keep]

    rel = U24 * (E + EPI + 2 * t.abs() +
                 2 * (gates * t.abs()).sum(1, keepdim=True))
    rel_row = rel.max(dim=1, keepdim=True).values
    w_tol = weights * (2 * rel_row + (k + EPI) * U24)
    l_aux_tol = (E * E / k) * (mask.mean(0) * (rel * gates).mean(0)).sum() \
        + (S + E + EPI) * U24 * l_aux
    return dict(idx=idx, loc=loc, keep=keep, weights=weights, counts=counts,
                l_aux=l_aux, slot_token=slot_token, capacity=capacity,
                gates=gates, den=den, gate_tol=rel * gates, rel_row=rel_row,
                w_tol=w_tol, l_aux_tol=l_aux_tol)


def assert_gaps(r):
    """fp32 and float64 must order every row alike: adjacent sorted gates
    differ by more than both their bounds."""
    g, order = torch.sort(r["gates"], dim=1, descending=True, stable=True)
    tol = r["gate_tol"].gather(1, order)
    assert (g[:, :-1] - g[:, 1:] > tol[:, :-1] + tol[:, 1:]).all()


def gate_grad_ref(r, dweights, dl_aux):
    """Closed-form float64 dlogits of sum(weights * dweights) + dl_aux *
    l_aux, the mask held constant; and its tolerance."""
    g, idx, keep = r["gates"], r["idx"], r["keep"]
    S, E = g.shape
    k = idx.shape[1]
    dw = dweights.double().cpu() * keep
    w, den = r["weights"], r["den"]
    live = (den > 1e-9).double()        # under the clamp den is a constant
    dv = (dw - live * (dw * w).sum(1, keepdim=True)) / den * keep
    dv_abs = (dw.abs() + (dw * w).abs().sum(1, keepdim=True)) / den * keep
    base = float(dl_aux) * (E * E / k) * r["counts"].double() / S / S
    dg = base.expand(S, E).clone().scatter_add_(1, idx, dv)
    dg_abs = base.abs().expand(S, E).clone().scatter_add_(1, idx, dv_abs)
    ref = g * (dg - (g * dg).sum(1, keepdim=True))
    terms = g * (dg_abs + (g * dg_abs).sum(1, keepdim=True))
    return ref, (4 * r["rel_row"] + (E + k + 2 * EPI) * U24) * terms


def rows_ref(r, x, expert_out, dout, d_disp):
    """float64 dispatch / combine and their gradients under routing `r`.
    x, dout [S, M]; expert_out, d_disp [E*C, M]. `*_abs` are sum|terms|."""
    idx, loc, keep, w = r["idx"], r["loc"], r["keep"], r["weights"]
    S, k = idx.shape
    C = r["capacity"]
    x, eo, dout, dd = (t.double().cpu() for t in (x, expert_out, dout, d_disp))
    st = r["slot_token"]
    full = st >= 0
    tok = st.clamp(min=0) // k
    disp = x[tok] * full.unsqueeze(1)
    pos = (idx * C + loc).clamp(max=eo.shape[0] - 1)            # [S, k]
    kd = keep.double().unsqueeze(-1)
    rows, drows = eo[pos] * kd, dd[pos] * kd                    # [S, k, M]
    wk = w.unsqueeze(-1)
    w_slot = w.reshape(-1)[st.clamp(min=0)] * full
    return dict(
        disp=disp, comb=(wk * rows).sum(1), comb_abs=(wk * rows).abs().sum(1),
        dx=drows.sum(1), dx_abs=drows.abs().sum(1),
        d_expert=dout[tok] * w_slot.unsqueeze(1),
        dw=(dout.unsqueeze(1) * rows).sum(-1),
        dw_abs=(dout.unsqueeze(1) * rows).abs().sum(-1))


def rows_tol(ref, terms, n, dtype):
    """One rounding to `dtype` of an n-term fp32 accumulation."""
    ulp = BF16_ULP if dtype == torch.bfloat16 else 0.0
    return ulp * ref.abs() + n * U24 * terms


def routing_on(r, device):
    """The reference routing as the functionals' argument tensors."""
    i32 = torch.int32
    return (r["idx"].to(device, i32), r["loc"].to(device, i32),
            r["keep"].to(device), r["slot_token"].to(device, i32))
