"""Banded causal flash attention (window=, segment_ids=). On the MI355X: the
BAND kernels against the float64 reference of band_attn_refs.py, nothing
exempt. Without a GPU: band bounds, SDPA fallback, arguments, model wiring."""
import math
from dataclasses import replace
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from attn_refs import (HALF_BF16, check_attention, make_inputs,
                       make_rope_tables, unrotated_grads)
from band_attn_refs import (band_adm, band_attention_ref, band_lo,
                            segment_ids)
from edge_refs import assert_within
from deepspeed_amd.ops.attention import (_band_bounds, flash_attention,
                                         rope_flash_attention)
from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
# Every window sweeps its edge across the V / dO sentinels of make_inputs (63,
# 64, 255, 256, the last tile) and a tile size (forward 256 / 32 rows, 64 keys;
# backward 128 rows, 64 keys, 32-row steps). Segment starts per batch row.
SEG_STARTS = ([0, 1, 64, 65, 256], [0, 130])
LAYOUTS = [(1, 1), (4, 1), (6, 2), (8, 2)]
CASES = [dict(S=S, D=D, Hq=LAYOUTS[(n + D // 64) % 4][0],
              Hk=LAYOUTS[(n + D // 64) % 4][1], window=w, seg=False)
         for S, ws in ((65, (1, 64, 65)), (257, (32, 33, 193)),
                       (321, (31, 65, 100, 256, 257)))
         for n, w in enumerate(ws) for D in (64, 128)]
CASES += [dict(S=577, D=128, Hq=8, Hk=2, window=129, seg=False)]
SEG_CASES = [dict(S=321, D=D, Hq=H[0], Hk=H[1], window=w, seg=True)
             for D, H in ((64, (6, 2)), (128, (4, 1))) for w in (None, 65)]
CASES += SEG_CASES
cid = lambda c: "-".join(f"{k}{v}" for k, v in c.items())      # noqa: E731


def _bands(c):                 # (window, segment starts) per batch row, B = 2
    return [(c["window"], st if c["seg"] else None) for st in SEG_STARTS]


def _seg(c, dev):
    return segment_ids(c["S"], _bands(c), dev) if c["seg"] else None


def _kernels(q, k, v, do, scale, band):
    e = get_ext(required=True)
    out, lse = e.flash_attn_fwd(q, k, v, True, scale, None, *band)
    dq, dk, dv = e.flash_attn_bwd(q, k, v, do, out, lse, True, scale, None,
                                  None, None, *band)
    return dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)


def _autograd(fn, q, k, v, do):
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = fn(q, k, v)
    out.backward(do)
    return dict(out=out, dq=q.grad, dk=k.grad, dv=v.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_band_forward_backward_vs_float64(c):
    S, scale = c["S"], 1.0 / math.sqrt(c["D"])
    q, k, v, do, _ = make_inputs(c, DEV)
    ref = band_attention_ref(q, k, v, band_adm(S, _bands(c), DEV), scale, do)
    band = _band_bounds(2, S, c["window"], _seg(c, DEV), DEV) or ()
    assert bool(band) == (c["seg"] or c["window"] < S)
    got = _kernels(q, k, v, do, scale, band)
    check_attention(got, ref, cid(c))
    # the public function runs the same kernels on the same bounds
    pub = _autograd(lambda *a: flash_attention(
        *a, window=c["window"], segment_ids=_seg(c, DEV)), q, k, v, do)
    assert all(torch.equal(t, got[name]) for name, t in pub.items())


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 128])
def test_open_band_is_bit_identical_to_plain_causal(D):
    """kv_lo = 0, q_hi = S: the band variant differs from the plain kernels
    only in which tiles it visits and masks, and here it visits the same."""
    q, k, v, do, _ = make_inputs(dict(S=321, D=D, Hq=6, Hk=2), DEV)
    lo = torch.zeros(2, 321, dtype=torch.int32, device=DEV)
    plain = _kernels(q, k, v, do, 0.0, ())
    banded = _kernels(q, k, v, do, 0.0, (lo, lo + 321))
    assert all(torch.equal(plain[name], banded[name]) for name in plain)


@pytest.mark.gpu
@pytest.mark.parametrize("D,S,window", [(64, 257, 33), (128, 321, 100)])
def test_rope_fused_path_with_window(D, S, window):
    q, k, v, do, _ = make_inputs(dict(S=S, D=D, Hq=6, Hk=2), DEV)
    cos, sin = make_rope_tables(S, D, 3, device=DEV)
    got = _autograd(lambda *a: rope_flash_attention(
        *a, cos, sin, window=window), q, k, v, do)
    qr, kr = get_ext(required=True).rope_qk(q, k, cos, sin)
    ref = band_attention_ref(qr, kr, v, band_adm(S, [(window, None)] * 2, DEV),
                             1.0 / math.sqrt(D), do)
    ref.update(unrotated_grads(ref, cos, sin))
    for name in got:           # the autograd function does not return lse
        assert_within(got[name], ref[name], ref[name + "_tol"], name)


@pytest.mark.parametrize("c", CASES, ids=cid)
def test_band_bounds_vs_brute_force(c):
    S, bands = c["S"], _bands(c)
    band = _band_bounds(2, S, c["window"], _seg(c, "cpu"), "cpu")
    lo = torch.tensor([band_lo(S, w, st) for w, st in bands])
    if not lo.any():
        assert band is None
        return
    kv_lo, q_hi = band
    assert all(t.dtype == torch.int32 and t.is_contiguous() for t in band)
    assert torch.equal(kv_lo, lo.int())
    idx = torch.arange(S)
    causal = idx[None, None] <= idx[None, :, None]
    by_lo = (idx[None, None] >= kv_lo[:, :, None]) & causal
    by_hi = (idx[None, :, None] < q_hi[:, None, :]) & causal
    assert torch.equal(by_lo, by_hi)
    assert torch.equal(by_lo, band_adm(S, _bands(c), "cpu"))


@pytest.mark.parametrize("c", SEG_CASES, ids=cid)
def test_sdpa_fallback_vs_float64(c):
    """fp32 inputs go to SDPA with the boolean band mask: the bound is the
    reference's out slack (EPI fp32 epilogue roundings) less its bf16 P."""
    q, k, v = (t.float() for t in make_inputs(c, "cpu")[:3])
    ref = band_attention_ref(q, k, v, band_adm(c["S"], _bands(c), "cpu"),
                             1.0 / math.sqrt(c["D"]))
    out = flash_attention(q, k, v, window=c["window"],
                          segment_ids=_seg(c, "cpu"))
    tol = ref["out_slack"] - HALF_BF16 * ref["pv_abs"]
    assert_within(out, ref["out"], tol.permute(0, 2, 1, 3), cid(c))


def test_band_argument_errors():
    q = torch.zeros(2, 8, 2, 64)
    seg = torch.zeros(2, 8, dtype=torch.long)
    for kw in (dict(window=4, causal=False), dict(window=0),
               dict(segment_ids=seg, causal=False), dict(window=4, k=q[:, :4]),
               dict(window=4, attn_mask=torch.zeros(2, 8)),
               dict(segment_ids=seg.float()), dict(segment_ids=seg[:, :4]),
               dict(segment_ids=torch.arange(8).flip(0).expand(2, 8))):
        with pytest.raises(ValueError):
            flash_attention(q, kw.pop("k", q), q, **kw)


def test_config_from_hf_reads_sliding_window():
    from deepspeed_amd.models.hf import config_from_hf
    hf = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=4,
              num_attention_heads=2, vocab_size=32, max_position_embeddings=64)
    win = lambda **kw: config_from_hf(                      # noqa: E731
        SimpleNamespace(**hf, **kw)).sliding_window
    assert win() is None and win(sliding_window=4096) == 4096
    assert win(sliding_window=4096, use_sliding_window=False) is None
    assert win(sliding_window=4096, use_sliding_window=True) == 4096
    assert win(sliding_window=4096, max_window_layers=4) is None
    assert win(sliding_window=4096, max_window_layers=0) == 4096
    with pytest.raises(NotImplementedError):
        win(sliding_window=4096, max_window_layers=2)


def test_llama_tiny_sliding_window_matches_dense_mask(monkeypatch):
    from deepspeed_amd.models import llama
    S, W = 32, 8
    torch.manual_seed(0)
    cfg = llama.LLAMA_CONFIGS["llama-tiny"]
    model = llama.LlamaForCausalLM(replace(cfg, sliding_window=W)).eval()
    ids = torch.randint(0, cfg.vocab_size, (2, S))
    i = torch.arange(S)
    dense = torch.where((i[None] <= i[:, None]) & (i[None] > i[:, None] - W),
                        0.0, float("-inf"))

    def dense_attn(q, k, v, causal=True, window=None):
        return F.scaled_dot_product_attention(
            q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
            attn_mask=dense, enable_gqa=True).transpose(1, 2)
    with torch.no_grad():
        got = model(ids)
        monkeypatch.setattr(llama, "flash_attention", dense_attn)
        want = model(ids)
        dense = torch.where(i[None] <= i[:, None], 0.0, float("-inf"))
        full = model(ids)
    torch.testing.assert_close(got, want)
    assert not torch.allclose(got[:, W:], full[:, W:], atol=1e-3)
