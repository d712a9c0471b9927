"""`ragged_prefill_gqa_fp8`, the MFMA fused-step kernel over the fp8 KV slot
pool (needs MI355X): elementwise against the float64 banded reference
(ragged_prefill_band_refs; ragged_prefill_ref without a window) over the
DEQUANTIZED clean pool, where code * scale is exact. The kernel reads the
poisoned pools: NaN codes AND NaN scales past each fill, in unnamed slots and
below each sequence's band.

Bound: the reference's tol plus the `extra` term of kv_fp8_refs "Attention
bound" with UNITS_PREFILL = 1. Beyond `ragged_prefill_gqa`, which passes the
plain tol with the same MFMAs and wave merge, the kernel rounds once more on
every score ((q . code) * k_scale) and once more on p * v_scale, as
ragged_prefill_fp8 does. Under a window the same formula runs over the band's
admissible set. Nothing is tuned."""
import functools
import math

import pytest
import torch

from edge_refs import U24, assert_within
from kv_fp8_refs import (FP8, UNITS_PREFILL, dequant64, fp8_extra_slack,
                         spread_quantize)
from ragged_prefill_band_refs import band_case, ragged_prefill_band_ref
from ragged_prefill_refs import (N_SLOTS, SMAX, make_ragged_prefill,
                                 ragged_prefill_ref)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF = torch.bfloat16


def _ext():
    return get_ext(required=True)


def _batch(seqs, n_slots=N_SLOTS, smax=SMAX):
    from deepspeed_amd.inference.ragged_batch import RaggedBatch
    return RaggedBatch(seqs, n_slots, smax, DEV)


def _band_extra(q, k64, v64, seqs, window):
    """kv_fp8_refs.fp8_extra_slack with pos - window < col <= pos, on q's
    device."""
    T, Hq, D = q.shape
    dev = q.device
    hmap = torch.arange(Hq, device=dev) // (Hq // k64.shape[2])
    scale = 1.0 / math.sqrt(D)
    out = torch.zeros(T, Hq, D, dtype=torch.float64, device=dev)
    for slot, q_start, q_len, kv_len in seqs:
        qs = q[q_start:q_start + q_len].double().transpose(0, 1)
        kk = k64[slot, :kv_len][:, hmap].transpose(0, 1)
        vv = v64[slot, :kv_len][:, hmap].transpose(0, 1)
        pos = torch.arange(kv_len - q_len, kv_len, device=dev).view(-1, 1)
        col = torch.arange(kv_len, device=dev).view(1, -1)
        adm = (col <= pos) & (col > pos - window)
        s = qs @ kk.transpose(-1, -2) * scale
        s_abs = qs.abs() @ kk.abs().transpose(-1, -2) * scale
        s = torch.where(adm, s, torch.full_like(s, float("-inf")))
        t = torch.softmax(s, -1) @ vv.abs()
        smax = torch.where(adm, s_abs, torch.zeros_like(s_abs)) \
            .max(-1, keepdim=True).values
        out[q_start:q_start + q_len] = \
            ((2.0 * smax + UNITS_PREFILL) * U24 * t).transpose(0, 1)
    return out


def _fp8(q, kp, vp, seqs, window):
    """(clean, poisoned) fp8 pools of bf16 pools, float64 reference, bound.
    The float64 work runs on the device, as in band_case."""
    clean, poisoned = spread_quantize(kp, vp)
    k64, v64 = dequant64(clean[0], clean[2]), dequant64(clean[1], clean[3])
    if window:
        k64, v64 = k64.to(q.device), v64.to(q.device)
        ref = ragged_prefill_band_ref(q, k64, v64, seqs, window)
        extra = _band_extra(q, k64, v64, seqs, window)
    else:
        ref = ragged_prefill_ref(q, k64.to(q.device), v64.to(q.device), seqs)
        extra = fp8_extra_slack(q, k64, v64, seqs, UNITS_PREFILL).to(q.device)
    return clean, poisoned, ref["out"], ref["tol"] + extra


@functools.lru_cache(maxsize=None)
def _case(G, D, Hk, window):
    """band_case through spread_quantize; shared, callers must not modify."""
    q, kp, vp, seqs, _ = band_case(G, D, Hk, window, DEV)
    return (q, seqs) + _fp8(q, kp, vp, seqs, window)


@pytest.mark.parametrize("Hk", (1, 2))
@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("G", (1, 3, 7, 8, 32))
def test_prefill_gqa_fp8_vs_float64(G, D, Hk):
    """The maxima only size the grid and the checks: max_kvlen = Smax and
    max_qlen = T (cut to Smax) give the same bits."""
    for window in (0, 1, 5, 33, 64, 1000):
        q, seqs, _, pools, ref, tol = _case(G, D, Hk, window)
        b = _batch(seqs)
        out = _ext().ragged_prefill_gqa_fp8(q, *pools, b.desc, b.max_qlen,
                                            b.max_kvlen, window)
        assert out.shape == q.shape and out.dtype == BF
        assert not out.isnan().any(), window
        assert_within(out, ref, tol, f"window {window}")
        wide = _ext().ragged_prefill_gqa_fp8(q, *pools, b.desc,
                                             min(q.shape[0], SMAX), SMAX,
                                             window)
        assert torch.equal(wide, out), window


@pytest.mark.parametrize("D", (64, 128))
@pytest.mark.parametrize("G", (3, 8))
def test_prefill_gqa_fp8_long_range(G, D):
    """More than 384 keys: every wave runs four or more rounds, so both
    stages are reloaded."""
    q, kp, vp, seqs = make_ragged_prefill([(1, 513), (40, 500)], G, D, 2,
                                          n_slots=3, Smax=520, device=DEV)
    b = _batch(seqs, 3, 520)
    for window in (0, 130):
        _, pools, ref, tol = _fp8(q, kp, vp, seqs, window)
        out = _ext().ragged_prefill_gqa_fp8(q, *pools, b.desc, b.max_qlen,
                                            b.max_kvlen, window)
        assert_within(out, ref, tol, f"window {window}")


@pytest.mark.parametrize("window", (0, 33))
def test_prefill_gqa_fp8_poison_does_not_leak(window):
    q, seqs, clean, poisoned, _, _ = _case(3, 128, 2, window)
    b = _batch(seqs)
    a, p = (_ext().ragged_prefill_gqa_fp8(q, *pools, b.desc, b.max_qlen,
                                          b.max_kvlen, window)
            for pools in (clean, poisoned))
    assert torch.equal(a.view(torch.int16), p.view(torch.int16))


def _count(monkeypatch, calls, *names):
    for name in names:
        real = getattr(_ext(), name)
        monkeypatch.setattr(_ext(), name, lambda *a, _n=name, _r=real: (
            calls.append((_n, a)), _r(*a))[1])


def test_prefill_gqa_fp8_dispatch(monkeypatch):
    import deepspeed_amd.ops.functional as Fops
    calls = []
    _count(monkeypatch, calls, "ragged_prefill_fp8", "ragged_prefill_gqa_fp8")
    monkeypatch.setattr(Fops, "_ragged_prefill_torch",
                        lambda *a, **k: pytest.fail("torch fallback ran"))
    for G, kw, window, want in (
            (4, {}, 0, "ragged_prefill_fp8"),
            (4, {"window": 16}, 16, "ragged_prefill_gqa_fp8"),
            (3, {}, 0, "ragged_prefill_gqa_fp8"),
            (4, {"mfma": True}, 0, "ragged_prefill_gqa_fp8")):
        q, seqs, _, pools, ref, tol = _case(G, 64, 2, window)
        out = Fops.ragged_prefill_attention_fp8(q, *pools, _batch(seqs), **kw)
        assert calls.pop()[0] == want and not calls, (G, kw)
        assert_within(out, ref, tol, f"G {G} {kw}")


def test_prefill_gqa_fp8_rejects_bad_arguments():
    """Built as in test_decode_gqa_fp8_rejects_bad_arguments: pools and scales
    are leading views of larger buffers and every bad tensor is at least as
    large as the good one."""
    T, Hk, G, D, B, Smax = 6, 2, 3, 64, 4, 16

    def codes(*shape):
        return torch.zeros(*shape, device=DEV, dtype=torch.uint8).view(FP8)

    kbuf, sbuf = codes(B + 2, Smax, Hk, D), torch.ones(B + 2, Smax, Hk,
                                                       device=DEV)
    desc = torch.tensor([[2, 0, 5, 9], [0, 5, 1, 16]], device=DEV)
    good = dict(q=torch.zeros(T, Hk * G, D, device=DEV, dtype=BF),
                kp=kbuf[:B], vp=codes(B + 2, Smax, Hk, D)[:B], ks=sbuf[:B],
                vs=sbuf[:B], desc=desc, mq=5, mk=16, w=4)

    def call(**kw):
        a = {**good, **kw}
        return _ext().ragged_prefill_gqa_fp8(
            a["q"], a["kp"], a["vp"], a["ks"], a["vs"], a["desc"], a["mq"],
            a["mk"], a["w"])
    call()
    k1, s1 = codes(B + 2, Smax, 1, D)[:B], sbuf[:B, :, :1].contiguous()
    wide = codes(B, Smax, Hk, 256)
    long8 = torch.zeros(4, 8, dtype=torch.long, device=DEV)
    bad = {
        "G = 33": dict(q=good["q"].new_zeros(T, 33, D), kp=k1, vp=k1, ks=s1,
                       vs=s1),
        "window -1": dict(w=-1),
        "max_kvlen > Smax": dict(mk=Smax + 1),
        "max_qlen > max_kvlen": dict(mq=9, mk=8),
        "head_dim 256": dict(q=good["q"].new_zeros(T, Hk * G, 256), kp=wide,
                             vp=wide),
        "q dtype": dict(q=good["q"].float()),
        "kpool dtype": dict(kp=good["kp"].to(BF)),
        "vpool dtype": dict(vp=good["vp"].view(torch.uint8)),
        "k_scale dtype": dict(ks=good["ks"].double()),
        "v_scale dtype": dict(vs=good["vs"].to(BF)),
        "desc int32": dict(desc=desc.int()),
        "k_scale shape": dict(ks=sbuf),
        "v_scale shape": dict(vs=sbuf.unsqueeze(-1)[:B]),
        "kpool misaligned": dict(
            kp=codes(B * Smax * Hk * D + 8)[8:].view(B, Smax, Hk, D)),
        "kpool strided": dict(kp=wide[..., :D]),
        "desc strided": dict(desc=long8[:2, ::2]),
        "kpool device": dict(kp=kbuf.cpu()[:B]),
        "k_scale device": dict(ks=sbuf.cpu()[:B]),
    }
    for name, kw in bad.items():
        with pytest.raises(RuntimeError):
            call(**kw)
            pytest.fail(f"'{name}' did not raise")


@pytest.mark.parametrize("heads,window,mfma", [((6, 2), None, {}),
                                               ((4, 2), 16, {}),
                                               ((4, 2), None,
                                                {"mfma_prefill": True})])
def test_prefill_gqa_fp8_engine_gpu(monkeypatch, heads, window, mfma):
    """test_decode_gqa_fp8_engine_gpu's model on the fused step over the fp8
    pool. Bookkeeping, the kernel called and the window reaching it are
    exact; the greedy-token agreement with the bf16-pool engine is printed,
    not asserted (nobody has measured it)."""
    import deepspeed_amd.models.llama as llama
    from deepspeed_amd.inference.serving import ContinuousBatchingEngine

    cfg = llama.LlamaConfig(hidden_size=64 * heads[0], intermediate_size=688,
                            num_hidden_layers=2, num_attention_heads=heads[0],
                            num_key_value_heads=heads[1], vocab_size=2048,
                            max_position_embeddings=512,
                            activation_checkpointing=False,
                            sliding_window=window)
    torch.manual_seed(0)
    model = llama.LlamaForCausalLM(cfg).to(DEV, BF).eval()
    torch.manual_seed(1)
    prompts = [torch.randint(0, 2000, (n,)) for n in (20, 40, 27, 70)]
    new = 8

    def run(**kw):
        cb = ContinuousBatchingEngine(model, max_batch=2, prefill_chunk=16,
                                      prefill_budget=32, fused_step=True,
                                      fused_kv_append=True, **kw)
        rids = [cb.add_request(p, max_new_tokens=new) for p in prompts]
        return cb, rids, cb.run()

    _, ref_rids, ref_out = run()
    calls = []
    _count(monkeypatch, calls, "ragged_prefill", "ragged_prefill_gqa",
           "ragged_prefill_fp8", "ragged_prefill_gqa_fp8")
    cb, rids, out = run(kv_dtype="fp8", **mfma)

    assert sorted(cb.free_slots) == [0, 1]
    assert not cb.running and not cb.pending and not cb.prefilling
    assert {name for name, _ in calls} == {"ragged_prefill_gqa_fp8"}
    assert all(a[8] == (window or 0) for _, a in calls)
    for rid, p in zip(rids, prompts):
        assert len(out[rid]) == len(p) + new, rid
        assert torch.equal(out[rid][:len(p)], p), rid
    agree = [float((out[a] == ref_out[b]).float().mean())
             for a, b in zip(rids, ref_rids)]
    print(f"greedy agreement fp8 pool vs bf16 pool, fused step (heads={heads}"
          f", window={window}, {mfma}, reported, not asserted): "
          f"{sum(agree) / len(agree):.3f}")
