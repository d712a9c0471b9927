"""`ragged_decode_gqa_fp8`, the MFMA split-KV decode kernel over the fp8 KV
slot pool (needs MI355X): elementwise against
ragged_prefill_refs.ragged_prefill_ref (float64) over the DEQUANTIZED pool,
where code * scale is exact, on decode sequences (slot, i, 1, L).

The bf16 case is test_ragged_decode_gqa_gpu's: under a window W the reference
sees each row's positions [L-W', L), W' = min(W, L), copied to 0..W'; the
kernel's pool is NaN below L-W', from L up and in unnamed slots (NaN codes AND
NaN scales after spread_quantize), and V carries the sentinel at L-1 and at
L-W'.

Bound: ragged_prefill_ref's tol plus kv_fp8_refs.fp8_extra_slack with
UNITS_PREFILL = 1. Beyond `ragged_decode_gqa`, which passes the plain tol with
the same MFMAs, wave merge and split combine, the kernel rounds once more on
every score ((q . code) * k_scale, the 2 * max s_abs term of the slack) and
once more on the PV side (p * v_scale in fp32, before P is rounded to bf16):
one unit, as in ragged_prefill_fp8. Nothing is tuned."""
import functools

import pytest
import torch

from attn_refs import SENT
from edge_refs import assert_within
from kv_fp8_refs import (FP8, UNITS_DECODE, UNITS_PREFILL, dequant64,
                         fp8_extra_slack, spread_quantize)
from ragged_prefill_refs import SMAX, make_ragged_prefill, ragged_prefill_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF = torch.bfloat16
# around the 32-key tile, the 128-key round (one tile per wave) and the
# 256-key pair of rounds (both prefetch stages)
LENS = [1, 2, 31, 32, 33, 127, 128, 129, 257, 300]
WINDOWS = [0, 1, 5, 33, 128, 1000]
SPLITS = [1, 3, 0]


def _ext():
    return get_ext(required=True)


def bits(t):
    return t.view(torch.int16)


@functools.lru_cache(maxsize=None)
def _case(G, D, Hk, window=0, lens=tuple(LENS), units=UNITS_PREFILL):
    """q [n,Hq,D], (clean, poisoned) fp8 pools, rows, lens and the float64
    reference and bound in row order; shared, callers must not modify them."""
    q, kp, vp, seqs = make_ragged_prefill([(1, L) for L in lens], G, D, Hk,
                                          device=DEV, poison=True)
    band = []
    for slot, q_start, _, L in seqs:
        w = min(window, L) if window > 0 else L
        vp[slot, L - w] = SENT
        kp[slot, :L - w] = float("nan")
        vp[slot, :L - w] = float("nan")
        band.append((slot, q_start, L, w))
    clean, poisoned = spread_quantize(kp, vp)
    k64, v64 = dequant64(clean[0], clean[2]), dequant64(clean[1], clean[3])
    rk, rv = k64.clone(), v64.clone()
    for slot, _, L, w in band:
        rk[slot, :w], rv[slot, :w] = k64[slot, L - w:L], v64[slot, L - w:L]
    rseqs = [(slot, q_start, 1, w) for slot, q_start, _, w in band]
    ref = ragged_prefill_ref(q.cpu(), rk, rv, rseqs)
    tol = ref["tol"] + fp8_extra_slack(q, rk, rv, rseqs, units)
    order = torch.tensor([s[1] for s in seqs])
    rows = torch.tensor([s[0] for s in seqs], device=DEV)
    ln = torch.tensor([s[3] for s in seqs], device=DEV)
    return (q[order.to(DEV)].contiguous(), clean, poisoned, rows, ln,
            ref["out"][order], tol[order])


@pytest.mark.parametrize("Hk", [1, 2])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [1, 3, 7, 8, 32])
def test_decode_gqa_fp8_vs_float64(G, D, Hk):
    """Every window and split count, on the poisoned pools; max_len only
    sizes the grid, so the output with max_len = Smax is bit-identical to the
    one that reads lens.max()."""
    for window in WINDOWS:
        q, _, pools, rows, ln, ref, tol = _case(G, D, Hk, window)
        for splits in SPLITS:
            out = _ext().ragged_decode_gqa_fp8(q, *pools, rows, ln, window, 0,
                                               splits)
            assert out.shape == (len(LENS), 1, G * Hk, D)
            assert_within(out, ref, tol, f"window={window} splits={splits}")
            out2 = _ext().ragged_decode_gqa_fp8(q, *pools, rows, ln, window,
                                                SMAX, splits)
            assert torch.equal(bits(out), bits(out2))


@pytest.mark.parametrize("window", [0, 33])
def test_decode_gqa_fp8_poison_does_not_leak(window):
    q, clean, poisoned, rows, ln, _, _ = _case(3, 128, 2, window)
    for splits in SPLITS:
        a = _ext().ragged_decode_gqa_fp8(q, *clean, rows, ln, window, 0,
                                         splits)
        b = _ext().ragged_decode_gqa_fp8(q, *poisoned, rows, ln, window, 0,
                                         splits)
        assert torch.equal(bits(a), bits(b)), f"splits={splits}"


@pytest.mark.parametrize("splits", SPLITS)
def test_decode_gqa_fp8_empty_row_is_zero(splits):
    q, _, pools, rows, ln, ref, tol = _case(3, 128, 2, 0, (9, 37, 5, 150, 2))
    ln = ln.clone()
    dead = [0, 3]
    ln[dead] = 0
    out = _ext().ragged_decode_gqa_fp8(q, *pools, rows, ln, 0, 0, splits)
    live = [1, 2, 4]
    assert_within(out[live], ref[live], tol[live], f"splits={splits}")
    assert torch.count_nonzero(bits(out[dead])) == 0


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_decode_gqa_fp8_and_ragged_decode_fp8_share_the_bound(G, D):
    """One reference, each kernel with its own units (kv_fp8_refs)."""
    q, _, pools, rows, ln, ref, tol = _case(G, D, 2)
    assert_within(_ext().ragged_decode_gqa_fp8(q, *pools, rows, ln), ref, tol,
                  "ragged_decode_gqa_fp8")
    tol_old = _case(G, D, 2, units=UNITS_DECODE)[6]
    assert_within(_ext().ragged_decode_fp8(q, *pools, rows, ln), ref, tol_old,
                  "ragged_decode_fp8")


def test_decode_gqa_fp8_rejects_bad_arguments():
    """Pools and scales are leading views of larger buffers and every bad
    tensor is at least as large as the good one: indexing would stay in
    allocated memory even without the checks."""
    f = _ext().ragged_decode_gqa_fp8
    n, Hk, G, D, B, Smax = 3, 2, 3, 64, 4, 16

    def codes(*shape):
        return torch.zeros(*shape, device=DEV, dtype=torch.uint8).view(FP8)

    kbuf, vbuf = codes(B + 2, Smax, Hk, D), codes(B + 2, Smax, Hk, D)
    sbuf = torch.ones(B + 2, Smax, Hk, device=DEV)
    kp, vp, sc = kbuf[:B], vbuf[:B], sbuf[:B]
    q = torch.zeros(n, 1, Hk * G, D, device=DEV, dtype=BF)
    rows = torch.tensor([2, 0, 1], device=DEV)
    lens = torch.tensor([5, 16, 1], device=DEV)
    f(q, kp, vp, sc, sc, rows, lens, 4, Smax, 2)            # the good call
    q33 = torch.zeros(n, 1, 33, D, device=DEV, dtype=BF)
    k1, s1 = codes(B + 2, Smax, 1, D)[:B], sbuf[:B, :, :1].contiguous()
    long2 = torch.zeros(2 * n, dtype=torch.long, device=DEV)
    wide = codes(B, Smax, Hk, 256)
    bad = {
        "G = 33": lambda: f(q33, k1, k1, s1, s1, rows, lens),
        "window -1": lambda: f(q, kp, vp, sc, sc, rows, lens, -1),
        "max_len > Smax": lambda: f(q, kp, vp, sc, sc, rows, lens, 0,
                                    Smax + 1),
        "lens.max() > Smax": lambda: f(
            q, kp, vp, sc, sc, rows,
            torch.tensor([5, Smax + 1, 1], device=DEV)),
        "splits -1": lambda: f(q, kp, vp, sc, sc, rows, lens, 0, 0, -1),
        "head_dim 256": lambda: f(
            torch.zeros(n, 1, Hk * G, 256, device=DEV, dtype=BF), wide, wide,
            sc, sc, rows, lens),
        "vpool shape": lambda: f(q, kp, vbuf, sc, sc, rows, lens),
        "q dtype": lambda: f(q.float(), kp, vp, sc, sc, rows, lens),
        "kpool dtype": lambda: f(q, kp.to(BF), vp, sc, sc, rows, lens),
        "vpool dtype": lambda: f(q, kp, vp.view(torch.uint8), sc, sc, rows,
                                 lens),
        "k_scale shape": lambda: f(q, kp, vp, sbuf, sc, rows, lens),
        "k_scale dtype": lambda: f(q, kp, vp, sc.double(), sc, rows, lens),
        "v_scale dtype": lambda: f(q, kp, vp, sc, sc.to(BF), rows, lens),
        "k_scale device": lambda: f(q, kp, vp, sc.cpu(), sc, rows, lens),
        "rows int32": lambda: f(q, kp, vp, sc, sc, rows.int(), lens),
        "lens int32": lambda: f(q, kp, vp, sc, sc, rows, lens.int()),
        "lens length": lambda: f(q, kp, vp, sc, sc, rows, long2[:n + 1]),
        "q strided": lambda: f(
            torch.zeros(n, 1, Hk * G, 2 * D, device=DEV, dtype=BF)[..., :D],
            kp, vp, sc, sc, rows, lens),
        "kpool misaligned": lambda: f(
            q, codes(B * Smax * Hk * D + 8)[8:].view(B, Smax, Hk, D), vp, sc,
            sc, rows, lens),
        "kpool strided": lambda: f(q, wide[..., :D], vp, sc, sc, rows, lens),
        "rows strided": lambda: f(q, kp, vp, sc, sc, long2[::2], lens),
        "rows device": lambda: f(q, kp, vp, sc, sc, rows.cpu(), lens),
        "kpool device": lambda: f(q, kbuf.cpu()[:B], vp, sc, sc, rows, lens),
    }
    for name, call in bad.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"'{name}' did not raise")


@pytest.mark.parametrize("heads,window", [((6, 2), None), ((4, 2), 16)])
def test_decode_gqa_fp8_engine_gpu(monkeypatch, heads, window):
    """2-layer bf16 llama, head_dim 64, fp8 pool: G = 3, and sliding_window 16
    with prompts past it. Bookkeeping, the kernel's call count and what
    reaches it are exact; the greedy-token agreement with the bf16-pool
    engine is printed, not asserted (nobody has measured it)."""
    import deepspeed_amd.models.llama as llama
    from deepspeed_amd.inference.serving import ContinuousBatchingEngine

    cfg = llama.LlamaConfig(hidden_size=64 * heads[0], intermediate_size=688,
                            num_hidden_layers=2, num_attention_heads=heads[0],
                            num_key_value_heads=heads[1], vocab_size=2048,
                            max_position_embeddings=512,
                            activation_checkpointing=False,
                            sliding_window=window)
    assert cfg.head_dim == 64
    torch.manual_seed(0)
    model = llama.LlamaForCausalLM(cfg).to(DEV, BF).eval()
    torch.manual_seed(1)
    prompts = [torch.randint(0, 2000, (n,)) for n in (20, 40, 27, 70)]
    new = 8

    def run(kv_dtype):
        cb = ContinuousBatchingEngine(model, max_batch=2, prefill_chunk=16,
                                      fused_kv_append=True, kv_dtype=kv_dtype)
        rids = [cb.add_request(p, max_new_tokens=new) for p in prompts]
        return cb, rids, cb.run()

    _, ref_rids, ref_out = run(None)

    calls = {"kernel": 0, "decode": 0}
    real_kernel = _ext().ragged_decode_gqa_fp8
    real_decode = ContinuousBatchingEngine._decode

    def kernel(*a):
        calls["kernel"] += 1
        assert a[7] == (window or 0) and 0 < a[8] <= 512, a[7:]
        return real_kernel(*a)

    def decode(self, active):
        calls["decode"] += 1
        return real_decode(self, active)

    monkeypatch.setattr(_ext(), "ragged_decode_gqa_fp8", kernel)
    monkeypatch.setattr(ContinuousBatchingEngine, "_decode", decode)
    cb, rids, out = run("fp8")

    assert sorted(cb.free_slots) == [0, 1]
    assert not cb.running and not cb.pending and not cb.prefilling
    assert calls["decode"] >= new - 1
    assert calls["kernel"] == calls["decode"] * cfg.num_hidden_layers
    for rid, p in zip(rids, prompts):
        assert len(out[rid]) == len(p) + new, rid
        assert torch.equal(out[rid][:len(p)], p), rid
    agree = [float((out[a] == ref_out[b]).float().mean())
             for a, b in zip(rids, ref_rids)]
    print(f"greedy agreement fp8 pool vs bf16 pool (heads={heads}, "
          f"window={window}, reported, not asserted): "
          f"{sum(agree) / len(agree):.3f}")
