"""`ragged_decode_gqa`, the MFMA split-KV decode kernel (needs MI355X):
elementwise against ragged_prefill_refs.ragged_prefill_ref (float64, derived
bound) on decode sequences (slot, i, 1, L).

Under a window W the reference sees a pool that holds each row's positions
[L-W', L), W' = min(W, L), copied to 0..W'; the kernel's pool is NaN below
L-W', from L up and in unnamed slots, and V carries the sentinel at L-1 and at
L-W': a read outside the band or a dropped edge of it fails the comparison."""
import functools

import pytest
import torch

from attn_refs import SENT
from edge_refs import assert_within
from ragged_prefill_refs import (N_SLOTS, SMAX, make_ragged_prefill,
                                 ragged_prefill_ref)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF = torch.bfloat16
# around the 32-key tile and the 128-key round (one tile per wave)
LENS = [1, 2, 31, 32, 33, 127, 128, 129, 257, 300]
WINDOWS = [0, 1, 5, 33, 128, 1000]
SPLITS = [1, 3, 0]


def _ext():
    return get_ext(required=True)


@functools.lru_cache(maxsize=None)
def _case(G, D, Hk, window=0, lens=tuple(LENS)):
    """q [n,Hq,D], the kernel's pools, rows, lens and the float64 reference
    in row order; shared, callers must not modify them."""
    q, kp, vp, seqs = make_ragged_prefill([(1, L) for L in lens], G, D, Hk,
                                          device=DEV, poison=True)
    rk, rv = kp.clone(), vp.clone()
    rseqs = []
    for slot, q_start, _, L in seqs:
        w = min(window, L) if window > 0 else L
        vp[slot, L - w] = SENT
        rk[slot, :w], rv[slot, :w] = kp[slot, L - w:L], vp[slot, L - w:L]
        kp[slot, :L - w] = float("nan")
        vp[slot, :L - w] = float("nan")
        rseqs.append((slot, q_start, 1, w))
    ref = ragged_prefill_ref(q, rk, rv, rseqs)
    order = torch.tensor([s[1] for s in seqs], device=DEV)
    rows = torch.tensor([s[0] for s in seqs], device=DEV)
    ln = torch.tensor([s[3] for s in seqs], device=DEV)
    return (q[order].contiguous(), kp, vp, rows, ln, ref["out"][order],
            ref["tol"][order])


@pytest.mark.parametrize("Hk", [1, 2])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [1, 3, 7, 8, 16, 32])
def test_decode_gqa_vs_float64(G, D, Hk):
    """Every window and split count; max_len only sizes the grid, so the
    output with max_len = Smax is bit-identical to the one that reads
    lens.max()."""
    for window in WINDOWS:
        q, kp, vp, rows, ln, ref, tol = _case(G, D, Hk, window)
        for splits in SPLITS:
            out = _ext().ragged_decode_gqa(q, kp, vp, rows, ln, window, 0,
                                           splits)
            assert out.shape == (len(LENS), 1, G * Hk, D)
            assert_within(out, ref, tol, f"window={window} splits={splits}")
            out2 = _ext().ragged_decode_gqa(q, kp, vp, rows, ln, window,
                                            SMAX, splits)
            assert torch.equal(out.view(torch.int16), out2.view(torch.int16))


@pytest.mark.parametrize("splits", SPLITS)
def test_decode_gqa_empty_row_is_zero(splits):
    q, kp, vp, rows, ln, ref, tol = _case(3, 128, 2, 0, (9, 37, 5, 150, 2))
    ln = ln.clone()
    dead = [0, 3]
    ln[dead] = 0
    out = _ext().ragged_decode_gqa(q, kp, vp, rows, ln, 0, 0, splits)
    live = [1, 2, 4]
    assert_within(out[live], ref[live], tol[live], f"splits={splits}")
    assert torch.count_nonzero(out[dead].view(torch.int16)) == 0


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("G", [1, 2, 4, 8])
def test_decode_gqa_and_ragged_decode_share_the_bound(G, D):
    q, kp, vp, rows, ln, ref, tol = _case(G, D, 2)
    assert_within(_ext().ragged_decode_gqa(q, kp, vp, rows, ln), ref, tol,
                  "ragged_decode_gqa")
    assert_within(_ext().ragged_decode(q, kp, vp, rows, ln), ref, tol,
                  "ragged_decode")


def test_decode_gqa_rejects_bad_arguments():
    """Pools are leading views of larger buffers and every bad tensor is at
    least as large as the good one: indexing would stay in allocated memory
    even without the checks."""
    f = _ext().ragged_decode_gqa
    n, Hk, G, D, B, Smax = 3, 2, 3, 64, 4, 16
    kbuf = torch.zeros(B + 2, Smax, Hk, D, device=DEV, dtype=BF)
    vbuf = torch.zeros(B + 2, Smax, Hk, D, device=DEV, dtype=BF)
    kp, vp = kbuf[:B], vbuf[:B]
    q = torch.zeros(n, 1, Hk * G, D, device=DEV, dtype=BF)
    rows = torch.tensor([2, 0, 1], device=DEV)
    lens = torch.tensor([5, 16, 1], device=DEV)
    f(q, kp, vp, rows, lens, 4, Smax, 2)                    # the good call
    q33 = torch.zeros(n, 1, 33, D, device=DEV, dtype=BF)
    k1 = torch.zeros(B + 2, Smax, 1, D, device=DEV, dtype=BF)[:B]
    long2 = torch.zeros(2 * n, dtype=torch.long, device=DEV)
    wide = torch.zeros(B, Smax, Hk, 256, device=DEV, dtype=BF)
    bad = {
        "G = 33": lambda: f(q33, k1, k1, rows, lens),
        "window -1": lambda: f(q, kp, vp, rows, lens, -1),
        "max_len > Smax": lambda: f(q, kp, vp, rows, lens, 0, Smax + 1),
        "lens.max() > Smax": lambda: f(
            q, kp, vp, rows, torch.tensor([5, Smax + 1, 1], device=DEV)),
        "splits -1": lambda: f(q, kp, vp, rows, lens, 0, 0, -1),
        "head_dim 256": lambda: f(
            torch.zeros(n, 1, Hk * G, 256, device=DEV, dtype=BF), wide, wide,
            rows, lens),
        "vpool shape": lambda: f(q, kp, vbuf, rows, lens),
        "q dtype": lambda: f(q.float(), kp, vp, rows, lens),
        "kpool dtype": lambda: f(q, kp.float(), vp, rows, lens),
        "vpool dtype": lambda: f(q, kp, vp.float(), rows, lens),
        "rows int32": lambda: f(q, kp, vp, rows.int(), lens),
        "lens int32": lambda: f(q, kp, vp, rows, lens.int()),
        "lens length": lambda: f(q, kp, vp, rows, long2[:n + 1]),
        "q strided": lambda: f(
            torch.zeros(n, 1, Hk * G, 2 * D, device=DEV, dtype=BF)[..., :D],
            kp, vp, rows, lens),
        "kpool strided": lambda: f(q, wide[..., :D], vp, rows, lens),
        "rows strided": lambda: f(q, kp, vp, long2[::2], lens),
        "rows device": lambda: f(q, kp, vp, rows.cpu(), lens),
        "lens device": lambda: f(q, kp, vp, rows, lens.cpu()),
        "kpool device": lambda: f(q, kbuf.cpu()[:B], vp, rows, lens),
    }
    for name, call in bad.items():
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"'{name}' did not raise")


def _greedy_no_cache(model, prompt, new):
    ids = prompt.view(1, -1).to(DEV)
    for _ in range(new):
        nxt = model(ids)[0, -1].float().argmax()
        ids = torch.cat([ids, nxt.view(1, 1)], dim=1)
    return ids[0]


@pytest.mark.parametrize("heads,window", [((6, 2), None), ((4, 2), 16)])
def test_decode_gqa_engine_gpu(monkeypatch, heads, window):
    """2-layer bf16 llama, head_dim 64: G = 3, and sliding_window 16 with
    prompts past it. Agreement criterion of test_fused_step_engine_gpu (bf16
    argmax ties break differently between batched shapes) against a no-cache
    recompute; bookkeeping and the kernel's call count are exact."""
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
    with torch.no_grad():
        refs = [_greedy_no_cache(model, p, new) for p in prompts]

    calls = {"kernel": 0, "decode": 0}
    real_kernel = _ext().ragged_decode_gqa
    real_decode = ContinuousBatchingEngine._decode

    def kernel(*a):
        calls["kernel"] += 1
        assert a[5] == (window or 0) and 0 < a[6] <= 512, a[5:]
        return real_kernel(*a)

    def decode(self, active):
        calls["decode"] += 1
        return real_decode(self, active)

    monkeypatch.setattr(_ext(), "ragged_decode_gqa", kernel)
    monkeypatch.setattr(ContinuousBatchingEngine, "_decode", decode)
    cb = ContinuousBatchingEngine(model, max_batch=2, prefill_chunk=16)
    rids = [cb.add_request(p, max_new_tokens=new) for p in prompts]
    out = cb.run()

    assert sorted(cb.free_slots) == [0, 1]
    assert not cb.running and not cb.pending and not cb.prefilling
    assert calls["decode"] >= new - 1
    assert calls["kernel"] == calls["decode"] * cfg.num_hidden_layers
    for rid, ref, p in zip(rids, refs, prompts):
        assert len(out[rid]) == len(p) + new, rid
        assert torch.equal(out[rid][:len(p)], p), rid
        agree = (out[rid].to(DEV) == ref).float().mean().item()
        assert agree >= 0.75, (rid, agree)
