"""fp8 KV slot pool on the GPU (needs MI355X): the three *_fp8 HIP kernels
and the engine with kv_dtype="fp8", against the float64 references and the
derived bounds of kv_fp8_refs (proved valid and sharp in test_kv_fp8_cpu).

Dispatch arms reached:
  ragged_rope_append_fp8_kernel<64> / <128>   4 / 8 lanes per row butterfly,
      Hq/Hk in {1, 4}; T in {1, 7, 300}: one lane group / tail / two blocks;
      with / without lens; slot -1 / B, pos -1 / Smax / P (device guard);
      identity table (K bit-exact) and random table (K within the bound)
  ragged_decode_fp8_kernel<D, G>   D in {64, 128} (8 / 4 row groups per
      wave), G in {1, 2, 4, 8}; chunk 4 / 8 / 512: multi-chunk rows, empty
      chunks, NS capped at 64, one chunk; row groups with no position
  ragged_prefill_fp8_kernel<D>     the mixed / lone / decode batches: q tiles
      and kv tiles on both sides of 32 / 64, chunks over a cached prefix
  every attention case twice: NaN codes and NaN scales past each slot's
      length must not change a bit of the output
"""
import pytest
import torch

from attn_refs import RAGGED_CHUNKS, RAGGED_SHAPES
from edge_refs import assert_within
from kv_fp8_refs import (FP8, check_append_fp8, check_engine, decode_case,
                         pool_pattern, prefill_case)
from ragged_prefill_refs import BATCHES
from ragged_rope_append_refs import (POOL, SEQS, SEQS_T1, SKIP_EDITS,
                                     SKIP_POOL, SKIP_SEQS, bits, make_inputs)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from deepspeed_amd.ops.loader import get_ext

DEV = "cuda:0"
BF = torch.bfloat16
APPEND_SHAPES = [(Hq, Hk, D) for D in (64, 128) for Hq, Hk in
                 ((1, 1), (4, 1), (4, 4))]
PREFILL_SHAPES = [(4, 64, 2), (1, 128, 1), (2, 128, 2), (8, 64, 1)]


def _ext():
    return get_ext(required=True)


def _dev(ts):
    return tuple(t.to(DEV) for t in ts)


# ---------------------------------------------------------------- append
def _append(seqs, B, Smax, P, Hq, Hk, D, identity, edits=(), with_lens=True):
    from deepspeed_amd.inference.ragged_batch import RaggedBatch
    b = RaggedBatch(seqs, B, Smax, DEV)
    slot, pos = b.tok_slot, b.tok_pos
    if edits:
        slot, pos = slot.clone(), pos.clone()
        for which, t, val in edits:
            (slot if which == "slot" else pos)[t] = val
    q, k, v, cos, sin = make_inputs(b.total_tokens, Hq, Hk, D, P, BF, DEV)
    k[0, 0] = 0                                  # all-zero rows
    v[-1, Hk - 1] = 0
    if identity:
        cos, sin = torch.ones_like(cos), torch.zeros_like(sin)
    # pools and scales are interior views of larger pattern buffers (two
    # slots of room on both sides): a stray write fails a bit compare
    kbuf, ksbuf = pool_pattern(B + 4, Smax, Hk, D, DEV, 1)
    vbuf, vsbuf = pool_pattern(B + 4, Smax, Hk, D, DEV, 2)
    bufs = (kbuf, vbuf, ksbuf, vsbuf)
    pools = tuple(t[2:2 + B] for t in bufs)
    assert all(t.is_contiguous() for t in pools)
    lbuf = torch.arange(98, 98 + B + 4, device=DEV)
    lens = lbuf[2:2 + B]
    snap = [t.clone() for t in (q, k, v) + bufs + (lbuf,)]
    what = f"D={D} Hq={Hq} Hk={Hk} T={b.total_tokens}"
    out = _ext().ragged_rope_append_fp8(q, k, v, cos, sin, slot, pos, *pools,
                                        lens if with_lens else None)
    torch.cuda.synchronize()
    for name, t, t0 in zip(("q", "k", "v"), (q, k, v), snap):
        assert torch.equal(bits(t), bits(t0)), f"{what}: {name} modified"
    for t, t0 in zip(bufs + (lbuf,), snap[3:]):
        u, u0 = (t.view(torch.uint8), t0.view(torch.uint8)) \
            if t.dtype == FP8 else (t, t0)
        assert torch.equal(u[:2], u0[:2]) and \
            torch.equal(u[2 + B:], u0[2 + B:]), \
            f"{what}: buffer changed outside the view"
    if not with_lens:
        assert torch.equal(lbuf, snap[7]), f"{what}: lens written"
    check_append_fp8(out, q, k, v, cos, sin, slot, pos, pools,
                     tuple(t[2:2 + B] for t in snap[3:7]),
                     lens if with_lens else None, snap[7][2:2 + B], what,
                     identity)
    return out, lens


@pytest.mark.parametrize("identity", [True, False])
@pytest.mark.parametrize("Hq,Hk,D", APPEND_SHAPES)
def test_append_kernel(Hq, Hk, D, identity):
    """V and identity-table K bit-exact against kv_quantize; random-table K
    within the derived bound; rows not named bitwise unchanged."""
    for T in (1, 7, 300):
        B, Smax, P = POOL[T]
        for seqs in (SEQS_T1 if T == 1 else [SEQS[T]]):
            _, lens = _append(seqs, B, Smax, P, Hq, Hk, D, identity)
            for slot, _, _, kv_len in seqs:
                assert int(lens[slot]) == kv_len
    _append(SEQS[7], *POOL[7], Hq, Hk, D, identity, with_lens=False)


@pytest.mark.parametrize("D", [64, 128])
def test_append_kernel_skip_rule(D):
    B, Smax, P = SKIP_POOL
    _append(SKIP_SEQS, B, Smax, P, 4, 2, D, False, edits=SKIP_EDITS)


def test_kernels_reject_bad_arguments():
    """Every bad tensor is at least as large as the good one."""
    e = _ext()
    T, Hq, Hk, D, B, Smax, P = 6, 4, 2, 64, 4, 16, 32
    q, k, v, cos, sin = make_inputs(T, Hq, Hk, D, P, BF, DEV)
    kp = torch.zeros(B, Smax, Hk, D, device=DEV, dtype=torch.uint8).view(FP8)
    sc = torch.ones(B, Smax, Hk, device=DEV)
    slot = torch.tensor([2, 2, 2, 0, 3, 1], device=DEV)
    pos = torch.tensor([0, 1, 2, 15, 7, 3], device=DEV)
    good = dict(q=q, k=k, v=v, cos=cos, sin=sin, tok_slot=slot, tok_pos=pos,
                kpool=kp, vpool=kp.clone(), k_scale=sc, v_scale=sc.clone())
    e.ragged_rope_append_fp8(**good)                        # the good call
    q32 = torch.zeros(T, Hq, 32, device=DEV, dtype=BF)
    bad = {
        "bf16 pool": dict(kpool=torch.zeros(B, Smax, Hk, D, device=DEV,
                                            dtype=BF)),
        "uint8 pool": dict(vpool=torch.zeros(B, Smax, Hk, D, device=DEV,
                                             dtype=torch.uint8)),
        "scale dtype": dict(k_scale=sc.double()),
        "scale shape": dict(v_scale=torch.ones(B, Smax, Hk, 2, device=DEV)),
        "scale device": dict(k_scale=sc.cpu()),
        "head_dim 32": dict(
            q=q32, k=q32[:, :Hk].contiguous(), v=q32[:, :Hk].contiguous(),
            cos=torch.ones(P, 16, device=DEV), sin=torch.ones(P, 16,
                                                              device=DEV),
            kpool=torch.zeros(B, Smax, Hk, 32, device=DEV,
                              dtype=torch.uint8).view(FP8),
            vpool=torch.zeros(B, Smax, Hk, 32, device=DEV,
                              dtype=torch.uint8).view(FP8)),
    }
    for name, change in bad.items():
        with pytest.raises(RuntimeError):
            e.ragged_rope_append_fp8(**{**good, **change})
            pytest.fail(f"'{name}' did not raise")
    qd = torch.zeros(3, 1, Hq, D, device=DEV, dtype=BF)
    rows = torch.tensor([2, 0, 1], device=DEV)
    lens = torch.tensor([5, 16, 1], device=DEV)
    e.ragged_decode_fp8(qd, kp, kp, sc, sc, rows, lens, 4)  # the good calls
    desc = torch.tensor([[2, 0, 3, 5], [0, 3, 3, 16]], device=DEV)
    e.ragged_prefill_fp8(q, kp, kp, sc, sc, desc, 3, 16)
    bf_pool = torch.zeros(B, Smax, Hk, D, device=DEV, dtype=BF)
    for call in (
            lambda: e.ragged_decode_fp8(qd, bf_pool, bf_pool, sc, sc, rows,
                                        lens, 4),
            lambda: e.ragged_decode_fp8(qd, kp, kp, sc[:, :, :1].contiguous(),
                                        sc, rows, lens, 4),
            lambda: e.ragged_decode_fp8(qd, kp, kp, sc, sc, rows,
                                        torch.tensor([5, Smax + 1, 1],
                                                     device=DEV), 4),
            lambda: e.ragged_prefill_fp8(q, bf_pool, bf_pool, sc, sc, desc,
                                         3, 16),
            lambda: e.ragged_prefill_fp8(q, kp, kp, sc.half(), sc, desc, 3,
                                         16),
            lambda: e.ragged_prefill_fp8(q, kp, kp, sc, sc, desc, 3,
                                         Smax + 1)):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail("a bad call did not raise")


# ------------------------------------------------------ decode / prefill
@pytest.mark.parametrize("G,D,Hk", RAGGED_SHAPES)
def test_decode_kernel_vs_float64(G, D, Hk):
    for lens_name in ("A", "B"):
        c = decode_case(lens_name, G, D, Hk)
        q, rows, lens = _dev((c["q"], c["rows"], c["lens"]))
        clean, poisoned = _dev(c["clean"]), _dev(c["poisoned"])
        for chunk in RAGGED_CHUNKS:
            out = _ext().ragged_decode_fp8(q, *clean, rows, lens, chunk)
            assert_within(out, c["out"], c["tol"],
                          f"lens {lens_name} chunk={chunk}")
            again = _ext().ragged_decode_fp8(q, *poisoned, rows, lens, chunk)
            assert torch.equal(bits(out), bits(again)), \
                f"lens {lens_name} chunk={chunk}: NaN past a length leaked"


@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("G,D,Hk", PREFILL_SHAPES)
def test_prefill_kernel_vs_float64(name, G, D, Hk):
    from deepspeed_amd.inference.ragged_batch import RaggedBatch
    c = prefill_case(name, G, D, Hk)
    q = c["q"].to(DEV)
    clean, poisoned = _dev(c["clean"]), _dev(c["poisoned"])
    b = RaggedBatch(c["seqs"], clean[0].shape[0], clean[0].shape[1], DEV)
    out = _ext().ragged_prefill_fp8(q, *clean, b.desc, b.max_qlen,
                                    b.max_kvlen)
    assert_within(out, c["out"], c["tol"], name)
    again = _ext().ragged_prefill_fp8(q, *poisoned, b.desc, b.max_qlen,
                                      b.max_kvlen)
    assert torch.equal(bits(out), bits(again)), \
        f"{name}: NaN past a length leaked"


def test_functional_wrappers_dispatch_to_the_kernels(monkeypatch):
    """bf16 on the GPU goes through the HIP entry points, not the torch
    fallback."""
    from deepspeed_amd.inference.ragged_batch import RaggedBatch
    from deepspeed_amd.ops import functional as Fops
    calls = []
    for name in ("ragged_decode_fp8", "ragged_prefill_fp8"):
        real = getattr(_ext(), name)
        monkeypatch.setattr(
            _ext(), name,
            lambda *a, _r=real, _n=name, **kw: (calls.append(_n),
                                                _r(*a, **kw))[1])
    monkeypatch.setattr(Fops, "_ragged_prefill_torch",
                        lambda *a, **kw: pytest.fail("torch fallback ran"))
    c = decode_case("A", 4, 64, 2)
    out = Fops.ragged_decode_attention_fp8(
        c["q"].to(DEV), *_dev(c["clean"]), c["rows"].to(DEV),
        c["lens"].to(DEV), chunk=8)
    assert_within(out, c["out"], c["tol"], "wrapper decode")
    c = prefill_case("mixed", 4, 64, 2)
    clean = _dev(c["clean"])
    b = RaggedBatch(c["seqs"], clean[0].shape[0], clean[0].shape[1], DEV)
    out = Fops.ragged_prefill_attention_fp8(c["q"].to(DEV), *clean, b)
    assert_within(out, c["out"], c["tol"], "wrapper prefill")
    assert calls == ["ragged_decode_fp8", "ragged_prefill_fp8"]


# ---------------------------------------------------------------- engine
@pytest.mark.parametrize("fused_step", [True, False])
def test_engine_fp8_gpu(monkeypatch, fused_step):
    """Bookkeeping, pool format and layer 0 as on the CPU; the ragged steps
    of the fp8 engine go through the fp8 kernels."""
    calls = {}
    for name in ("ragged_rope_append_fp8", "ragged_decode_fp8",
                 "ragged_prefill_fp8"):
        real = getattr(_ext(), name)
        calls[name] = 0

        def spy(*a, _r=real, _n=name, **kw):
            calls[_n] += 1
            return _r(*a, **kw)

        monkeypatch.setattr(_ext(), name, spy)
    agree = check_engine(DEV, BF, fused_step)
    print(f"greedy agreement fp8 pool vs bf16 pool (fused_step={fused_step},"
          f" reported, not asserted): {agree:.3f}")
    assert calls["ragged_rope_append_fp8"] > 0
    assert calls["ragged_prefill_fp8" if fused_step
                 else "ragged_decode_fp8"] > 0
    assert calls["ragged_decode_fp8" if fused_step
                 else "ragged_prefill_fp8"] == 0
