"""Ragged decode HIP kernel vs fp32 reference (mixed sequence lengths)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _ref_decode(q, kpool, vpool, rows, lens):
    """fp32 per-row attention over each row's valid KV prefix."""
    n, _, Hq, D = q.shape
    Hk = kpool.shape[2]
    G = Hq // Hk
    outs = []
    for i in range(n):
        L = int(lens[i])
        s = int(rows[i])
        k = kpool[s, :L].float()                  # [L, Hk, D]
        v = vpool[s, :L].float()
        qi = q[i, 0].float()                      # [Hq, D]
        k = k.repeat_interleave(G, dim=1)
        v = v.repeat_interleave(G, dim=1)
        att = torch.einsum("hd,lhd->hl", qi, k) / math.sqrt(D)
        p = torch.softmax(att, dim=-1)
        outs.append(torch.einsum("hl,lhd->hd", p, v))
    return torch.stack(outs).unsqueeze(1)         # [n,1,Hq,D]


@pytest.mark.parametrize("D,G", [(128, 4), (128, 1), (64, 2), (128, 8)])
def test_ragged_decode_matches_reference(D, G):
    from deepspeed_amd.ops.loader import get_ext
    torch.manual_seed(0)
    Hk = 4
    Hq = Hk * G
    n, B, Smax = 5, 8, 700
    kpool = torch.randn(B, Smax, Hk, D, device="cuda", dtype=torch.bfloat16)
    vpool = torch.randn(B, Smax, Hk, D, device="cuda", dtype=torch.bfloat16)
    q = torch.randn(n, 1, Hq, D, device="cuda", dtype=torch.bfloat16)
    rows = torch.tensor([7, 2, 4, 0, 5], device="cuda")
    lens = torch.tensor([700, 1, 33, 512, 130], device="cuda")
    out = get_ext().ragged_decode(q, kpool, vpool, rows, lens)
    ref = _ref_decode(q, kpool, vpool, rows, lens)
    err = (out.float() - ref).abs().max().item()
    assert err < 3e-2, f"D={D} G={G}: max err {err}"


def test_ragged_decode_long_context_split():
    """Lengths spanning many split-KV chunks."""
    from deepspeed_amd.ops.loader import get_ext
    torch.manual_seed(1)
    D, Hk, G = 128, 8, 4
    Hq = Hk * G
    n, B, Smax = 3, 4, 8192
    kpool = torch.randn(B, Smax, Hk, D, device="cuda", dtype=torch.bfloat16)
    vpool = torch.randn(B, Smax, Hk, D, device="cuda", dtype=torch.bfloat16)
    q = torch.randn(n, 1, Hq, D, device="cuda", dtype=torch.bfloat16)
    rows = torch.tensor([0, 2, 3], device="cuda")
    lens = torch.tensor([8192, 4097, 640], device="cuda")
    out = get_ext().ragged_decode(q, kpool, vpool, rows, lens)
    ref = _ref_decode(q, kpool, vpool, rows, lens)
    err = (out.float() - ref).abs().max().item()
    assert err < 3e-2, f"max err {err}"


def test_serving_engine_uses_ragged_kernel():
    """Continuous-batching decode routes through the pool-direct kernel
    and generates the same tokens as the masked-SDPA fallback.

    Both paths greedy-decode a random-init bf16 model, whose top logits
    are frequently within a bf16 rounding step of each other, and one
    flipped tie used to change every later token of that request. So the
    fallback run is teacher-forced with the kernel run's tokens: every
    decode step of the two runs sees the same context, the fallback's own
    argmax is what gets compared, and wherever the two disagree the
    kernel's token must be a near-tie in the fallback's logits.
    Tie tolerance: logits are bf16 (8 significant bits), so at magnitude
    |l| their spacing is at most 2^-7*|l|; allowing 2 steps of rounding
    difference on each of the two logits compared gives 4 steps,
    i.e. max|logit| / 32.
    Since every step now sees the same context, the two paths' logits are
    also compared directly: at every step they must agree within that
    same 4-step allowance over the whole vocabulary (the paths differ only
    in the order of fp32 accumulation and one bf16 rounding of the
    attention output per layer)."""
    from deepspeed_amd.inference.serving import ContinuousBatchingEngine
    from deepspeed_amd.models.llama import LLAMA_CONFIGS, LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LLAMA_CONFIGS["llama-small"]  # head_dim 64 (tiny is 32)
    with torch.device("cuda"):
        model = LlamaForCausalLM(cfg).bfloat16().eval()

    def run(force_fallback, forced=None):
        eng = ContinuousBatchingEngine(model, max_batch=4)
        if force_fallback:
            for c in eng.caches:
                c._use_ragged = False
        else:
            assert all(c._use_ragged for c in eng.caches)
        own = {}        # rid -> this path's own greedy tokens
        margins = {}    # (rid, k) -> (max logit - logit of forced token, tol)
        seen = {}       # (rid, k) -> fp32 logits this path sampled from
        greedy = eng._sample

        def sample(logits, req):
            tok = greedy(logits, req)
            k = len(req.generated)
            own.setdefault(req.rid, []).append(tok)
            lf = logits.float()
            seen[(req.rid, k)] = lf.cpu()
            if forced is None:
                return tok
            margins[(req.rid, k)] = (float(lf.max() - lf[forced[req.rid][k]]),
                                     float(lf.abs().max()) / 32)
            return forced[req.rid][k]

        eng._sample = sample
        g = torch.Generator().manual_seed(3)
        prompts = {}
        for i in range(3):
            p = torch.randint(0, cfg.vocab_size, (8 + 3 * i,), generator=g)
            prompts[eng.add_request(p, max_new_tokens=12)] = p.tolist()
        out = eng.run()
        for rid in sorted(out):   # the engine returns prompt + what it fed
            fed = forced[rid] if forced is not None else own[rid]
            assert out[rid].tolist() == prompts[rid] + fed
        return [prompts[rid] + own[rid] for rid in sorted(out)], own, \
            margins, seen

    fast, fast_own, _, fast_logits = run(False)
    slow, slow_own, margins, slow_logits = run(True, forced=fast_own)
    flat_f = [t for rr in fast for t in rr]
    flat_s = [t for rr in slow for t in rr]
    assert len(flat_f) == len(flat_s) == 8 + 11 + 14 + 3 * 12
    same = sum(int(a == b) for a, b in zip(flat_f, flat_s))
    total = len(flat_f)
    ties = {key: margins[key] for key in margins
            if fast_own[key[0]][key[1]] != slow_own[key[0]][key[1]]}
    print(f"token agreement {same}/{total}; disagreements "
          f"(rid, step) -> (margin, tolerance): {ties}")
    assert sorted(fast_logits) == sorted(slow_logits)
    gaps = {key: (float((fast_logits[key] - slow_logits[key]).abs().max()),
                  float(slow_logits[key].abs().max()) / 32)
            for key in sorted(slow_logits)}
    worst = max(gaps, key=lambda key: gaps[key][0] / gaps[key][1])
    print(f"largest logit gap relative to its tolerance at (rid, step) "
          f"{worst}: {gaps[worst]}")
    assert same / total > 0.9, f"token agreement {same}/{total}"
    for key, (gap, tol) in gaps.items():
        assert gap <= tol, \
            f"request/step {key}: kernel and fallback logits differ by " \
            f"{gap} > {tol}"
    for key, (margin, tol) in ties.items():
        assert margin <= tol, \
            f"request/step {key}: kernel token is no near-tie for the " \
            f"fallback (logit margin {margin} > {tol})"
