#!/usr/bin/env python3
"""Attention microbenchmark for the HIP flash kernels.

Times, with device events:
  - the forward kernel (`flash_attn_fwd`) against torch SDPA,
  - forward + backward through autograd against torch SDPA,
  - the backward alone: the call into `flash_attn_bwd` and nothing else
    (pre-pass + dK/dV pass + dQ pass), min and median over AB_ITERS calls.

The backward rate is printed twice: as EXECUTED work, 7 MFMA products (S and
dP are recomputed in both passes), and as the ALGORITHMIC 5 products of a
flash backward. One product is 2*B*Hq*S*S*D FLOP, halved under the causal
mask.

Environment: AB_B (1), AB_S (4096), AB_D (128), AB_HQ (32), AB_HK (8),
AB_CAUSAL (1), AB_ITERS (20, at least 20 are run), AB_BWD_ONLY (0: set to 1
to skip the forward and SDPA timings), AB_FWD_ONLY (0: set to 1 to time
`flash_attn_fwd` alone, min and median, and nothing else).
"""
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

B = int(os.environ.get("AB_B", 1))
S = int(os.environ.get("AB_S", 4096))
D = int(os.environ.get("AB_D", 128))
Hq = int(os.environ.get("AB_HQ", 32))
Hk = int(os.environ.get("AB_HK", 8))
CAUSAL = bool(int(os.environ.get("AB_CAUSAL", 1)))
ITERS = max(20, int(os.environ.get("AB_ITERS", 20)))
BWD_ONLY = bool(int(os.environ.get("AB_BWD_ONLY", 0)))
FWD_ONLY = bool(int(os.environ.get("AB_FWD_ONLY", 0)))
WARMUP = 5


def bench(fn, iters=ITERS):
    """Per-call device time in ms: (min, median)."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return min(times), statistics.median(times)


def main():
    torch.manual_seed(0)
    bf = dict(device="cuda", dtype=torch.bfloat16)
    q = torch.randn(B, S, Hq, D, requires_grad=True, **bf)
    k = torch.randn(B, S, Hk, D, requires_grad=True, **bf)
    v = torch.randn(B, S, Hk, D, requires_grad=True, **bf)
    g = torch.randn(B, S, Hq, D, **bf)
    scale = 1.0 / math.sqrt(D)

    from deepspeed_amd.ops.loader import get_ext
    ext = get_ext(required=True)
    product = 2.0 * B * Hq * S * S * D * (0.5 if CAUSAL else 1.0)
    print(f"shape: B {B} S {S} Hq {Hq} Hk {Hk} D {D} "
          f"{'causal' if CAUSAL else 'full'}, {ITERS} timed calls")

    if FWD_ONLY:
        with torch.no_grad():
            t_min, t_med = bench(
                lambda: ext.flash_attn_fwd(q, k, v, CAUSAL, scale))
        print(f"fwd only: min {t_min:8.3f} ms  median {t_med:8.3f} ms")
        print(f"fwd only: {2 * product / t_min / 1e9:7.1f} TF/s "
              f"(2 products), at min")
        return

    with torch.no_grad():
        out, lse = ext.flash_attn_fwd(q, k, v, CAUSAL, scale)
        t_min, t_med = bench(lambda: ext.flash_attn_bwd(
            q, k, v, g, out, lse, CAUSAL, scale, None))
    print(f"bwd only: min {t_min:8.3f} ms  median {t_med:8.3f} ms")
    print(f"bwd only: {7 * product / t_min / 1e9:7.1f} TF/s executed "
          f"(7 products)  {5 * product / t_min / 1e9:7.1f} TF/s algorithmic "
          f"(5 products), both at min")
    if BWD_ONLY:
        return

    import torch.nn.functional as F
    from deepspeed_amd.ops.attention import _FlashAttnFn
    qt, kt, vt = (t.transpose(1, 2) for t in (q, k, v))

    def sdpa():
        return F.scaled_dot_product_attention(qt, kt, vt, is_causal=CAUSAL,
                                              enable_gqa=True)

    with torch.no_grad():
        hip_f = bench(lambda: ext.flash_attn_fwd(q, k, v, CAUSAL, scale))
        sdpa_f = bench(sdpa)

    def hip_fb():
        _FlashAttnFn.apply(q, k, v, CAUSAL, scale).backward(g)
        q.grad = k.grad = v.grad = None

    def sdpa_fb():
        sdpa().backward(g.transpose(1, 2))
        q.grad = k.grad = v.grad = None

    hip_fb_t = bench(hip_fb)
    sdpa_fb_t = bench(sdpa_fb)
    print(f"fwd:      HIP min {hip_f[0]:8.3f} ms "
          f"({2 * product / hip_f[0] / 1e9:7.1f} TF/s)  "
          f"SDPA min {sdpa_f[0]:8.3f} ms "
          f"({2 * product / sdpa_f[0] / 1e9:7.1f} TF/s)")
    print(f"fwd+bwd:  HIP min {hip_fb_t[0]:8.3f} ms  "
          f"SDPA min {sdpa_fb_t[0]:8.3f} ms")


if __name__ == "__main__":
    main()
