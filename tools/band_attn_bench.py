#!/usr/bin/env python3
"""Banded causal flash attention against the plain causal kernels.

Times with device events, ms per call as median [min-max] of --iters calls
after a warm-up, the forward (`flash_attn_fwd`) and the whole backward
(`flash_attn_bwd`: pre-pass, pass 1, pass 2) at B 1, --hq/--hk heads, D --d:
the plain causal kernels, and with --window W > 0 the BAND kernels on the
same inputs, next to the ratio of key tiles / q steps the band visits,
counted from the shapes as the kernels count them. --sdpa adds what a user
had before: SDPA forward + backward with the dense boolean band mask.
Per-kernel times come from running this under a kernel trace.
"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def bench(fn, iters, warmup=5):
    for _ in range(warmup):
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
    return f"{statistics.median(times):8.3f} [{min(times):.3f}-{max(times):.3f}]"


def visited(S, W):
    """(plain, band) counts of forward 64-key tiles per 256-row block, pass 2
    32-key steps per 128-row block, pass 1 32-row steps per 64-key block."""
    up = lambda x, m: (x + m - 1) // m                      # noqa: E731
    lo = lambda i: max(0, i - W + 1)                        # noqa: E731
    hi = lambda j: min(S, j + W)                            # noqa: E731
    out = []
    for rows, step in ((256, 64), (128, 32)):
        ends = [up(min(S, b + rows), step) for b in range(0, S, rows)]
        out.append((sum(ends), sum(e - lo(b) // step for e, b in
                                   zip(ends, range(0, S, rows)))))
    out.append((sum(up(S - b, 32) for b in range(0, S, 64)),
                sum(up(min(S, up(hi(min(b + 63, S - 1)), 32) * 32) - b, 32)
                    for b in range(0, S, 64))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--s", type=int, default=4096)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--hq", type=int, default=32)
    ap.add_argument("--hk", type=int, default=8)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sdpa", action="store_true")
    a = ap.parse_args()
    S, W, D = a.s, a.window, a.d
    torch.manual_seed(0)
    bf = dict(device="cuda", dtype=torch.bfloat16)
    q = torch.randn(1, S, a.hq, D, **bf)
    k = torch.randn(1, S, a.hk, D, **bf)
    v = torch.randn(1, S, a.hk, D, **bf)
    g = torch.randn(1, S, a.hq, D, **bf)
    scale = 1.0 / math.sqrt(D)
    from deepspeed_amd.ops.loader import get_ext
    ext = get_ext(required=True)
    print(f"B 1 S {S} Hq {a.hq} Hk {a.hk} D {D} causal, window {W}, "
          f"{a.iters} calls, ms median [min-max]")

    def pair(name, band):
        out, lse = ext.flash_attn_fwd(q, k, v, True, scale, None, *band)
        print(f"{name} fwd", bench(lambda: ext.flash_attn_fwd(
            q, k, v, True, scale, None, *band), a.iters))
        print(f"{name} bwd", bench(lambda: ext.flash_attn_bwd(
            q, k, v, g, out, lse, True, scale, None, None, None, *band),
            a.iters))

    pair("plain", ())
    if W <= 0:
        return
    from deepspeed_amd.ops.attention import _band_bounds, _band_mask
    band = _band_bounds(1, S, W, None, q.device)
    pair("band ", band)
    for name, (p, b) in zip(("fwd tiles", "pass 2 steps", "pass 1 steps"),
                            visited(S, W)):
        print(f"{name}: plain {p} band {b} ratio {b / p:.3f}")
    if a.sdpa:
        import torch.nn.functional as F
        mask = _band_mask(band[0])
        ql, kl, vl = (t.transpose(1, 2).detach().requires_grad_(True)
                      for t in (q, k, v))

        def sdpa():
            F.scaled_dot_product_attention(
                ql, kl, vl, attn_mask=mask,
                enable_gqa=True).backward(g.transpose(1, 2))
            ql.grad = kl.grad = vl.grad = None
        print("sdpa dense band mask fwd+bwd", bench(sdpa, max(5, a.iters // 10)))


if __name__ == "__main__":
    main()
