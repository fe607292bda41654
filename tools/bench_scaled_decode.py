"""Per-token-scaled fp8 against plain fp8: the paged decode step.

The shapes and the method of tools/bench_paged_decode.py: Hkv = 8, G = 4
(Hq = 32), D = 128, B = 8, world size 1, page 256, the "uniform" mix (eight
sequences at 32K) and the "skewed" mix (one at 128K, seven at 4K). One
decode step = append one token to every sequence + attend, replayed from
PagedDecodeSession.graphed_step. Variants:

  fp8          kv_dtype="fp8": torch casts the new rows, the append kernel
               copies bytes, fa_fwd_fp8_kernel multiplies raw e4m3
  fp8_scaled   kv_dtype="fp8_scaled": the append kernel quantizes bf16 rows
               and stores their scales; the decode kernel streams 8 more
               bytes per 256 payload bytes, carries PV under a second
               running max and feeds P as two e4m3 terms

Both run the same split plan over the same capacity, in ONE process,
alternating, each twice (the difference between a variant's two windows is
the run-to-run spread); every window is warmed up and timed with a host
clock around work that ends in a device synchronise; the default step count
makes a window 0.4 to 1.1 s. Prints one JSON line; needs a GPU.

Usage: python tools/bench_scaled_decode.py [--steps 3000] [--warmup 20]
           [--page 256] [--mixes uniform,skewed]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tree_attention_torch_amd.session import PagedDecodeSession  # noqa: E402

B, HKV, G, D = 8, 8, 4, 128
HQ = HKV * G
BLOCK = 256
MIXES = {
    "uniform": (32768,) * 8,
    "skewed": (131072,) + (4096,) * 7,
}
DTYPES = ("fp8", "fp8_scaled")


def _randn(*shape):
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16)


def _variants(lengths, margin, page):
    """kv_dtype -> graphed step over a freshly prefilled session."""
    q = _randn(B, HQ, 1, D)
    k_new, v_new = _randn(B, HKV, 1, D), _randn(B, HKV, 1, D)
    cap = max(lengths) + margin
    pool_tokens = sum(-(-(n + margin) // page) * page for n in lengths)
    sessions = {dt: PagedDecodeSession(B, HKV, D, cap, pool_tokens, page,
                                       "cuda", dt, BLOCK) for dt in DTYPES}
    for b, n in enumerate(lengths):
        k, v = _randn(HKV, n, D), _randn(HKV, n, D)
        for s in sessions.values():
            s.prefill(b, k, v)
    return {dt: s.graphed_step(q, k_new, v_new) for dt, s in sessions.items()}


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--mixes", default="uniform,skewed")
    ap.add_argument("--page", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_scaled_decode: needs a GPU")
    torch.manual_seed(0)
    rounds = 2
    margin = rounds * (args.steps + args.warmup) + 4 * BLOCK
    result = {"bench": "scaled_decode", "B": B, "Hq": HQ, "Hkv": HKV, "D": D,
              "page": args.page, "steps": args.steps, "warmup": args.warmup,
              "unit": "us/step", "mixes": {}}
    for name in args.mixes.split(","):
        lengths = MIXES[name]
        variants = _variants(lengths, margin, args.page)
        windows = {v: [] for v in variants}
        for _ in range(rounds):             # every variant, then again
            for v, fn in variants.items():
                windows[v].append(round(_time(fn, args.steps, args.warmup), 2))
        result["mixes"][name] = {
            "lengths": list(lengths),
            "us": windows,
            "spread_pct": {v: round(abs(w[0] - w[1]) / min(w) * 100, 1)
                           for v, w in windows.items()},
            "scaled_over_fp8": round(min(windows["fp8_scaled"]) /
                                     min(windows["fp8"]), 3),
        }
        del variants
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
