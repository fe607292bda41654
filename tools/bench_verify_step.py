"""Cost of a speculative verify step against a plain decode step.

The shapes and the method of tools/bench_paged_decode.py: bf16 (or --dtype
fp8), Hkv = 8, G = 4 (Hq = 32), D = 128, B = 8 sequences at 32K tokens each
(--length), world size 1. Variants, over a slab (RaggedDecodeSession) and a
paged (PagedDecodeSession, --page) session each:

  T1   graphed_step replay: append one token per sequence + attend
  T2   graphed_step_many replay at T = 2: append two drafts + verify them
  T4   the same at T = 4 (G * T = 16: the full MFMA tile, one launch)

The step streams the whole KV once whatever T is, so in this bandwidth-bound
regime T = 4 is expected to cost about what T = 1 costs; this tool measures
it and asserts nothing. Every sequence grows by T tokens per step (every
draft accepted). All variants run in ONE process, alternating, each twice
(the difference between a variant's two windows is the run-to-run spread);
every window is warmed up, which also ramps the clocks, and timed with a
host clock around work that ends in a device synchronise. Prints one JSON
line; needs a GPU.

Usage: python tools/bench_verify_step.py [--steps 200] [--warmup 20]
           [--length 32768] [--page 256] [--dtype bf16]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tree_attention_torch_amd.session import (PagedDecodeSession,  # noqa: E402
                                              RaggedDecodeSession)

B, HKV, G, D = 8, 8, 4, 128
HQ = HKV * G
BLOCK = 256
TS = (1, 2, 4)


def _randn(*shape):
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16)


def _variants(length, margin, page, dtype):
    """name -> replay() of a captured step over a freshly prefilled
    session of its own."""
    cap = length + margin
    sessions = {}
    for t in TS:
        sessions[f"slab_T{t}"] = RaggedDecodeSession(
            B, HKV, D, cap, "cuda", dtype, BLOCK)
        pool_tokens = B * (-(-cap // page) * page)
        sessions[f"paged_T{t}"] = PagedDecodeSession(
            B, HKV, D, cap, pool_tokens, page, "cuda", dtype, BLOCK)
    for b in range(B):
        k, v = _randn(HKV, length, D), _randn(HKV, length, D)
        for s in sessions.values():
            s.prefill(b, k, v)
    out = {}
    for name, s in sessions.items():
        t = int(name.rsplit("T", 1)[1])
        q = _randn(B, HQ, t, D)
        k_new, v_new = _randn(B, HKV, t, D), _randn(B, HKV, t, D)
        out[name] = (s.graphed_step(q, k_new, v_new) if t == 1
                     else s.graphed_step_many(q, k_new, v_new))
    return out


def _time(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--length", type=int, default=32768)
    ap.add_argument("--page", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp8"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_verify_step: needs a GPU")
    torch.manual_seed(0)
    rounds = 2
    margin = rounds * (args.steps + args.warmup) * max(TS) + 4 * BLOCK
    variants = _variants(args.length, margin, args.page, args.dtype)
    windows = {v: [] for v in variants}
    for _ in range(rounds):             # every variant, then again
        for v, fn in variants.items():
            windows[v].append(round(_time(fn, args.steps, args.warmup), 4))
    print(json.dumps({
        "bench": "verify_step", "dtype": args.dtype, "B": B, "Hq": HQ,
        "Hkv": HKV, "D": D, "length": args.length, "page": args.page,
        "steps": args.steps, "warmup": args.warmup, "unit": "ms/step",
        "ms": windows,
        "spread_pct": {v: round(abs(w[0] - w[1]) / min(w) * 100, 1)
                       for v, w in windows.items()},
    }))


if __name__ == "__main__":
    main()
