"""Paged against contiguous ragged decode: step latency and reserved bytes.

The shapes and the method of tools/bench_ragged_decode.py: bf16 (or
--dtype fp8), Hkv = 8, G = 4 (Hq = 32), D = 128, B = 8, world size 1, the
"uniform" mix (eight sequences at 32K) and the "skewed" mix (one at 128K,
seven at 4K). One decode step = append one token to every sequence + attend.
Variants:

  ragged        RaggedDecodeSession.graphed_step replay: one (B, Hkv,
                capacity, D) slab, capacity = the longest sequence + margin
  paged<P>      PagedDecodeSession.graphed_step replay at page size P, the
                pool sized for the LIVE tokens + the same margin per row
  ragged_eager  RaggedDecodeSession eager append + attend
  paged_eager   PagedDecodeSession eager append + attend at the first page
                size

Both sessions plan their splits over the same per-row capacity, so the two
graphed variants run the same grid; what differs is the table lookup per
tile and where the pages lie. All variants run in ONE process, alternating,
each twice (the difference between a variant's two windows is the
run-to-run spread); every window is warmed up and timed with a host clock
around work that ends in a device synchronise. ``reserved_bytes`` is K + V
storage (slab, or pool + table). Prints one JSON line; needs a GPU.

Usage: python tools/bench_paged_decode.py [--steps 200] [--warmup 20]
           [--pages 256,128] [--dtype bf16] [--mixes uniform,skewed]
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
MIXES = {
    "uniform": (32768,) * 8,
    "skewed": (131072,) + (4096,) * 7,
}


def _randn(*shape):
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16)


def _bytes(*tensors):
    return sum(t.numel() * t.element_size() for t in tensors)


def _variants(lengths, margin, pages, dtype):
    """name -> (step() closure over a freshly prefilled session, reserved
    bytes)."""
    q = _randn(B, HQ, 1, D)
    k_new, v_new = _randn(B, HKV, 1, D), _randn(B, HKV, 1, D)
    cap = max(lengths) + margin
    ragged = [RaggedDecodeSession(B, HKV, D, cap, "cuda", dtype, BLOCK)
              for _ in range(2)]
    paged = {}
    for i, page in enumerate(pages):
        pool_tokens = sum(-(-(n + margin) // page) * page for n in lengths)
        for name in [f"paged{page}"] + (["paged_eager"] if i == 0 else []):
            paged[name] = PagedDecodeSession(
                B, HKV, D, cap, pool_tokens, page, "cuda", dtype, BLOCK)
    for b, n in enumerate(lengths):
        k, v = _randn(HKV, n, D), _randn(HKV, n, D)
        for s in ragged + list(paged.values()):
            s.prefill(b, k, v)

    def eager(sess):
        def step():
            sess.append(k_new, v_new)
            return sess.attend(q)
        return step

    out = {"ragged": (ragged[0].graphed_step(q, k_new, v_new),
                      _bytes(ragged[0].k, ragged[0].v))}
    for name, s in paged.items():
        nbytes = _bytes(s.k_pool, s.v_pool, s.page_table)
        if name == "paged_eager":
            out["ragged_eager"] = (eager(ragged[1]),
                                   _bytes(ragged[1].k, ragged[1].v))
            out[name] = (eager(s), nbytes)
        else:
            out[name] = (s.graphed_step(q, k_new, v_new), nbytes)
    return out


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
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--mixes", default="uniform,skewed")
    ap.add_argument("--pages", default="256,128")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp8"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_paged_decode: needs a GPU")
    torch.manual_seed(0)
    pages = [int(p) for p in args.pages.split(",")]
    rounds = 2
    margin = rounds * (args.steps + args.warmup) + 4 * BLOCK
    result = {"bench": "paged_decode", "dtype": args.dtype, "B": B, "Hq": HQ,
              "Hkv": HKV, "D": D, "steps": args.steps, "warmup": args.warmup,
              "unit": "us/step", "mixes": {}}
    for name in args.mixes.split(","):
        lengths = MIXES[name]
        variants = _variants(lengths, margin, pages, args.dtype)
        windows = {v: [] for v in variants}
        for _ in range(rounds):             # every variant, then again
            for v, (fn, _) in variants.items():
                windows[v].append(round(_time(fn, args.steps, args.warmup), 2))
        result["mixes"][name] = {
            "lengths": list(lengths),
            "live_tokens": sum(lengths),
            "us": windows,
            "spread_pct": {v: round(abs(w[0] - w[1]) / min(w) * 100, 1)
                           for v, w in windows.items()},
            "reserved_bytes": {v: nb for v, (_, nb) in variants.items()},
        }
        del variants
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
