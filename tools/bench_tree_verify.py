"""Cost of a tree-shaped verify step against the chain verify step of the
same T.

The shapes and the method of tools/bench_verify_step.py: bf16 (or --dtype
fp8), Hkv = 8, G = 4 (Hq = 32), D = 128, B = 8 sequences at 32K tokens each
(--length), world size 1. Variants, over a slab (RaggedDecodeSession) and a
paged (PagedDecodeSession, --page) session each:

  chain_T4   graphed_step_many replay at T = 4 (one attention launch)
  tree_T4    graphed_step_tree replay at T = 4, a 2-branch tree
             (parents -1, 0, 0, 1)
  chain_T16  graphed_step_many replay at T = 16 (four attention launches)
  tree_T16   graphed_step_tree replay at T = 16: two branches of 7 and 8
             nodes under one root (parents -1, 0, 0, 1, 2, ..., 13)

The step streams the whole KV once whatever the mask is, so a tree step is
expected to cost what the chain step of the same T costs; this tool measures
it and asserts nothing. Every sequence grows by T tokens per step in both
(no truncate, no commit: the same KV length in every window of a pair). All
variants run in ONE process, alternating, each twice (the difference between
a variant's two windows is the run-to-run spread); every window is warmed
up, which also ramps the clocks, and timed with a host clock around work
that ends in a device synchronise. Prints one JSON line; needs a GPU.

Usage: python tools/bench_tree_verify.py [--steps 200] [--warmup 20]
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
TS = (4, 16)
PARENTS = {4: [-1, 0, 0, 1], 16: [-1, 0, 0] + list(range(1, 14))}


def _randn(*shape):
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16)


def _variants(length, margin, page, dtype):
    """name -> replay() of a captured step over a freshly prefilled
    session of its own."""
    cap = length + margin
    sessions = {}
    for t in TS:
        for shape in ("chain", "tree"):
            sessions[f"slab_{shape}_T{t}"] = RaggedDecodeSession(
                B, HKV, D, cap, "cuda", dtype, BLOCK)
            pool_tokens = B * (-(-cap // page) * page)
            sessions[f"paged_{shape}_T{t}"] = PagedDecodeSession(
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
        if "chain" in name:
            out[name] = s.graphed_step_many(q, k_new, v_new)
        else:
            parents = torch.tensor([PARENTS[t]] * B, dtype=torch.int32,
                                   device="cuda")
            out[name] = s.graphed_step_tree(q, k_new, v_new, parents)
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
        sys.exit("bench_tree_verify: needs a GPU")
    torch.manual_seed(0)
    rounds = 2
    margin = rounds * (args.steps + args.warmup) * max(TS) + 4 * BLOCK
    variants = _variants(args.length, margin, args.page, args.dtype)
    windows = {v: [] for v in variants}
    for _ in range(rounds):             # every variant, then again
        for v, fn in variants.items():
            windows[v].append(round(_time(fn, args.steps, args.warmup), 4))
    print(json.dumps({
        "bench": "tree_verify", "dtype": args.dtype, "B": B, "Hq": HQ,
        "Hkv": HKV, "D": D, "length": args.length, "page": args.page,
        "steps": args.steps, "warmup": args.warmup, "unit": "ms/step",
        "ms": windows,
        "spread_pct": {v: round(abs(w[0] - w[1]) / min(w) * 100, 1)
                       for v, w in windows.items()},
    }))


if __name__ == "__main__":
    main()
