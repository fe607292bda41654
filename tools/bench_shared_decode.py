"""Decode step over a forked prompt: graphed_step(shared=False) against
graphed_step(shared=True).

Hkv = 8, D = 128, page 256 (--page), world size 1, PagedDecodeSession. 16
rows share one prompt of --lengths tokens (whole pages: row 0 is prefilled,
rows 1..15 are forked from it) and each holds --own tokens of its own behind
it; all 16 are active. Per dtype (bf16, fp8), G = Hq / Hkv (4: four rows per
KV stream, 1: sixteen) and prompt length, two variants on sessions of their
own:

  plain   graphed_step(): every row streams the prompt's pages itself
  shared  graphed_step(shared=True): one stream per group of 16 / G rows over
          the prompt, one per row over its own tokens, one combine

By bytes the shared step reads the prompt ceil(16 / (16 / G)) times instead
of 16. Every step is timed on its own, with a host clock from a device
synchronise to the synchronise after the replay, so the host's bookkeeping
(the plan's staleness check included) is part of the figure. All variants run
in ONE process, alternating, each twice (the difference between a variant's
two windows is the run-to-run spread); every window is warmed up. A replay
that takes longer than --step-limit seconds ends the run: nothing more is
started on the device. Measures and asserts nothing else. Prints one JSON
line; needs a GPU.

Usage: python tools/bench_shared_decode.py [--steps 200] [--warmup 20]
           [--lengths 8192,32768] [--own 256] [--page 256] [--dtypes bf16,fp8]
           [--groups 4,1] [--step-limit 10]
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

ROWS, HKV, D = 16, 8, 128
BLOCK = 256


def _randn(*shape):
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16)


def _variant(dtype, g, length, own, page, margin, shared, limit):
    """-> step(): one timed replay, in ms."""
    cap = length + own + margin
    pages = length // page + ROWS * (-(-(own + margin) // page) + 1)
    sess = PagedDecodeSession(ROWS, HKV, D, cap, pages * page, page, "cuda",
                              dtype, BLOCK)
    sess.prefill(0, _randn(HKV, length, D), _randn(HKV, length, D))
    for b in range(1, ROWS):
        sess.fork(0, b, length)
    for b in range(ROWS):
        sess.prefill(b, _randn(HKV, own, D), _randn(HKV, own, D))
    replay = sess.graphed_step(_randn(ROWS, HKV * g, 1, D),
                               _randn(ROWS, HKV, 1, D),
                               _randn(ROWS, HKV, 1, D), shared=shared)

    def step():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        replay()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt > limit:
            sys.exit(f"bench_shared_decode: a replay took {dt:.1f} s, over "
                     f"the limit of {limit} s")
        return dt * 1e3

    return step, sess


def _window(step, steps, warmup):
    for _ in range(warmup):
        step()
    return sum(step() for _ in range(steps)) / steps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--lengths", default="8192,32768")
    ap.add_argument("--own", type=int, default=256)
    ap.add_argument("--page", type=int, default=256)
    ap.add_argument("--dtypes", default="bf16,fp8")
    ap.add_argument("--groups", default="4,1")
    ap.add_argument("--step-limit", type=float, default=10.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_shared_decode: needs a GPU")
    lengths = [int(x) for x in args.lengths.split(",")]
    if any(n % args.page for n in lengths):
        sys.exit("bench_shared_decode: prompts are whole pages")
    torch.manual_seed(0)
    rounds = 2
    margin = rounds * (args.steps + args.warmup) + BLOCK
    variants, uploads = {}, {}
    for dtype in args.dtypes.split(","):
        for g in (int(x) for x in args.groups.split(",")):
            for n in lengths:
                for shared in (False, True):
                    name = (f"{dtype}_G{g}_{n // 1024}K_"
                            f"{'shared' if shared else 'plain'}")
                    variants[name] = _variant(dtype, g, n, args.own,
                                              args.page, margin, shared,
                                              args.step_limit)
    windows = {v: [] for v in variants}
    for _ in range(rounds):             # every variant, then again
        for v, (step, sess) in variants.items():
            before = sess.shared_plan_uploads
            windows[v].append(round(_window(step, args.steps, args.warmup),
                                    4))
            uploads[v] = sess.shared_plan_uploads - before
    ratio = {}
    for v, w in windows.items():
        if v.endswith("_shared"):
            p = windows[v[:-len("shared")] + "plain"]
            ratio[v[:-len("_shared")]] = [round(a / b, 3)
                                          for a, b in zip(w, p)]
    print(json.dumps({
        "bench": "shared_decode", "rows": ROWS, "Hkv": HKV, "D": D,
        "own": args.own, "page": args.page, "steps": args.steps,
        "warmup": args.warmup, "unit": "ms/step", "ms": windows,
        # shared / plain, window by window
        "shared_over_plain": ratio,
        # plan uploads during the last window (a steady step uploads nothing)
        "uploads_last_window": {v: n for v, n in uploads.items()
                                if v.endswith("_shared")},
        "spread_pct": {v: round(abs(w[0] - w[1]) / min(w) * 100, 1)
                       for v, w in windows.items()},
    }))


if __name__ == "__main__":
    main()
