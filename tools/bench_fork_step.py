"""Cost of the copy-on-write step after an n-way fork.

bf16, Hkv = 8, G = 4 (Hq = 32), D = 128, page 256 (--page), world size 1.
Row 0 holds a prompt of --length tokens whose tail page is partly full
(--tail rows) and sits idle, as a prompt kept for later forks does; rows
1..16 are forked from it, so the tail page has 17 holders and the first step
of the 16 active rows carries 16 tail-page copies. Variants, each a
graphed_step replay under the same active mask on a session of its own:

  steady      the rows have their own tail pages: no copy
  cow_kernel  re-forked before every step: 16 copies, one kv_pool_copy_rows
              launch ahead of the replay
  cow_slices  the same with the copies done as 2 x 16 torch slice
              assignments (the session's path where the kernel does not
              apply)

Every step is timed on its own, with a host clock from a device synchronise
to the synchronise after the replay, so the host's page bookkeeping is part
of the figure in every variant; the re-fork between the steps is not. All
variants run in ONE process, alternating, each twice (the difference between
a variant's two windows is the run-to-run spread); every window is warmed
up. Measures and asserts nothing. Prints one JSON line; needs a GPU.

Usage: python tools/bench_fork_step.py [--steps 200] [--warmup 20]
           [--length 8192] [--tail 200] [--page 256]
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

ROWS, HKV, G, D = 16, 8, 4, 128
B = ROWS + 1       # row 0: the idle holder of the prompt
HQ = HKV * G
BLOCK = 256


class SliceCopySession(PagedDecodeSession):
    """The copies as torch slice assignments, whatever the device."""

    def _copy_pages(self, copies) -> None:
        for src, dst, rows in copies:
            self.k_pool[dst, :, :rows] = self.k_pool[src, :, :rows]
            self.v_pool[dst, :, :rows] = self.v_pool[src, :, :rows]


def _randn(*shape):
    return torch.randn(*shape, device="cuda", dtype=torch.bfloat16)


def _variant(cls, length, page, margin, refork):
    """-> step(): (re-fork, untimed) then one timed replay, in ms."""
    cap = length + margin
    pages = -(-length // page) + ROWS * (-(-margin // page) + 2)
    sess = cls(B, HKV, D, cap, pages * page, page, "cuda", "bf16", BLOCK)
    sess.prefill(0, _randn(HKV, length, D), _randn(HKV, length, D))
    mask = [False] + [True] * ROWS

    def fork_all():
        for b in range(1, B):
            sess.fork(0, b, length)

    fork_all()
    replay = sess.graphed_step(_randn(B, HQ, 1, D), _randn(B, HKV, 1, D),
                               _randn(B, HKV, 1, D))
    copies = []

    def step():
        if refork:
            fork_all()
        free = sess.free_pages
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        replay(mask)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        copies.append(free - sess.free_pages)
        return dt * 1e3

    return step, copies


def _window(step, copies, steps, warmup):
    for _ in range(warmup):
        step()
    copies.clear()
    return sum(step() for _ in range(steps)) / steps


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--length", type=int, default=8192)
    ap.add_argument("--tail", type=int, default=200)
    ap.add_argument("--page", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fork_step: needs a GPU")
    if not 0 < args.tail < args.page:
        sys.exit("bench_fork_step: need 0 < tail < page")
    torch.manual_seed(0)
    length = args.length // args.page * args.page + args.tail
    rounds = 2
    # a re-forked row never grows past length + 1; the steady rows do
    margin = rounds * (args.steps + args.warmup) + 2 * BLOCK
    variants = {
        "steady": _variant(PagedDecodeSession, length, args.page, margin,
                           False),
        "cow_kernel": _variant(PagedDecodeSession, length, args.page, margin,
                               True),
        "cow_slices": _variant(SliceCopySession, length, args.page, margin,
                               True),
    }
    windows = {v: [] for v in variants}
    for _ in range(rounds):             # every variant, then again
        for v, (step, copies) in variants.items():
            windows[v].append(round(
                _window(step, copies, args.steps, args.warmup), 4))
    print(json.dumps({
        "bench": "fork_step", "dtype": "bf16", "rows": ROWS, "B": B,
        "Hq": HQ, "Hkv": HKV, "D": D, "length": length, "tail": args.tail,
        "page": args.page, "steps": args.steps, "warmup": args.warmup,
        "unit": "ms/step", "ms": windows,
        # pages taken per timed step of the last window: the copies
        # (steady: the pages the growing rows open)
        "pages_per_step": {v: [min(c), max(c)]
                           for v, (_, c) in variants.items()},
        "spread_pct": {v: round(abs(w[0] - w[1]) / min(w) * 100, 1)
                       for v, w in windows.items()},
    }))


if __name__ == "__main__":
    main()
