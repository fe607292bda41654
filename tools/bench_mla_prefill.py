#!/usr/bin/env python3
"""MLA chunked prefill: one mla_prefill_paged call against the loop of
mla_decode_paged at Tq = 16 over the same queries and limits.

B = 1, bf16, page 128; Hq 16 and 128, T 256 and 2048 behind prefixes of 8K and
32K. Device events around back-to-back calls after warm-up, median of 5
windows, the two variants alternating, spread = (max - min) / median of the
windows. TF/s = 2 * (576 + 512) * Hq * sum over queries of visible keys / t.
One JSON line per shape.

    python tools/bench_mla_prefill.py [--quick]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import tree_attention_torch_amd as ta  # noqa: E402


def window(fn, calls):
    start, end = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true",
                    help="only T = 2048 behind 32K")
    args = ap.parse_args()
    shapes = [(hq, t, pre) for hq in (16, 128) for t in (256, 2048)
              for pre in (8192, 32768)]
    if args.quick:
        shapes = [s for s in shapes if s[1:] == (2048, 32768)]
    dev = torch.device("cuda:0")
    for hq, t, pre in shapes:
        n = pre + t
        n_pages = -(-n // 128)
        pool = torch.randn(n_pages, 1, 128, 576, device=dev).bfloat16()
        table = torch.arange(n_pages, dtype=torch.int32, device=dev)[None]
        lens = torch.tensor([n], device=dev)
        q = torch.randn(1, hq, t, 576, device=dev).bfloat16()
        vis = ta.ops.flash.mla_chain_vis(lens, t)
        q16 = [q[:, :, i : i + 16].contiguous() for i in range(0, t, 16)]
        v16 = [vis[:, i : i + 16].contiguous() for i in range(0, t, 16)]

        def one():
            return ta.mla_prefill_paged(q, pool, table, lens, vis)

        def loop():
            return [ta.mla_decode_paged(a, pool, table, lens, b)
                    for a, b in zip(q16, v16)]

        got = one()[0]
        want = torch.cat([o for o, _ in loop()], dim=2)
        err = (got - want).abs().max().item()
        calls = 3 if t >= 2048 else 10
        times = {"prefill": [], "loop": []}
        for _ in range(5):
            for name, fn in (("prefill", one), ("loop", loop)):
                times[name].append(window(fn, calls))
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
        flop = 2 * (576 + 512) * hq * float(vis.sum())
        print(json.dumps({
            "hq": hq, "t": t, "prefix": pre,
            "prefill_ms": round(med["prefill"], 4),
            "loop_ms": round(med["loop"], 4),
            "speedup": round(med["loop"] / med["prefill"], 3),
            "spread": {k: round(v, 4) for k, v in spread.items()},
            "prefill_tflops": round(flop / med["prefill"] / 1e9, 1),
            "max_abs_diff_vs_loop": err}), flush=True)


if __name__ == "__main__":
    main()
