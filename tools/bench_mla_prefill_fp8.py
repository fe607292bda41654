#!/usr/bin/env python3
"""MLA chunked prefill over the fp8_block pool on e4m3 MFMA operands:
(a) fp8    one mla_prefill_paged(..., compute="fp8") call on the fp8_block pool
(b) loop   what an fp8_block caller had before: the loop of mla_decode_paged
           at Tq = 16 over the same pool, queries and limits
(c) bf16   mla_prefill_paged on a bf16 pool of the same rows

B = 1, page 128; Hq 16 and 128, T 256 and 2048 behind prefixes of 8K and 32K.
Device events around back-to-back calls after warm-up, median of 5 windows,
the three variants alternating, spread = (max - min) / median of the windows.
TF/s = 2 * (576 + 512) * Hq * sum over queries of visible keys / t.
One JSON line per shape.

    python tools/bench_mla_prefill_fp8.py [--quick]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import tree_attention_torch_amd as ta  # noqa: E402
from tree_attention_torch_amd.quant import (dequantize_mla_fp8,  # noqa: E402
                                            quantize_mla_fp8)


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
        rows = torch.randn(n_pages, 1, 128, 576, device=dev).bfloat16()
        pool8 = quantize_mla_fp8(rows)
        pool16 = dequantize_mla_fp8(pool8).bfloat16()
        table = torch.arange(n_pages, dtype=torch.int32, device=dev)[None]
        lens = torch.tensor([n], device=dev)
        q = torch.randn(1, hq, t, 576, device=dev).bfloat16()
        vis = ta.ops.flash.mla_chain_vis(lens, t)
        q16 = [q[:, :, i : i + 16].contiguous() for i in range(0, t, 16)]
        v16 = [vis[:, i : i + 16].contiguous() for i in range(0, t, 16)]

        def fp8():
            return ta.mla_prefill_paged(q, pool8, table, lens, vis,
                                        compute="fp8")

        def loop():
            return [ta.mla_decode_paged(a, pool8, table, lens, b)
                    for a, b in zip(q16, v16)]

        def bf16():
            return ta.mla_prefill_paged(q, pool16, table, lens, vis)

        got = fp8()[0]
        # (b) and (c) see unrounded queries: the distance is the consent's cost
        err_loop = (got - torch.cat([o for o, _ in loop()], dim=2)).abs().max()
        err_bf16 = (got - bf16()[0]).abs().max()
        calls = 3 if t >= 2048 else 10
        variants = (("fp8", fp8), ("loop", loop), ("bf16", bf16))
        times = {name: [] for name, _ in variants}
        for _ in range(5):
            for name, fn in variants:
                times[name].append(window(fn, calls))
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
        flop = 2 * (576 + 512) * hq * float(vis.sum())
        print(json.dumps({
            "hq": hq, "t": t, "prefix": pre,
            "fp8_ms": round(med["fp8"], 4),
            "loop_ms": round(med["loop"], 4),
            "bf16_ms": round(med["bf16"], 4),
            "loop_over_fp8": round(med["loop"] / med["fp8"], 3),
            "fp8_over_bf16": round(med["fp8"] / med["bf16"], 3),
            "spread": {k: round(v, 4) for k, v in spread.items()},
            "fp8_tflops": round(flop / med["fp8"] / 1e9, 1),
            "bf16_tflops": round(flop / med["bf16"] / 1e9, 1),
            "max_abs_diff_vs_loop": err_loop.item(),
            "max_abs_diff_vs_bf16": err_bf16.item()}), flush=True)


if __name__ == "__main__":
    main()
