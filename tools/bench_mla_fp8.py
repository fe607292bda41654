#!/usr/bin/env python3
"""The PagedMlaSession verify step over the fp8_block latent pool against the
same step over the bf16 pool (profiles/README.md, "MLA fp8 latent").

A step is append_many of Tq rows, attend_many (Tq = 1: append, attend) and a
truncate back to the starting length, so every step sees the same keys. Times
as tools/bench_mla_paged.py takes them, the two stores alternating.
"""

import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mla_paged import DEV, timed  # noqa: E402

import tree_attention_torch_amd as ta  # noqa: E402


def step_fn(dtype, hq, tkv, tq):
    g = torch.Generator(device=DEV).manual_seed(0)
    sess = ta.PagedMlaSession(1, tkv + 256, page=128, dtype=dtype)
    sess.prefill(0, torch.randn(tkv, 576, device=DEV, generator=g).bfloat16())
    q = torch.randn(1, hq, tq, 576, device=DEV, generator=g).bfloat16()
    c = torch.randn(1, 1, tq, 576, device=DEV, generator=g).bfloat16()

    def step():
        if tq == 1:
            sess.append(c)
            out = sess.attend(q)
        else:
            sess.append_many(c)
            out = sess.attend_many(q)
        sess.truncate(0, tkv)
        return out
    return step


def main():
    for tkv, iters in ((8192, 200), (131072, 60)):
        for hq in (16, 128):
            for tq in (1, 4):
                fns = {d: step_fn(d, hq, tkv, tq) for d in ("bf16", "fp8_block")}
                row = {"hq": hq, "tkv": tkv, "tq": tq, **timed(fns, iters)}
                row["fp8_over_bf16"] = round(
                    row["fp8_block_us"] / row["bf16_us"], 3)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
