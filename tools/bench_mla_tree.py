#!/usr/bin/env python3
"""PagedMlaSession.attend_tree against attend_many with the same T on the same
session: the tree step against the chain step (profiles/README.md, "MLA tree
drafts").

Per shape one session holds the prefix; every window appends T chain drafts,
times `iters` back-to-back attend_many calls between device events, takes the
drafts back, appends the same rows as a branching tree, times attend_tree the
same way and rejects the tree, so the two alternate. 10 warm-up calls each,
median of 5 windows, spread = (max - min) / median.
"""

import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tree_attention_torch_amd as ta  # noqa: E402

DEV = "cuda"
T = 8
PARENTS = [[-1, 0, 0, 1, 1, 2, 4, 4]]   # two branches, depth 4


def window(fn, iters):
    for _ in range(10):
        fn()
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3   # us


def shape(hq, tkv, dtype, iters, windows=5):
    g = torch.Generator(device=DEV).manual_seed(0)
    new = lambda *s: torch.randn(*s, device=DEV, generator=g).bfloat16()
    sess = ta.PagedMlaSession(1, tkv + 4096, page=128, dtype=dtype)
    sess.prefill(0, new(tkv, 576))
    q, c = new(1, hq, T, 576), new(1, 1, T, 576)
    times = {"chain": [], "tree": []}
    for _ in range(windows):
        sess.append_many(c)
        times["chain"].append(window(lambda: sess.attend_many(q), iters))
        sess.truncate(0, tkv)
        sess.append_tree(c, PARENTS)
        times["tree"].append(window(lambda: sess.attend_tree(q), iters))
        sess.commit([[0]], [0])
    row = {"hq": hq, "tkv": tkv, "T": T, "dtype": dtype}
    for name, t in times.items():
        med = statistics.median(t)
        row[name + "_us"] = round(med, 2)
        row[name + "_spread"] = round((max(t) - min(t)) / med, 3)
    return row


def main():
    for dtype in ("bf16", "fp8_block"):
        for tkv, iters in ((32768, 1000), (131072, 400)):
            for hq in (16, 128):
                print(json.dumps(shape(hq, tkv, dtype, iters)), flush=True)


if __name__ == "__main__":
    main()
