#!/usr/bin/env python3
"""MLA decode over the paged latent pool against the slab entry, multi-token
verify queries against a loop of single-query calls, and the PagedMlaSession
step eager against graphed (profiles/README.md, "MLA paged decode").

Step times: device events around `iters` back-to-back calls after 10 warm-up
calls, median of 5 windows, the variants of a shape alternating. With
--only HQ,TKV,TQ the script runs that one shape a few times and prints
nothing: the form a `rocprofv3 --kernel-trace --stats` run of its own takes.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import tree_attention_torch_amd as ta  # noqa: E402
from tree_attention_torch_amd.ops.flash import mla_chain_vis  # noqa: E402

DEV = "cuda"


def timed(fns, iters, windows=5):
    """{name}_us: median over the windows; {name}_spread: (max - min) / it."""
    for fn in fns.values():
        for _ in range(10):
            fn()
    out = {name: [] for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) / iters * 1e3)   # us
    row = {}
    for name, t in out.items():
        med = statistics.median(t)
        row[name + "_us"] = round(med, 2)
        row[name + "_spread"] = round((max(t) - min(t)) / med, 3)
    return row


def shape(hq, tkv, tq, page):
    """q, the slab, and the same rows in a pool behind a permuted table."""
    g = torch.Generator(device=DEV).manual_seed(0)
    q = torch.randn(1, hq, tq, 576, device=DEV, generator=g).bfloat16()
    ckv = torch.randn(1, 1, tkv, 576, device=DEV, generator=g).bfloat16()
    n = tkv // page
    perm = torch.randperm(n, device=DEV, generator=g)
    pool = torch.empty(n, 1, page, 576, device=DEV, dtype=torch.bfloat16)
    pool[perm] = ckv.view(n, 1, page, 576)
    lens = torch.tensor([tkv], device=DEV)
    return q, ckv, pool, perm.int().view(1, n), lens


def variants(hq, tkv, tq, pages):
    fns = {}
    for page in pages:
        q, ckv, pool, table, lens = shape(hq, tkv, tq, page)
        # the visible lengths a session's append kernel leaves on the device
        vis = mla_chain_vis(lens, tq) if tq > 1 else None
        fns[f"paged{page}"] = (
            lambda q=q, pool=pool, table=table, lens=lens, vis=vis:
            ta.mla_decode_paged(q, pool, table, lens, vis))
    qs = [q[:, :, i : i + 1].contiguous() for i in range(tq)]
    fns["slab" if tq == 1 else "slab_loop"] = (
        lambda: [ta.mla_decode(qi, ckv) for qi in qs])
    return fns


def session_step(b=8, hq=16, length=8192):
    def make():
        s = ta.PagedMlaSession(b, length + 4096, page=128)
        for i in range(b):
            s.prefill(i, torch.randn(length - 64 * i, 576, device=DEV).bfloat16())
        return s
    q = torch.randn(b, hq, 1, 576, device=DEV).bfloat16()
    c = torch.randn(b, 1, 1, 576, device=DEV).bfloat16()
    eager, graphed = make(), make()
    replay = graphed.graphed_step(q, c)

    def eager_step():
        eager.append(c)
        return eager.attend(q)
    return {"eager": eager_step, "graphed": replay}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="HQ,TKV,TQ: profile form")
    args = ap.parse_args()
    if args.only:
        hq, tkv, tq = map(int, args.only.split(","))
        for fn in variants(hq, tkv, tq, (128,)).values():
            for _ in range(30):
                fn()
        torch.cuda.synchronize()
        return
    for tkv, iters in ((32768, 200), (131072, 60)):
        for hq in (16, 128):
            for tq in (1, 2, 4):
                fns = variants(hq, tkv, tq, (128, 1024) if tq == 1 else (128,))
                row = {"hq": hq, "tkv": tkv, "tq": tq, **timed(fns, iters)}
                print(json.dumps(row), flush=True)
    row = {"session": "B=8 Hq=16 len~8K page 128",
           **timed(session_step(), 200)}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
