"""Ragged batched decode step latency: RaggedDecodeSession (graphed and
eager) against what the package offered before it for the same batch.

bf16, Hkv = 8, G = 4 (Hq = 32), D = 128, B = 8, world size 1, two length
mixes: "uniform" (eight sequences at 32K) and "skewed" (one at 128K, seven at
4K). One decode step = append one token to every sequence + attend. Variants:

  a  RaggedDecodeSession.graphed_step replay
  b  RaggedDecodeSession eager append + attend
  c  eight B = 1 DecodeSessions, each append + sync_len + graphed_attend
     replay, in turn
  d  (uniform only) one B = 8 DecodeSession, eager append + attend

All variants run in ONE process, alternating, each twice (the difference
between a variant's two windows is the run-to-run spread); every window is
warmed up and timed with a host clock around work that ends in a device
synchronise. Prints one JSON line; needs a GPU.

Usage: python tools/bench_ragged_decode.py [--steps 200] [--warmup 20]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tree_attention_torch_amd.session import (DecodeSession,  # noqa: E402
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


def _variants(lengths, margin):
    """name -> step() closures over freshly prefilled sessions."""
    q = _randn(B, HQ, 1, D)
    k_new, v_new = _randn(B, HKV, 1, D), _randn(B, HKV, 1, D)
    cap = max(lengths) + margin
    ragged = [RaggedDecodeSession(B, HKV, D, cap, "cuda", "bf16", BLOCK)
              for _ in range(2)]
    singles = [DecodeSession(1, HKV, D, n + margin, "cuda", "bf16", BLOCK)
               for n in lengths]
    uniform = len(set(lengths)) == 1
    batched = DecodeSession(B, HKV, D, cap, "cuda", "bf16", BLOCK) \
        if uniform else None
    for b, n in enumerate(lengths):
        k, v = _randn(HKV, n, D), _randn(HKV, n, D)
        for s in ragged:
            s.prefill(b, k, v)
        singles[b].prefill(k[None], v[None])
        if batched is not None:     # DecodeSession prefills whole batches
            batched.k[b, :, :n] = k
            batched.v[b, :, :n] = v
    if batched is not None:
        batched.total = batched.local_len = lengths[0]

    replay_a = ragged[0].graphed_step(q, k_new, v_new)

    def step_b():
        ragged[1].append(k_new, v_new)
        return ragged[1].attend(q)

    replays_c = []
    for b, s in enumerate(singles):
        s.sync_len()
        replays_c.append(s.graphed_attend(q[b:b + 1].contiguous())[0])

    def step_c():
        for b, s in enumerate(singles):
            s.append(k_new[b:b + 1], v_new[b:b + 1])
            s.sync_len()
            out = replays_c[b]()
        return out

    out = {"a": replay_a, "b": step_b, "c": step_c}
    if batched is not None:
        def step_d():
            batched.append(k_new, v_new)
            return batched.attend(q)

        out["d"] = step_d
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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ragged_decode: needs a GPU")
    torch.manual_seed(0)
    rounds = 2
    margin = rounds * (args.steps + args.warmup) + 4 * BLOCK
    result = {"bench": "ragged_decode", "dtype": "bf16", "B": B, "Hq": HQ,
              "Hkv": HKV, "D": D, "steps": args.steps, "warmup": args.warmup,
              "unit": "us/step", "mixes": {}}
    for name in args.mixes.split(","):
        lengths = MIXES[name]
        variants = _variants(lengths, margin)
        windows = {v: [] for v in variants}
        for _ in range(rounds):             # a b c d a b c d
            for v, fn in variants.items():
                windows[v].append(round(_time(fn, args.steps, args.warmup), 2))
        result["mixes"][name] = {
            "lengths": list(lengths),
            "us": windows,
            "spread_pct": {v: round(abs(w[0] - w[1]) / min(w) * 100, 1)
                           for v, w in windows.items()},
        }
        del variants
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
