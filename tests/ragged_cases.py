"""Ragged-batch needle inputs: one KV length per batch row.

The construction of tests/needle_cases.py (docs/NEEDLE_TESTS.md) on a batch
whose rows have their own lengths. B = 4, Hq = 8, Hkv = 2, D = 128 over a
cache of capacity 1024 (two 512-key splits, 64- and 128-key tiles). Every
query row is ``2 * K[b, h // 4, target(b, h)]``; head 0 of every batch row
targets that row's LAST key, so a length one short loses it, and every cache
row at or past a row's length holds a decoy K and a NaN V, so a length one
long (or another row's longer length) poisons the output. A row of length 0
must come back as out = 0, lse = -inf.

One more length set, (4097, 0, 513, 2560), runs at a capacity of 4608 (nine
512-key splits): its rows leave none, all, seven and four trailing splits
empty, and their heads target the first key of every live split they reach.

This module is a plain helper (not a conftest). K/V are drawn once per dtype
and capacity and shared, unchanged, by every length set and test.
"""

from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import torch

import needle_cases as nc

SEED = 20261021
B, HQ, HKV, D, CAP = 4, 8, 2, 128, 1024
G = HQ // HKV
LENGTH_SETS = (
    (513, 0, 64, 1023),
    (1, 65, 512, 1024),
    (511, 129, 127, 1000),
)
# a second capacity, 4608 = nine 512-key splits: row 0 fills all nine (the
# last with one key), row 1 is empty, row 2 leaves splits 2..8 empty and row
# 3 splits 5..8 (empty trailing splits below and at or above the combine
# kernel's group count of 4)
CAP_BIG = 4608
LENGTH_SETS_BIG = ((4097, 0, 513, 2560),)
CHUNK = 512    # needle_cases.split_plan(4, 2, cap)[1] for both capacities
DTYPES = ("bf16", "fp8")
KIND = {"bf16": "half", "fp8": "fp8"}
SEAMS = (0, 63, 64, 127, 128, 511, 512)
# the graphed-step test: row 0 crosses the split seam (511 -> 512 -> 513),
# row 1 sits inactive, row 2 is empty, row 3 grows alongside
GRAPH_START = (510, 65, 0, 999)
GRAPH_MASK = (True, False, False, True)
GRAPH_STEPS = tuple(
    tuple(n + (i + 1) * m for n, m in zip(GRAPH_START, GRAPH_MASK))
    for i in range(3))

_TD = {"bf16": torch.bfloat16, "fp8": torch.float8_e4m3fn}


def cap_of(lengths) -> int:
    """The cache capacity a length set runs at."""
    return CAP_BIG if tuple(lengths) in LENGTH_SETS_BIG else CAP


@dataclass
class Ragged:
    lengths: tuple
    dtype: str
    kind: str
    cap: int
    k: torch.Tensor         # (B, Hkv, cap, D) storage dtype; row b's live
    v: torch.Tensor         # keys are [:lengths[b]]
    q: torch.Tensor         # (B, Hq, 1, D) bf16
    targets: torch.Tensor   # (B, Hq) key each head attends; -1: empty row
    k_cache: torch.Tensor   # k / v with the guard pattern at and past each
    v_cache: torch.Tensor   # row's length
    ref_out: torch.Tensor   # fp32 oracle (B, Hq, 1, D)
    ref_lse: torch.Tensor   # (B, Hq, 1); -inf for an empty row
    targets2: torch.Tensor | None = None   # family "pair": the second target


@lru_cache(maxsize=None)
def kv(dtype: str, cap: int = CAP):
    """randn rounded to the cache dtype, every batch row different; one
    draw per capacity."""
    g = torch.Generator().manual_seed(SEED + (cap if cap != CAP else 0))
    k = torch.randn(B, HKV, cap, D, generator=g).to(_TD[dtype])
    v = torch.randn(B, HKV, cap, D, generator=g).to(_TD[dtype])
    return k, v


def targets(lengths) -> torch.Tensor:
    """Head 0 of every row targets L_b - 1; the other heads rotate, offset
    by b, over L_b - 1 and the seams below L_b. At the capacity of nine
    splits the seams are the first keys of the row's live splits, last split
    first (eight heads: row 0 reaches splits 8..1, rows 2 and 3 every live
    split)."""
    tg = torch.full((B, HQ), -1, dtype=torch.long)
    big = cap_of(lengths) == CAP_BIG
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        seams = reversed(range(0, n, CHUNK)) if big else SEAMS
        cand = [n - 1] + [s for s in seams if s < n and s != n - 1]
        tg[b, 0] = n - 1
        for h in range(1, HQ):
            tg[b, h] = cand[(h + b) % len(cand)]
    return tg


def guard_fill(q: torch.Tensor, cap: int = CAP):
    """(B, Hkv, cap, D) fp32 guard rows: decoy K = twice a query of that KV
    head's group (rotating), V = NaN."""
    j = torch.arange(cap)
    heads = torch.arange(HKV)[:, None] * G + (j % G)[None, :]    # (Hkv, CAP)
    gk = 2.0 * q.float()[:, heads, 0]                     # (B, Hkv, CAP, D)
    return gk, torch.full_like(gk, float("nan"))


def write_guards(k, v, q, lengths) -> None:
    """Overwrite, IN PLACE, every row of k / v (B, Hkv, cap, D) at or past
    lengths[b] with the guard pattern (any device, the tensors' dtype)."""
    cap = k.shape[2]
    gk, gv = guard_fill(q.cpu(), cap)
    for b, n in enumerate(lengths):
        k[b, :, n:] = gk[b, :, n:cap].to(device=k.device, dtype=k.dtype)
        v[b, :, n:] = gv[b, :, n:cap].to(device=v.device, dtype=v.dtype)


def with_guards(k, v, q, lengths):
    """Copies of k / v with the guard pattern at and past each length."""
    kc, vc = k.clone(), v.clone()
    write_guards(kc, vc, q, lengths)
    return kc, vc


def attend_lengths(rg: "Ragged", lengths, fn):
    """Row-by-row attention over the GUARDED cache with row b cut at
    lengths[b] (clipped to [0, capacity]): the true lengths give the oracle,
    any other lengths a mutant. fn(q, k, v) -> (out, lse)."""
    outs, lses = [], []
    for b, n in enumerate(lengths):
        n = max(0, min(int(n), rg.cap))
        qb = rg.q[b:b + 1].float()
        if n == 0:
            outs.append(torch.zeros(1, HQ, 1, D))
            lses.append(torch.full((1, HQ, 1), float("-inf")))
            continue
        o, l = fn(qb, rg.k_cache[b:b + 1, :, :n].float(),
                  rg.v_cache[b:b + 1, :, :n].float())
        outs.append(o.float())
        lses.append(l.float())
    return torch.cat(outs), torch.cat(lses)


@lru_cache(maxsize=None)
def build(lengths: tuple, dtype: str, family: str = "seam") -> Ragged:
    """family "pair" (the nine-split capacity): every head of a row with at
    least three live splits reads 2 * (K[t1] + K[t2]), t1 its seam target
    and t2 a key of the partner split chosen by needle_cases.pair_key, so
    the combine weighs two live splits at 0.67..0.82 / 0.18..0.33; the other
    rows keep their one-hot query. rg.targets2 holds t2 (-1: none)."""
    from tree_attention_torch_amd.ops.reference import flash_res_lse

    cap = cap_of(lengths)
    k, v = kv(dtype, cap)
    tg = targets(lengths)
    kvh = torch.arange(HQ) // G
    bi = torch.arange(B)[:, None]
    # an empty row has no target: its query still points at stored data
    # (key h of the dead buffer), so a kernel that reads it answers O(1)
    idx = torch.where(tg >= 0, tg, torch.arange(HQ)[None, :].expand(B, HQ))
    qf = nc.needle_gain(D) * k.float()[bi, kvh[None, :], idx]    # (B, Hq, D)
    q = qf.to(torch.bfloat16)[:, :, None, :].contiguous()
    assert torch.equal(q.float()[:, :, 0], qf), "gain*K must be exact in bf16"
    tg2 = torch.full_like(tg, -1)
    if family == "pair":
        assert cap == CAP_BIG
        for b, n in enumerate(lengths):
            live = -(-n // CHUNK)
            for h in range(HQ if live >= 3 else 0):
                tg2[b, h], q[b, h, 0] = nc.pair_key(
                    k[b, h // G, :n].float(), int(tg[b, h]), live, CHUNK,
                    nc.needle_gain(D), 1.0 / D ** 0.5, dtype == "fp8",
                    torch.bfloat16, what=(lengths, dtype, b, h))
    else:
        assert family == "seam", family
    k_cache, v_cache = with_guards(k, v, q, lengths)
    rg = Ragged(tuple(lengths), dtype, KIND[dtype], cap, k, v, q, tg, k_cache,
                v_cache, None, None, tg2)
    rg.ref_out, rg.ref_lse = attend_lengths(rg, lengths, flash_res_lse)
    return rg


def mutant_lengths(lengths) -> dict:
    """The length errors the inputs must expose."""
    n = list(lengths)
    return {
        "L+1": [x + 1 for x in n],
        "L-1": [x - 1 for x in n],
        "row0_for_all": [n[0]] * B,
        "max_for_all": [max(n)] * B,
        "capacity_for_all": [cap_of(lengths)] * B,
        "row_b^1": [n[b ^ 1] for b in range(B)],
    }


def chunk_mutant_lengths(lengths) -> dict:
    """The live length rounded to a boundary of the 512-key split chunk."""
    return {
        "chunk_down": [x // CHUNK * CHUNK for x in lengths],
        "chunk_up": [-(-x // CHUNK) * CHUNK for x in lengths],
    }


def compare(rg: Ragged, out, lse, what: str = "") -> None:
    """Finite rows at the kind's bars (nc.compare); an empty row by
    equality: out = 0 and lse = -inf exactly."""
    out = out.detach().float().cpu()
    lse = None if lse is None else lse.detach().float().cpu()
    live = torch.tensor([n > 0 for n in rg.lengths])
    try:
        nc.compare(out[live], None if lse is None else lse[live],
                   rg.ref_out[live], rg.ref_lse[live], rg.kind)
        assert torch.equal(out[~live], torch.zeros_like(out[~live])), \
            "an empty row must be all zeros"
        if lse is not None:
            assert bool((lse[~live] == float("-inf")).all()), \
                "an empty row's lse must be -inf"
    except AssertionError as e:
        raise AssertionError(
            f"ragged {rg.dtype} lengths {rg.lengths} {what}\n{e}") from None


def rejected(rg: Ragged, out, lse) -> bool:
    try:
        compare(rg, out, lse)
    except AssertionError:
        return True
    return False


def stream(rg: Ragged):
    """The K/V a session is fed: bf16 tensors whose cast to the cache dtype
    gives back rg.k / rg.v bit for bit (e4m3 values are exact in bf16)."""
    return rg.k.float().bfloat16(), rg.v.float().bfloat16()
