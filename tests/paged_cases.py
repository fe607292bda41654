"""Paged needle inputs: the ragged construction of tests/ragged_cases.py
scattered into a page pool (n_pages, Hkv, page, D) behind a (B, max_pages)
page table, for both cache dtypes and page sizes 128 and 256, at the two
capacities of ragged_cases (1024: two 512-key splits; 4608: nine).

What paging adds to the targets. A page id that is one tile stale, or the
chunk's first id kept for the whole chunk, reads the wrong page only on keys
behind a page boundary that is NOT a split-chunk start (a chunk start loads
its id fresh). ragged_cases' seams (0, 63, 64, 127, 128, 511, 512) hold no
key of [256, 384), so at page 256 nothing would see it. Every row long
enough therefore also targets the first key of each page that starts no
split chunk: 128 at page 128, 256 and 768 at page 256, and at the nine-split
capacity ``s * 512 + page`` for live splits s.

The pool. Page ids come from a seeded permutation handed out row-interleaved
(logical page j of every row in turn), so the consecutive logical pages of a
row are neither adjacent nor ordered. Every pool page no row owns is POISON:
decoy K (twice a query) and NaN V; every table entry past a row's last live
page names one poison page. A row's last live page keeps ragged_cases' guard
rows past the row's length.

A plain helper (not a conftest). Inputs are built once per key and shared.
"""

from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import torch

import needle_cases as nc
import ragged_cases as rc

PAGES = (128, 256)
# capacity 1024: the first keys of the pages that start no 512-key split and
# that the tests must hit (the issue's list; 128 is a ragged seam already)
PAGE_STARTS = {128: (128,), 256: (256, 768)}
SPARE = 5          # pool pages beyond the ones the rows own: all poison
PERM_SEED = 7
SETS = rc.LENGTH_SETS + rc.LENGTH_SETS_BIG
MUTANTS = ("identity", "row_b^1", "j+1", "j-1", "pid_lag",
           "pid_first_of_chunk", "head_layout", "head_swapped")
TILE = {"bf16": 64, "fp8": 128}    # keys per staged tile of the two kernels


def targets(lengths, page: int) -> torch.Tensor:
    """Head 0 of every row targets L_b - 1. Capacity 1024: the next heads
    take the page starts below L_b, the rest rotate, offset by b, over
    ragged_cases' seams. Capacity 4608: odd heads rotate over the first keys
    of the row's live splits (last split first, as in ragged_cases), even
    heads over ``s * 512 + page`` of its live splits (first split first)."""
    tg = torch.full((rc.B, rc.HQ), -1, dtype=torch.long)
    big = rc.cap_of(lengths) == rc.CAP_BIG
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        tg[b, 0] = n - 1
        if big:
            seams = [s for s in reversed(range(0, n, rc.CHUNK)) if s != n - 1]
            starts = [s + page for s in range(0, n, rc.CHUNK)
                      if s + page < n - 1]
        else:
            seams = [s for s in rc.SEAMS if s < n - 1]
            starts = [s for s in PAGE_STARTS[page]
                      if s < n - 1 and s not in seams]
        seams = seams or [n - 1]
        for h in range(1, rc.HQ):
            if big:
                i = (h - 1) // 2 + b
                pick = starts if (h % 2 == 0 and starts) else seams
                tg[b, h] = pick[i % len(pick)]
            elif h - 1 < len(starts):
                tg[b, h] = starts[h - 1]
            else:
                tg[b, h] = seams[(h + b) % len(seams)]
    return tg


@lru_cache(maxsize=None)
def build(lengths: tuple, dtype: str, page: int,
          family: str = "seam") -> rc.Ragged:
    """ragged_cases.build with this module's targets: same K/V draw, gain,
    guard pattern, pair rule and fp32 reference."""
    from tree_attention_torch_amd.ops.reference import flash_res_lse

    cap = rc.cap_of(lengths)
    k, v = rc.kv(dtype, cap)
    tg = targets(lengths, page)
    kvh = torch.arange(rc.HQ) // rc.G
    bi = torch.arange(rc.B)[:, None]
    idx = torch.where(tg >= 0, tg,
                      torch.arange(rc.HQ)[None, :].expand(rc.B, rc.HQ))
    qf = nc.needle_gain(rc.D) * k.float()[bi, kvh[None, :], idx]
    q = qf.to(torch.bfloat16)[:, :, None, :].contiguous()
    assert torch.equal(q.float()[:, :, 0], qf), "gain*K must be exact in bf16"
    tg2 = torch.full_like(tg, -1)
    if family == "pair":
        assert cap == rc.CAP_BIG
        for b, n in enumerate(lengths):
            live = -(-n // rc.CHUNK)
            for h in range(rc.HQ if live >= 3 else 0):
                tg2[b, h], q[b, h, 0] = nc.pair_key(
                    k[b, h // rc.G, :n].float(), int(tg[b, h]), live,
                    rc.CHUNK, nc.needle_gain(rc.D), 1.0 / rc.D ** 0.5,
                    dtype == "fp8", torch.bfloat16,
                    what=(lengths, dtype, page, b, h))
    else:
        assert family == "seam", family
    k_cache, v_cache = rc.with_guards(k, v, q, lengths)
    rg = rc.Ragged(tuple(lengths), dtype, rc.KIND[dtype], cap, k, v, q, tg,
                   k_cache, v_cache, None, None, tg2)
    rg.ref_out, rg.ref_lse = rc.attend_lengths(rg, lengths, flash_res_lse)
    return rg


@dataclass
class Pool:
    rg: rc.Ragged
    page: int
    n_pages: int
    max_pages: int
    k_pool: torch.Tensor    # (n_pages, Hkv, page, D), the cache's dtype
    v_pool: torch.Tensor
    table: torch.Tensor     # (B, max_pages) int32
    owned: list             # owned[b]: row b's pages, logical order
    poison: int             # the page every dead table entry names


def pages_of(n: int, page: int) -> int:
    return -(-n // page)


def scatter(rg: rc.Ragged, page: int) -> Pool:
    """rg's guarded cache scattered into a fresh pool (see the module
    docstring)."""
    max_pages = rg.cap // page
    need = [pages_of(n, page) for n in rg.lengths]
    n_pages = sum(need) + SPARE
    g = torch.Generator().manual_seed(PERM_SEED + page + rg.cap)
    perm = torch.randperm(n_pages, generator=g).tolist()
    gk, gv = rc.guard_fill(rg.q, rg.cap)
    td = rg.k_cache.dtype
    k_pool = torch.stack([gk[p % rc.B, :, :page] for p in range(n_pages)])
    k_pool = k_pool.to(td)
    v_pool = torch.full((n_pages, rc.HKV, page, rc.D), float("nan")).to(td)
    poison = perm[-1]
    table = torch.full((rc.B, max_pages), poison, dtype=torch.int32)
    owned = [[] for _ in range(rc.B)]
    it = iter(perm)
    for j in range(max_pages):
        for b in range(rc.B):
            if j < need[b]:
                pid = next(it)
                owned[b].append(pid)
                table[b, j] = pid
                k_pool[pid] = rg.k_cache[b, :, j * page:(j + 1) * page]
                v_pool[pid] = rg.v_cache[b, :, j * page:(j + 1) * page]
    assert poison not in [p for row in owned for p in row]
    return Pool(rg, page, n_pages, max_pages, k_pool, v_pool, table, owned,
                poison)


@lru_cache(maxsize=None)
def pool(lengths: tuple, dtype: str, page: int, family: str = "seam") -> Pool:
    """Shared and read-only: a test that writes takes scatter() of its own."""
    return scatter(build(lengths, dtype, page, family), page)


def gather(pl: Pool, mutant: str | None = None):
    """Attention of every row over the keys a paged reader collects, in
    fp64 (needle_cases.oracle): the true reader (mutant None) or one of
    MUTANTS. -> (out, lse) fp32."""
    rg, page, n_pages, max_pages = pl.rg, pl.page, pl.n_pages, pl.max_pages
    tile = TILE[rg.dtype]
    kf = pl.k_pool.float().reshape(n_pages * rc.HKV, page, rc.D)
    vf = pl.v_pool.float().reshape(n_pages * rc.HKV, page, rc.D)
    outs, lses = [], []
    for b, n in enumerate(rg.lengths):
        if n == 0:
            outs.append(torch.zeros(1, rc.HQ, 1, rc.D))
            lses.append(torch.full((1, rc.HQ, 1), float("-inf")))
            continue
        pos = torch.arange(n)
        j, off = pos // page, pos % page

        def entry(row, jj):
            return pl.table[row, jj.clamp(0, max_pages - 1)].long()

        pid = entry(b, j)
        if mutant == "identity":            # the table is ignored
            pid = (b * max_pages + j) % n_pages
        elif mutant == "row_b^1":           # another row's table
            pid = entry(b ^ 1, j)
        elif mutant == "j+1":
            pid = entry(b, j + 1)
        elif mutant == "j-1":
            pid = entry(b, j - 1)
        elif mutant == "pid_lag":
            # the id arrives one tile late: a page's first tile is read
            # from the page before, unless it starts a split chunk
            lag = (off < tile) & (pos % rc.CHUNK >= tile)
            pid = torch.where(lag, entry(b, j - 1), pid)
        elif mutant == "pid_first_of_chunk":
            pid = entry(b, (pos // rc.CHUNK) * (rc.CHUNK // page))
        ks, vs = [], []
        for h in range(rc.HKV):
            idx = pid * rc.HKV + h
            if mutant == "head_layout":     # pool read as (Hkv, n_pages)
                idx = h * n_pages + pid
            elif mutant == "head_swapped":
                idx = pid * rc.HKV + (h ^ 1)
            ks.append(kf[idx, off])
            vs.append(vf[idx, off])
        o, l = nc.oracle(rg.q[b:b + 1].float(), torch.stack(ks)[None],
                         torch.stack(vs)[None])
        outs.append(o.float())
        lses.append(l.float())
    return torch.cat(outs), torch.cat(lses)


def contiguous(pl: Pool):
    """The pool read back through the true table into (B, Hkv, cap, D)
    caches; positions past a row's last live page come from the poison
    page."""
    idx = pl.table.long()                                   # (B, max_pages)
    out = []
    for p in (pl.k_pool, pl.v_pool):
        raw = p.view(torch.uint8)[idx]     # (B, max_pages, Hkv, page, bytes)
        out.append(raw.permute(0, 2, 1, 3, 4).reshape(
            rc.B, rc.HKV, pl.max_pages * pl.page, -1).contiguous()
            .view(p.dtype))
    return out
