"""Prefix sharing inputs: a byte-level model of kv_pool_copy_rows, and the fork
scenario every fork test runs, with a plain-torch model of a paged pool that
forks and copies on write.

The scenario (B, Hq, Hkv, D and the K/V draw of tests/ragged_cases.py). Row 0
is prefilled with PREFIX = 300 tokens; rows 1..3 are forked from it at
FORKS[page]. At page 128 the fork points 129, 255 and 128 give copies of 1
and of 127 rows and a fork on a page boundary, which copies nothing; row 0's
own tail is 44 rows of a page nobody shares. At page 256 the fork points 300,
129 and 256 give a tail page that row 0 itself shares with a fork, a copy of
129 rows, and another boundary. Then every row, row 0 included, continues
with STEPS = 130 tokens of its OWN stream (row b's draw from its start on):
each continuation starts inside the page it shared (or on its boundary), at
the offset its siblings' data or continuation occupies, and at page 128
crosses a page boundary. A write in place therefore lands on a sibling.

The queries are needles (needle_cases.needle_gain). Heads h and h + 4 of a
row (KV heads 0 and 1) target, for h = 0..3: the row's last key, the last
shared key start - 1, the row's first own key `start`, and key 0. Checkpoints
are `at(page, dtype, n)`: the state after n continuation steps, and
`after_reset(page, dtype)`: the final state once row 0 has left.

Every pool page the scenario does not own is poison as in paged_cases: decoy
K (twice a query), NaN V.

A plain helper (not a conftest). Inputs are built once per key and shared.
"""

from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import torch

import needle_cases as nc
import paged_cases as pc
import ragged_cases as rc

PAGES = (128, 256)
PREFIX = 300
STEPS = 130
FORKS = {128: (129, 255, 128), 256: (300, 129, 256)}
SPARE = pc.SPARE
COPY_MUTANTS = ("no_copy", "rows-1", "k_only", "head_layout",
                "src_dst_swapped", "whole_page")
SESSION_MUTANTS = ("in_place", "free_early")
# What the rules of the issue predict, row by row, when the rows take their
# first continuation token one after the other (row 0 first): pages taken
# (a copy or a fresh page), the (row, rows copied) of the copies, and the
# pages more than one row holds after the fork / after those appends.
#   page 128: rows 1 and 2 leave the page of positions [128, 256) (1 and 127
#     rows), row 3 opens a page at 128; row 0 wrote its own tail in place.
#   page 256: row 0 leaves the tail page it shares with row 1 (44 rows), so
#     row 1 then writes in place; row 2 leaves page 0 (129 rows); row 3 opens
#     a page at 256.
EXPECT = {
    128: dict(shared_forked=2, taken=(0, 1, 1, 1), copies=((1, 1), (2, 127)),
              shared_after=1),
    256: dict(shared_forked=2, taken=(1, 0, 1, 1), copies=((0, 44), (2, 129)),
              shared_after=1),
}


def starts(page: int) -> tuple:
    """Tokens every row holds when its continuation begins."""
    return (PREFIX,) + FORKS[page]


def lengths_at(page: int, n: int) -> tuple:
    return tuple(s + n for s in starts(page))


def pool_pages(page: int) -> int:
    """Pages of the final lengths, held independently, plus the spare ones."""
    return sum(pc.pages_of(s + STEPS, page) for s in starts(page)) + SPARE


# --------------------------------------------------------------------------
# kv_pool_copy_rows, byte for byte
# --------------------------------------------------------------------------
def copy_rows(k_pool, v_pool, triples, mutant: str | None = None) -> None:
    """IN PLACE: for each (src, dst, rows) the first `rows` rows of every
    head of page src go to page dst, in both (n_pages, Hkv, page, D) pools,
    as bytes. `mutant` is one of COPY_MUTANTS."""
    assert mutant is None or mutant in COPY_MUTANTS, mutant
    n_pages, hkv, page, _ = k_pool.shape
    if mutant == "no_copy":
        return
    for pool in (k_pool,) if mutant == "k_only" else (k_pool, v_pool):
        assert pool.is_contiguous()
        flat = pool.view(torch.uint8).view(n_pages * hkv, page, -1)
        for src, dst, rows in triples:
            if mutant == "src_dst_swapped":
                src, dst = dst, src
            r = {"rows-1": max(rows - 1, 0), "whole_page": page}.get(mutant,
                                                                    rows)
            for h in range(hkv):
                if mutant == "head_layout":     # pool read as (Hkv, n_pages)
                    si, di = h * n_pages + src, h * n_pages + dst
                else:
                    si, di = src * hkv + h, dst * hkv + h
                flat[di, :r] = flat[si, :r].clone()


# --------------------------------------------------------------------------
# the scenario
# --------------------------------------------------------------------------
@lru_cache(maxsize=None)
def streams(page: int, dtype: str):
    """(B, Hkv, CAP, D) K and V in the cache dtype: row b's whole sequence,
    the shared prefix of row 0 up to its start and its own draw from there."""
    k, v = (t.clone() for t in rc.kv(dtype))
    for b, s in enumerate(starts(page)):
        k[b, :, :s] = k[0, :, :s]
        v[b, :, :s] = v[0, :, :s]
    return k, v


def fed(page: int, dtype: str):
    """The streams as a session is fed them (ragged_cases.stream): bf16
    tensors whose cast to the cache dtype gives the stored bits back."""
    k, v = streams(page, dtype)
    return k.float().bfloat16(), v.float().bfloat16()


def step_tokens(ks, vs, page: int, i: int):
    """(B, Hkv, 1, D) K and V of continuation step i."""
    at = torch.tensor(starts(page)) + i
    bi = torch.arange(rc.B)
    return ks[bi, :, at][:, :, None], vs[bi, :, at][:, :, None]


def targets(page: int, lengths) -> torch.Tensor:
    tg = torch.full((rc.B, rc.HQ), -1, dtype=torch.long)
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        s = starts(page)[b]
        for h in range(rc.HQ):
            tg[b, h] = (n - 1, s - 1, min(s, n - 1), 0)[h % 4]
    return tg


def _build(page: int, dtype: str, lengths: tuple) -> rc.Ragged:
    from tree_attention_torch_amd.ops.reference import flash_res_lse

    k, v = streams(page, dtype)
    tg = targets(page, lengths)
    kvh = torch.arange(rc.HQ) // rc.G
    bi = torch.arange(rc.B)[:, None]
    idx = torch.where(tg >= 0, tg,
                      torch.arange(rc.HQ)[None, :].expand(rc.B, rc.HQ))
    qf = nc.needle_gain(rc.D) * k.float()[bi, kvh[None, :], idx]
    q = qf.to(torch.bfloat16)[:, :, None, :].contiguous()
    assert torch.equal(q.float()[:, :, 0], qf), "gain*K must be exact in bf16"
    k_cache, v_cache = rc.with_guards(k, v, q, lengths)
    rg = rc.Ragged(tuple(lengths), dtype, rc.KIND[dtype], rc.CAP, k, v, q,
                   tg, k_cache, v_cache, None, None)
    rg.ref_out, rg.ref_lse = rc.attend_lengths(rg, lengths, flash_res_lse)
    return rg


@lru_cache(maxsize=None)
def at(page: int, dtype: str, n: int) -> rc.Ragged:
    """The needles and the fp32 oracle after n continuation steps."""
    return _build(page, dtype, lengths_at(page, n))


@lru_cache(maxsize=None)
def after_reset(page: int, dtype: str) -> rc.Ragged:
    """The final state with row 0 gone (an empty row: zeros)."""
    return _build(page, dtype, (0,) + lengths_at(page, STEPS)[1:])


def load(sess, page: int, dtype: str, forked: bool, device="cpu"):
    """Row 0's prefix, then rows 1..3 by fork() or, `forked` False, each
    prefilled on its own with the same tokens. -> the fed streams."""
    ks, vs = (t.to(device) for t in fed(page, dtype))
    sess.prefill(0, ks[0, :, :PREFIX], vs[0, :, :PREFIX])
    for b in range(1, rc.B):
        s = starts(page)[b]
        if forked:
            sess.fork(0, b, s)
        else:
            sess.prefill(b, ks[b, :, :s], vs[b, :, :s])
    assert sess.totals == list(starts(page))
    assert sess.total_dev.tolist() == sess.totals
    assert sess.local_len_dev.tolist() == sess.local_lens
    return ks, vs


def poison(sess, q, pids=None) -> None:
    """paged_cases' poison, in place, over the session's free pages (or
    `pids`): decoy K, NaN V; every table entry past a row's live pages names
    a free page."""
    gk, _ = rc.guard_fill(q.cpu(), rc.CAP)
    td, page = sess.k_pool.dtype, sess.page
    for pid in (sess._free if pids is None else pids):
        sess.k_pool[pid] = gk[pid % rc.B, :, :page].to(
            device=sess.k_pool.device, dtype=td)
        sess.v_pool[pid] = float("nan")
    if sess._free:
        for b in range(rc.B):
            sess.page_table[b, len(sess._pages[b]):] = sess._free[0]


def table_matches(sess) -> None:
    for b, ids in enumerate(sess._pages):
        assert sess.page_table[b, :len(ids)].tolist() == ids, b
        assert len(ids) == pc.pages_of(sess.local_lens[b], sess.page), b


# --------------------------------------------------------------------------
# a paged pool that forks, in plain torch: what the tests can see
# --------------------------------------------------------------------------
class PoolModel:
    """Pages, counts and a free list on the host, the pools in torch, the
    copies through copy_rows. `copy_mutant` goes to copy_rows;
    `session_mutant` is "in_place" (a shared tail page is written where it
    lies, no copy) or "free_early" (a page goes back to the free list the
    first time a row lets go of it, whatever its count). A page that goes
    back is poisoned at once, and every page starts out poisoned."""

    def __init__(self, page: int, dtype: str, q, copy_mutant=None,
                 session_mutant=None):
        assert session_mutant is None or session_mutant in SESSION_MUTANTS
        self.page, self.dtype = page, dtype
        self.copy_mutant, self.session_mutant = copy_mutant, session_mutant
        self.n_pages = pool_pages(page)
        td = rc._TD[dtype]
        self.gk, _ = rc.guard_fill(q, rc.CAP)
        self.k_pool = torch.zeros(self.n_pages, rc.HKV, page, rc.D).to(td)
        self.v_pool = torch.zeros_like(self.k_pool)
        self.refs = [0] * self.n_pages
        self.free = list(range(self.n_pages - 1, -1, -1))
        self.pages = [[] for _ in range(rc.B)]
        self.lens = [0] * rc.B
        for pid in range(self.n_pages):
            self._poison(pid)

    def _poison(self, pid: int) -> None:
        self.k_pool[pid] = self.gk[pid % rc.B, :, :self.page].to(
            self.k_pool.dtype)
        self.v_pool[pid] = float("nan")

    def _take(self) -> int:
        pid = self.free.pop()
        self.refs[pid] = 1
        return pid

    def _unref(self, pid: int) -> None:
        self.refs[pid] = max(self.refs[pid] - 1, 0)
        gone = self.refs[pid] == 0 or self.session_mutant == "free_early"
        if gone and pid not in self.free:
            self.free.append(pid)
            self._poison(pid)

    def write(self, b: int, k_rows, v_rows) -> None:
        """Append (Hkv, n, D) rows, in the pool's dtype, to row b."""
        for i in range(k_rows.shape[1]):
            pos, page = self.lens[b], self.page
            j, off = pos // page, pos % page
            if off == 0:
                self.pages[b].append(self._take())
            elif (self.refs[self.pages[b][j]] > 1
                  and self.session_mutant != "in_place"):
                old, new = self.pages[b][j], self._take()
                copy_rows(self.k_pool, self.v_pool, [(old, new, off)],
                          self.copy_mutant)
                self.pages[b][j] = new
                self._unref(old)
            pid = self.pages[b][j]
            self.k_pool[pid, :, off] = k_rows[:, i]
            self.v_pool[pid, :, off] = v_rows[:, i]
            self.lens[b] = pos + 1

    def fork(self, src: int, dst: int, tokens: int) -> None:
        assert not self.pages[dst]
        self.pages[dst] = self.pages[src][:pc.pages_of(tokens, self.page)]
        for pid in self.pages[dst]:
            self.refs[pid] += 1
        self.lens[dst] = tokens

    def reset(self, b: int) -> None:
        for pid in reversed(self.pages[b]):
            self._unref(pid)
        self.pages[b], self.lens[b] = [], 0

    def pool(self, rg: rc.Ragged) -> pc.Pool:
        """What a paged reader is handed: paged_cases.gather reads it."""
        assert tuple(self.lens) == rg.lengths
        max_pages = rc.CAP // self.page
        dead = self.free[0]
        table = torch.full((rc.B, max_pages), dead, dtype=torch.int32)
        for b, ids in enumerate(self.pages):
            table[b, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
        return pc.Pool(rg, self.page, self.n_pages, max_pages, self.k_pool,
                       self.v_pool, table, self.pages, dead)


def model_checkpoints(page: int, dtype: str, copy_mutant=None,
                      session_mutant=None):
    """Run the scenario through PoolModel -> [(what, rg, out, lse)] at the
    three checkpoints: after step 1, after step STEPS, after reset(0)."""
    k, v = streams(page, dtype)
    m = PoolModel(page, dtype, at(page, dtype, STEPS).q, copy_mutant,
                  session_mutant)
    m.write(0, k[0, :, :PREFIX], v[0, :, :PREFIX])
    for b in range(1, rc.B):
        m.fork(0, b, starts(page)[b])
    seen = []

    def look(what, rg):
        seen.append((what, rg) + pc.gather(m.pool(rg)))

    for i in range(STEPS):
        for b, s in enumerate(starts(page)):
            m.write(b, k[b, :, s + i:s + i + 1], v[b, :, s + i:s + i + 1])
        if i == 0:
            look("step 1", at(page, dtype, 1))
    look(f"step {STEPS}", at(page, dtype, STEPS))
    m.reset(0)
    look("row 0 gone", after_reset(page, dtype))
    return seen
