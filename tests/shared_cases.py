"""Shared-prefix decode inputs: rows of a paged pool that hold the same
leading pages, the groups and prefixes the plan rule predicts for them, and a
plain-torch model of the two passes (prefix pass per group, suffix pass per
row, one merge) with the ways they can go wrong.

A case is a list of rows (src, fork, length): the row's first `fork` tokens
are row `src`'s (src < 0: a row of its own) and it holds `length` tokens in
all. Pages that lie wholly below the fork point carry the source's ids; every
other page is the row's own (as after the copy-on-write of its tail). Page ids
come from a seeded permutation, every page no row owns is POISON as in
paged_cases / fork_cases (decoy K = twice a query, NaN V), a row's last page
keeps poison rows past its length, and every table entry past a row's live
pages names a poison page.

The scenario (scenario(), B = 6, Hq = 8, Hkv = 2: four rows per group, D = 128,
capacity 1024 = two 512-key splits, pages 128 and 256):
  row 0  a prompt of 700 tokens: at page 128 five full pages = 640 shared
         keys, so the prefix covers split 0 and 128 keys of split 1 and the
         suffix starts inside split 1
  row 1  forked at 700: a shared partial tail that is no part of the prefix
  row 2  forked at 640, on the prefix boundary: before its first append its
         suffix is empty
  row 3  forked at 700, then 3 own tokens
  row 4  forked at 700 (layout "fork"): the family has five rows, so the cut
         leaves a group of four and a lone row with prefix 0; or (layout
         "mixed") an unrelated row of 65 tokens
  row 5  empty: zeros, lse -inf
Checkpoints are the state after n = 0, 1 and STEPS = 130 decode steps of rows
0..4.

Needles (needle_cases.needle_gain): per member and head the targets rotate
over key 0, keys 511 and 512 (the split seam), the last prefix key P - 1, the
first own key P and the row's last key, and no two members of a group have the
same target on the same head: a query gathered from the wrong member, or a
partial scattered to the wrong one, names the wrong key.

A plain helper (not a conftest). Inputs are built once per key and shared.
"""

from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import torch

import needle_cases as nc

SEED = 20261022
D = 128
CHUNK = 512
PAGES = (128, 256)
DTYPES = ("bf16", "fp8")
KIND = {"bf16": "half", "fp16": "half", "fp8": "fp8"}
_TD = {"bf16": torch.bfloat16, "fp16": torch.float16,
       "fp8": torch.float8_e4m3fn}
SPARE = 5
PERM_SEED = 11

B, HQ, HKV, CAP = 6, 8, 2, 1024
PROMPT, STEPS = 700, 130
LAYOUTS = ("fork", "mixed")
ACTIVE = (True, True, True, True, True, False)
CHECKPOINTS = (0, 1, STEPS)
# What the plan rule gives for the scenario, at every checkpoint and in both
# layouts: rows 0..3 tie on their five (page 128) or two (page 256) shared
# full pages and sort by index, the cut after 16 / G = 4 rows leaves row 4
# alone (in "mixed" it has no full page before step 63 and no shared one
# ever), row 5 is empty.
EXPECT = {
    128: [([0, 1, 2, 3], 640), ([4], 0), ([5], 0)],
    256: [([0, 1, 2, 3], 512), ([4], 0), ([5], 0)],
}
MUTANTS = ("prefix-1page", "prefix+1page", "start-1page", "start+1page",
           "gather_j+1", "scatter_j+1", "tail_via_nonleader", "count-1",
           "suffix_only")
# start-1page counts a page of keys twice: a needle row keeps its one-hot
# weights, so `out` does not move, and lse grows by ln 2 where the needle is
# in that page. Everything else loses or mixes a needle, or reads poison, and
# moves `out`.
LSE_ONLY = ("start-1page",)


def scenario(layout: str, n: int = 0) -> tuple:
    """The rows (src, fork, length) after n decode steps."""
    assert layout in LAYOUTS, layout
    r4 = (0, PROMPT, PROMPT + n) if layout == "fork" else (-1, 0, 65 + n)
    return ((-1, 0, PROMPT + n), (0, PROMPT, PROMPT + n), (0, 640, 640 + n),
            (0, PROMPT, PROMPT + 3 + n), r4, (-1, 0, 0))


def pages_of(n: int, page: int) -> int:
    return -(-n // page)


def plan_of(pages, lens, refs, page: int, per: int) -> list:
    """The plan rule, written out on its own: -> [(rows, prefix tokens)]."""
    full = [n // page for n in lens]
    fams, groups = {}, []
    for b, f in enumerate(full):
        if f:
            fams.setdefault(pages[b][0], []).append(b)
        else:
            groups.append(([b], 0))

    def run(b):
        ids = []
        for pid in pages[b][:full[b]]:
            if refs[pid] < 2:
                break
            ids.append(pid)
        return ids

    for fam in fams.values():
        fam.sort(key=lambda b: (run(b), b))
        for i in range(0, len(fam), per):
            rows = fam[i:i + per]
            n = 0
            if len(rows) > 1:
                while (n < min(full[b] for b in rows)
                       and len({pages[b][n] for b in rows}) == 1):
                    n += 1
            groups.append((rows, n * page))
    return sorted(groups, key=lambda g: min(g[0]))


@dataclass
class Case:
    rows: tuple
    hq: int
    hkv: int
    page: int
    dtype: str
    cap: int
    lengths: tuple
    k: torch.Tensor          # (B, Hkv, cap, D) storage dtype: row b's stream
    v: torch.Tensor
    q: torch.Tensor          # (B, Hq, 1, D) bf16 (fp16 for an fp16 pool)
    targets: torch.Tensor    # (B, Hq); -1: empty row
    owned: list              # owned[b]: row b's page ids, logical order
    plan: list               # [(rows, prefix)]
    n_pages: int
    k_pool: torch.Tensor     # (n_pages, Hkv, page, D) storage dtype
    v_pool: torch.Tensor
    table: torch.Tensor      # (B, max_pages) int32
    poison: int
    ref_out: torch.Tensor    # fp32 oracle (B, Hq, 1, D)
    ref_lse: torch.Tensor

    @property
    def kind(self) -> str:
        return KIND[self.dtype]

    def tables(self, n_groups: int | None = None):
        """members (n, 16) int32, counts (n,) int32, prefix (n,) int64 and
        start (B,) int64 of the plan; groups past the plan have count 0."""
        n = n_groups or len(self.plan)
        members = torch.zeros(n, 16, dtype=torch.int32)
        counts = torch.zeros(n, dtype=torch.int32)
        prefix = torch.zeros(n, dtype=torch.long)
        start = torch.zeros(len(self.rows), dtype=torch.long)
        for g, (rows, p) in enumerate(self.plan):
            members[g, :len(rows)] = torch.tensor(rows, dtype=torch.int32)
            counts[g], prefix[g] = len(rows), p
            start[rows] = p
        return members, counts, prefix, start


@lru_cache(maxsize=None)
def streams(rows: tuple, hkv: int, dtype: str, cap: int):
    """(B, Hkv, cap, D) K and V in the storage dtype: every row its own draw
    behind the tokens it took from its source."""
    g = torch.Generator().manual_seed(SEED + cap + 7 * len(rows) + hkv)
    k = torch.randn(len(rows), hkv, cap, D, generator=g).to(_TD[dtype])
    v = torch.randn(len(rows), hkv, cap, D, generator=g).to(_TD[dtype])
    for b, (src, fork, _) in enumerate(rows):
        if src >= 0:
            assert src < b
            k[b, :, :fork] = k[src, :, :fork]
            v[b, :, :fork] = v[src, :, :fork]
    return k, v


def _own_pages(rows, page):
    """owned[b] with fresh ids 0, 1, ... in logical order (before the
    permutation), and the number of ids used."""
    owned, nxt = [], 0
    for src, fork, n in rows:
        ids = list(owned[src][:fork // page]) if src >= 0 else []
        while len(ids) < pages_of(n, page):
            ids.append(nxt)
            nxt += 1
        owned.append(ids)
    return owned, nxt


def _targets(lens, plan, hq, hkv):
    tg = torch.full((len(lens), hq), -1, dtype=torch.long)
    for members, prefix in plan:
        for h in range(hq):
            used = set()
            for b in members:
                n = lens[b]
                if n == 0:
                    continue
                cand = [c for c in (0, CHUNK - 1, CHUNK, prefix - 1, prefix,
                                    n - 1) if 0 <= c < n]
                order = [cand[(h + b + i) % len(cand)]
                         for i in range(len(cand))]
                free = [c for c in order if c not in used]
                # (more members than candidate keys: a far key of its own)
                pick = free[0] if free else next(
                    c for c in range(n - 2, -1, -1) if c not in used)
                used.add(pick)
                tg[b, h] = pick
    return tg


@lru_cache(maxsize=None)
def build(rows: tuple, hq: int, hkv: int, page: int, dtype: str,
          cap: int, gone: tuple = ()) -> Case:
    """`gone`: rows that have left since (reset): they hold nothing and name
    no page, the rows forked from them keep what they took."""
    from tree_attention_torch_amd.ops.reference import flash_res_lse

    nb, g = len(rows), hq // hkv
    lens = tuple(0 if b in gone else r[2] for b, r in enumerate(rows))
    assert max(lens) <= cap and cap % page == 0
    k, v = streams(rows, hkv, dtype, cap)
    logical, used = _own_pages(rows, page)
    n_pages = used + SPARE
    gen = torch.Generator().manual_seed(PERM_SEED + page + cap + nb)
    perm = torch.randperm(n_pages, generator=gen).tolist()
    owned = [[] if b in gone else [perm[i] for i in ids]
             for b, ids in enumerate(logical)]
    poison = perm[-1]
    refs = [0] * n_pages
    for ids in owned:
        for pid in ids:
            refs[pid] += 1
    plan = plan_of(owned, lens, refs, page, 16 // g)
    tg = _targets(lens, plan, hq, hkv)
    kvh = torch.arange(hq) // g
    bi = torch.arange(nb)[:, None]
    idx = torch.where(tg >= 0, tg, torch.arange(hq)[None, :].expand(nb, hq))
    qf = nc.needle_gain(D) * k.float()[bi, kvh[None, :], idx]
    qd = torch.float16 if dtype == "fp16" else torch.bfloat16
    q = qf.to(qd)[:, :, None, :].contiguous()
    assert torch.equal(q.float()[:, :, 0], qf), "gain*K must be exact in q"
    # pools: poison everywhere, then the rows' pages (a shared page is
    # written by its first holder; later holders write the same bytes)
    j = torch.arange(page)
    heads = torch.arange(hkv)[:, None] * g + (j % g)[None, :]
    gk = 2.0 * q.float()[:, heads, 0]                    # (B, Hkv, page, D)
    td = _TD[dtype]
    k_pool = torch.stack([gk[p % nb] for p in range(n_pages)]).to(td)
    v_pool = torch.full((n_pages, hkv, page, D), float("nan")).to(td)
    max_pages = cap // page
    table = torch.full((nb, max_pages), poison, dtype=torch.int32)
    for b, ids in enumerate(owned):
        for jj, pid in enumerate(ids):
            lo, hi = jj * page, min((jj + 1) * page, lens[b])
            k_pool[pid, :, :hi - lo] = k[b, :, lo:hi]
            v_pool[pid, :, :hi - lo] = v[b, :, lo:hi]
            table[b, jj] = pid
    outs, lses = [], []
    for b, n in enumerate(lens):
        if n == 0:
            outs.append(torch.zeros(1, hq, 1, D))
            lses.append(torch.full((1, hq, 1), float("-inf")))
            continue
        o, l = flash_res_lse(q[b:b + 1].float(), k[b:b + 1, :, :n].float(),
                             v[b:b + 1, :, :n].float())
        outs.append(o.float())
        lses.append(l.float())
    return Case(rows, hq, hkv, page, dtype, cap, lens, k, v, q, tg, owned,
                plan, n_pages, k_pool, v_pool, table, poison,
                torch.cat(outs), torch.cat(lses))


def at(layout: str, page: int, dtype: str, n: int, gone: tuple = ()) -> Case:
    """The scenario after n decode steps (and the reset of the rows `gone`)."""
    return build(scenario(layout, n), HQ, HKV, page, dtype, CAP, gone)


def coverage(cs: Case) -> set:
    """Which kinds of target the case's needles hit."""
    seen = set()
    lens = cs.lengths
    for rows, p in cs.plan:
        for b in rows:
            for t in cs.targets[b].tolist():
                for name, key in (("key0", 0), ("seam-1", CHUNK - 1),
                                  ("seam", CHUNK), ("P-1", p - 1), ("P", p),
                                  ("last", lens[b] - 1)):
                    if t == key and (p or name not in ("P-1", "P")):
                        seen.add(name)
    return seen


def compare(cs: Case, out, lse, what: str = "") -> None:
    """Live rows at the kind's unchanged bars (nc.compare); an empty row by
    equality: out = 0 and lse = -inf."""
    out = out.detach().float().cpu()
    lse = None if lse is None else lse.detach().float().cpu()
    live = torch.tensor([n > 0 for n in cs.lengths])
    try:
        nc.compare(out[live], None if lse is None else lse[live],
                   cs.ref_out[live], cs.ref_lse[live], cs.kind)
        assert torch.equal(out[~live], torch.zeros_like(out[~live])), \
            "an empty row must be all zeros"
        if lse is not None:
            assert bool((lse[~live] == float("-inf")).all()), \
                "an empty row's lse must be -inf"
    except AssertionError as e:
        raise AssertionError(
            f"shared {cs.dtype} page {cs.page} lengths {cs.lengths} {what}\n"
            f"{e}") from None


def rejected(cs: Case, out, lse) -> bool:
    try:
        compare(cs, out, lse)
    except AssertionError:
        return True
    return False


# --------------------------------------------------------------------------
# the two passes in plain torch
# --------------------------------------------------------------------------
def _keys(cs: Case, row: int, lo: int, hi: int):
    """(1, Hkv, hi - lo, D) fp32 K and V of local positions [lo, hi) as read
    through `row`'s table row."""
    pos = torch.arange(lo, hi)
    pid = cs.table[row, (pos // cs.page).clamp(0, cs.table.shape[1] - 1)]
    off = pos % cs.page
    k = cs.k_pool.float()[pid.long(), :, off].permute(1, 0, 2)[None]
    v = cs.v_pool.float()[pid.long(), :, off].permute(1, 0, 2)[None]
    return k, v


def model(cs: Case, mutant: str | None = None):
    """(out, lse) of the two passes over the case's pool and plan: per group
    one prefix partial per member from the LEADER's pages, per row one suffix
    partial from its own, merged by combine_partials. `mutant`: one of
    MUTANTS."""
    from tree_attention_torch_amd.parallel.combine import combine_partials

    assert mutant is None or mutant in MUTANTS, mutant
    nb, page = len(cs.rows), cs.page
    out = torch.zeros(2, nb, cs.hq, 1, D)
    lse = torch.full((2, nb, cs.hq, 1), float("-inf"))
    members, counts, prefix, start = (t.clone() for t in cs.tables())
    big = prefix > 0      # the mutants act on the groups that have a prefix
    if mutant == "prefix-1page":
        prefix[big] -= page
    elif mutant == "prefix+1page":
        prefix[big] += page
    elif mutant in ("start-1page", "start+1page"):
        step = -page if mutant == "start-1page" else page
        for g in torch.nonzero(big).flatten().tolist():
            rows = members[g, :counts[g]].long()
            start[rows] = (start[rows] + step).clamp(min=0)
    elif mutant == "count-1":
        counts[big] -= 1
    elif mutant == "tail_via_nonleader":
        # the prefix taken as the pages of the fork point, the partial tail
        # page included, and read through a member that has since copied its
        # tail and written behind it
        for g in torch.nonzero(big).flatten().tolist():
            rows = members[g, :counts[g]].tolist()
            fork = pages_of(max(cs.rows[b][1] for b in rows), page) * page
            prefix[g] = fork
            start[rows] = fork
            members[g, :len(rows)] = torch.tensor(rows[1:] + rows[:1],
                                                  dtype=torch.int32)
    for g in range(len(cs.plan)):
        c, p = int(counts[g]), int(prefix[g])
        rows = members[g, :c].tolist()
        if not rows or p <= 0:
            continue
        k, v = _keys(cs, rows[0], 0, min(p, cs.cap))
        for j, b in enumerate(rows):
            src = rows[(j + 1) % c] if mutant == "gather_j+1" else b
            dst = rows[(j + 1) % c] if mutant == "scatter_j+1" else b
            o, l = nc.oracle(cs.q[src:src + 1].float(), k, v)
            out[0, dst], lse[0, dst] = o[0].float(), l[0].float()
    for b, n in enumerate(cs.lengths):
        s = int(start[b]) // 128 * 128
        if n > s:
            k, v = _keys(cs, b, s, n)
            o, l = nc.oracle(cs.q[b:b + 1].float(), k, v)
            out[1, b], lse[1, b] = o[0].float(), l[0].float()
    if mutant == "suffix_only":
        out, lse = out[1:], lse[1:]
    return combine_partials(out, lse)


# --------------------------------------------------------------------------
# the scenario on a PagedDecodeSession
# --------------------------------------------------------------------------
def fed(layout: str, dtype: str):
    """The final streams as a session is fed them: bf16 tensors whose cast to
    the cache dtype gives the stored bits back."""
    k, v = streams(scenario(layout, STEPS), HKV, dtype, CAP)
    return k.float().bfloat16(), v.float().bfloat16()


def pool_pages(page: int) -> int:
    """Pages of the final lengths held independently, plus the spare ones."""
    return sum(pages_of(r[2], page) for r in scenario("fork", STEPS)) + SPARE


def load(sess, layout: str, dtype: str, device="cpu"):
    """Row 0's prompt, the forks, row 3's three own tokens (and row 4's own
    prefill in "mixed"). -> the fed streams."""
    ks, vs = (t.to(device) for t in fed(layout, dtype))
    rows = scenario(layout, 0)
    sess.prefill(0, ks[0, :, :PROMPT], vs[0, :, :PROMPT])
    for b, (src, fork, n) in enumerate(rows):
        if b == 0 or n == 0:
            continue
        if src >= 0:
            sess.fork(src, b, fork)
        if n > fork:
            sess.prefill(b, ks[b, :, fork:n], vs[b, :, fork:n])
    assert sess.totals == [r[2] for r in rows]
    return ks, vs


def step_tokens(ks, vs, layout: str, i: int):
    """(B, Hkv, 1, D) K and V of decode step i (row 5 never takes one)."""
    at_ = torch.tensor([min(r[2], CAP - 1) for r in scenario(layout, i)])
    bi = torch.arange(B)
    return ks[bi, :, at_][:, :, None], vs[bi, :, at_][:, :, None]


def poison(sess, q) -> None:
    """Decoy K and NaN V over the session's free pages, in place; every
    table entry past a row's live pages names a free page."""
    g, page = HQ // HKV, sess.page
    j = torch.arange(page)
    heads = torch.arange(HKV)[:, None] * g + (j % g)[None, :]
    gk = 2.0 * q.float().cpu()[:, heads, 0]
    for pid in sess._free:
        sess.k_pool[pid] = gk[pid % B].to(device=sess.k_pool.device,
                                          dtype=sess.k_pool.dtype)
        sess.v_pool[pid] = float("nan")
    for b in range(B):
        sess.page_table[b, len(sess._pages[b]):] = sess._free[0]


def table_matches(sess) -> None:
    for b, ids in enumerate(sess._pages):
        assert sess.page_table[b, :len(ids)].tolist() == ids, b
        assert len(ids) == pages_of(sess.local_lens[b], sess.page), b


def one_group_each(plan, batch: int) -> None:
    """Every row is in exactly one group."""
    rows = sorted(b for members, _ in plan for b in members)
    assert rows == list(range(batch)), plan
