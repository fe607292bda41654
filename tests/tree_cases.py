"""Draft-tree needle inputs: T draft nodes per batch row, one ancestor mask
per (row, query position).

The construction of tests/spec_cases.py (docs/NEEDLE_TESTS.md): B = 4,
Hq = 8, Hkv = 2, D = 128 over a cache of capacity 1024 (two 512-key splits,
64- and 128-key tiles), the same K/V draw, gain and guard pattern. Sequence b
holds starts[b] tokens and takes counts[b] of T draft NODES, node j at
position starts[b] + j with parent parents[b][j] in [-1, j - 1] (-1: the last
committed token). Query i < counts[b] sees the prefix [0, starts[b]) and the
nodes of anc(i) = {i, parent(i), ...}; a query at or past counts[b] the prefix
alone. What a query sees is written the way the kernels read it,

    key pos is visible  iff  pos < base  or  bit (pos - base) of bits is set
                             (pos - base < 16),

with base = starts[b] and bits = the ancestor set at world size 1, so every
mask error is another (base, bits). Every cache row at or past lengths[b] =
starts[b] + counts[b] holds a decoy K and a NaN V.

Starts put the drafts across the split seam 511 | 512 (510), the 64-key tile
seam (62), the 128-key tile and page seam (126) and at 0 (the drafts are the
whole sequence); rows with count 0, one of them empty (out = 0, lse = -inf).
Trees: a chain, a star, two branches at T = 6 (two launches of 4 and 2 query
positions; node 4 hangs off node 2 across the group boundary), a different
tree in every batch row, and 16 nodes of depth 6.

Query families, by the head's place g = h % G in its KV group:
  own  (g = 0): gain * K of the query's own node (at or past counts[b]: the
                last key of the prefix). A mask without self loses it.
  root (g = 1): gain * K of the query's ROOT-MOST ancestor: a mask without
                the transitive closure loses it (a root: own).
  sib  (g = 2): the highest lower-indexed node that is NO ancestor, masked
                by the tree and visible to a chain mask (at or past
                counts[b]: the last node taken; none: own). ANCHORED, as
                needle_cases' first_masked is: q = 4 K[own] + 6 K[sib],
                rounded to the query dtype (fp8: to e4m3 first, which the
                kernel casts Q to) and read back by the oracle. A query on
                the hidden key alone leaves a diffuse softmax over the few
                visible keys, where e4m3's 2^-4 step on a p ~ 0.5 is past the
                bar by the format's own precision; the anchor keeps the right
                answer one-hot, and a mask that admits the sibling (score
                ~68 against ~45) hands it the row.
  seam (g = 3): gain * K of a prefix key on a tile, page or split seam (no
                prefix: own).

This module is a plain helper (not a conftest). Inputs are built once per
case and shared, unchanged, by every test.
"""

from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import torch

import needle_cases as nc
import ragged_cases as rc

B, HQ, HKV, D, CAP, G = rc.B, rc.HQ, rc.HKV, rc.D, rc.CAP, rc.G
DTYPES = rc.DTYPES
PER_CALL = 16 // G     # query positions one launch carries
SLOTS = 16             # draft slots a mask holds

CHAIN4 = (-1, 0, 1, 2)
STAR4 = (-1, -1, -1, -1)
TWO6 = (-1, 0, 0, 1, 2, 2)
DEEP16 = (-1, 0, 0, 1, 1, 2, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)
# (T, starts, counts, parents per row)
CASES = (
    (4, (510, 62, 126, 0), (4, 4, 4, 4), (CHAIN4,) * 4),
    (4, (510, 0, 126, 62), (4, 0, 3, 2), (STAR4,) * 4),   # row 1: empty
    (6, (510, 62, 126, 0), (6, 3, 6, 5), (TWO6,) * 4),
    (4, (126, 0, 510, 62), (4, 4, 0, 3),
     ((-1, 0, 0, 2), (-1, -1, 0, 1), CHAIN4, (-1, 0, 1, 1))),
    (16, (510, 62, 126, 0), (16, 9, 0, 16), (DEEP16,) * 4),
)
CASE_NAMES = ("chain", "star", "two_branch", "per_row", "deep16")
FAMILY = ("own", "root", "sib", "seam")   # by h % G


def case_id(case) -> str:
    return CASE_NAMES[CASES.index(case)]


def ancestors(parents, i: int) -> list[int]:
    """anc(i), self first, root-most last."""
    out = []
    while i >= 0:
        out.append(i)
        i = parents[i]
    return out


def anc_bits(t: int, counts, parents) -> torch.Tensor:
    """(B, T) int64: bit j of [b, i] set iff node j is in anc(i); 0 at or
    past counts[b]. The masks at world size 1, where slot = node index."""
    return torch.tensor(
        [[sum(1 << j for j in ancestors(parents[b], i)) if i < c else 0
          for i in range(t)] for b, c in enumerate(counts)],
        dtype=torch.long)


def depth(parents) -> int:
    return max(len(ancestors(parents, i)) for i in range(len(parents)))


@dataclass
class Tree:
    t: int
    starts: tuple
    counts: tuple
    parents: tuple          # per row, T entries
    lengths: tuple          # starts + counts
    dtype: str
    kind: str
    cap: int
    base: torch.Tensor      # (B,) int64 = starts
    bits: torch.Tensor      # (B, T) int64 ancestor masks
    k: torch.Tensor         # (B, Hkv, cap, D) storage dtype: row b's tokens
    v: torch.Tensor         # are [:lengths[b]], its nodes [starts[b]:][:T]
    q: torch.Tensor         # (B, Hq, T, D) bf16
    k_cache: torch.Tensor   # k / v with the guard pattern at and past each
    v_cache: torch.Tensor   # row's final length
    ref_out: torch.Tensor   # fp32 oracle (B, Hq, T, D)
    ref_lse: torch.Tensor   # (B, Hq, T); -inf where no key is visible


def _own_key(t0: int, c: int, h: int, i: int) -> int:
    own = t0 + i if i < c else t0 - 1
    # nothing visible: point at stored data all the same
    return own if own >= 0 else h


def _query_key(t0: int, c: int, parents, b: int, h: int, i: int) -> int:
    """The key query (b, h, i) targets (see the module docstring)."""
    fam = FAMILY[h % G]
    own = _own_key(t0, c, h, i)
    if fam == "seam":
        below = [s for s in rc.SEAMS if s < t0]
        return below[(i + b + h // G) % len(below)] if below else own
    if fam == "root" and i < c:
        return t0 + ancestors(parents, i)[-1]
    if fam == "sib":
        if i >= c:
            return t0 + c - 1 if c else own
        anc = ancestors(parents, i)
        sibs = [j for j in range(i) if j not in anc]
        return t0 + sibs[-1] if sibs else own
    return own


def per_head(x: torch.Tensor) -> torch.Tensor:
    """(B, T) -> (B, Hq, T)."""
    return x[:, None, :].expand(B, HQ, x.shape[1])


def canon(base: int, bits: int, cap: int) -> tuple:
    """(n, extra): what (base, bits) shows inside [0, cap) as the prefix [0,
    n) plus the positions `extra` past it; equal for masks that show the
    same keys."""
    n = max(0, min(base, cap))
    extra = [base + s for s in range(SLOTS)
             if (bits >> s) & 1 and n <= base + s < cap]
    while extra and extra[0] == n:
        n, extra = n + 1, extra[1:]
    return n, tuple(extra)


def visible(base: int, bits: int, cap: int) -> list[int]:
    """The key positions (base, bits) shows, inside [0, cap)."""
    n, extra = canon(base, bits, cap)
    return list(range(n)) + list(extra)


def attend_masks(q, k_cache, v_cache, base, bits, like=None):
    """Attention of every query (b, h, i) of q (B, Hq, T, D) over the keys
    visible(base[b, h, i], bits[b, h, i]) of k_cache / v_cache (B, Hkv, n,
    D): the true masks give the oracle, any other a mutant. like = (base,
    bits, out, lse) of an earlier call over the same q and cache: entries
    with the same mask are taken from it. -> (out, lse) fp32."""
    from tree_attention_torch_amd.ops.reference import flash_res_lse

    t, cap = q.shape[2], k_cache.shape[2]
    out = torch.zeros(B, HQ, t, D)
    lse = torch.full((B, HQ, t), float("-inf"))
    kf, vf = k_cache.float(), v_cache.float()
    for b in range(B):
        for h in range(HQ):
            for i in range(t):
                bs, bt = int(base[b, h, i]), int(bits[b, h, i])
                if like is not None and bs == int(like[0][b, h, i]) and \
                        bt == int(like[1][b, h, i]):
                    out[b, h, i], lse[b, h, i] = \
                        like[2][b, h, i], like[3][b, h, i]
                    continue
                idx = torch.tensor(visible(bs, bt, cap), dtype=torch.long)
                if idx.numel() == 0:
                    continue
                kv = h // G
                o, l = flash_res_lse(q[b:b + 1, h:h + 1, i:i + 1].float(),
                                     kf[b:b + 1, kv:kv + 1][:, :, idx],
                                     vf[b:b + 1, kv:kv + 1][:, :, idx])
                out[b, h, i], lse[b, h, i] = o[0, 0, 0], l[0, 0, 0]
    return out, lse


def true_masks(tr: "Tree"):
    """(base, bits) per head, (B, Hq, T) each."""
    return per_head(tr.base[:, None].expand(B, tr.t)), per_head(tr.bits)


@lru_cache(maxsize=None)
def build(case: tuple, dtype: str) -> Tree:
    return build_from(case, dtype, *rc.kv(dtype))


def build_from(case: tuple, dtype: str, k, v) -> Tree:
    """The inputs of one case over the streams k / v (B, Hkv, cap, D) in the
    storage dtype (build: the shared draw)."""
    t, starts, counts, parents = case
    assert all(len(p) == t and all(-1 <= p[j] < j for j in range(t))
               for p in parents)
    lengths = tuple(s + c for s, c in zip(starts, counts))
    qf = torch.empty(B, HQ, t, D)
    for b in range(B):
        for h in range(HQ):
            for i in range(t):
                key = _query_key(starts[b], counts[b], parents[b], b, h, i)
                own = _own_key(starts[b], counts[b], h, i)
                qf[b, h, i] = nc.needle_gain(D) * k[b, h // G, key].float()
                if FAMILY[h % G] == "sib" and key != own:
                    # anchored on the query's own, visible key
                    a = 4.0 * k[b, h // G, own].float() + \
                        6.0 * k[b, h // G, key].float()
                    if dtype == "fp8":
                        a = a.to(torch.float8_e4m3fn).float()
                    qf[b, h, i] = a.bfloat16().float()
    q = qf.to(torch.bfloat16).contiguous()
    assert torch.equal(q.float(), qf), "the query must be exact in bf16"
    k_cache, v_cache = rc.with_guards(k, v, q, lengths)
    tr = Tree(t, tuple(starts), tuple(counts), tuple(parents), lengths, dtype,
              rc.KIND[dtype], CAP, torch.tensor(starts, dtype=torch.long),
              anc_bits(t, counts, parents), k, v, q, k_cache, v_cache, None,
              None)
    tr.ref_out, tr.ref_lse = attend_masks(q, k_cache, v_cache,
                                          *true_masks(tr))
    return tr


def mutant_masks(tr: Tree) -> dict:
    """The mask errors the inputs must expose -> (base, bits), (B, Hq, T)
    each, at world size 1."""
    t, bits = tr.t, tr.bits
    base = tr.base[:, None].expand(B, t)

    def rows(fn):
        return torch.tensor([[fn(b, i) if i < c else 0 for i in range(t)]
                             for b, c in enumerate(tr.counts)],
                            dtype=torch.long)

    par = tr.parents
    other = [b ^ 1 for b in range(B)]
    # the mask taken by row / G in place of row % Tq, per launch of PER_CALL
    # query positions: row = g * n + (i - i0) of the group's n
    by_row = torch.empty(B, HQ, t, dtype=torch.long)
    no_offset = bits.clone()
    for i0 in range(0, t, PER_CALL):
        n = min(PER_CALL, t - i0)
        no_offset[:, i0:i0 + n] = bits[:, :n]
        for h in range(HQ):
            for i in range(i0, i0 + n):
                row = (h % G) * n + (i - i0)
                by_row[:, h, i] = bits[:, i0 + row // G]
    return {
        "chain": (per_head(base), per_head(rows(lambda b, i: (2 << i) - 1))),
        "self_only": (per_head(base), per_head(rows(lambda b, i: 1 << i))),
        "self+parent": (per_head(base), per_head(rows(
            lambda b, i: (1 << i) | (1 << par[b][i] if par[b][i] >= 0
                                     else 0)))),
        "no_self": (per_head(base), per_head(rows(
            lambda b, i: int(bits[b, i]) & ~(1 << i)))),
        "row_b^1": (per_head(base), per_head(anc_bits(
            t, [tr.counts[o] for o in other], [par[o] for o in other]))),
        "row/G": (per_head(base), by_row),
        "no_group_offset": (per_head(base), per_head(no_offset)),
        "base+1": (per_head(base + 1), per_head(bits)),
        "base-1": (per_head(base - 1), per_head(bits)),
    }


# ---- a shard of a block-cyclic sharded sequence, on the host ----
def shard_positions(rank: int, world: int, block: int, cap: int = CAP):
    """The global positions below cap that `rank` owns, in local order."""
    return [p for p in range(cap) if (p // block) % world == rank]


def shard_masks(tr: Tree, rank: int, world: int, block: int):
    """(base (B,), bits (B, T)) of `rank`'s shard as kv_append_tree_kernel
    leaves them: base = this rank's tokens below starts[b]; bit s set for the
    owned ancestors, s their local slot counted from base."""
    own = set(shard_positions(rank, world, block))
    base, bits = [], []
    for b, (t0, c) in enumerate(zip(tr.starts, tr.counts)):
        base.append(sum(1 for p in range(t0) if p in own))
        row = []
        for i in range(tr.t):
            m = 0
            for j in (ancestors(tr.parents[b], i) if i < c else []):
                if t0 + j in own:
                    m |= 1 << sum(1 for x in range(j) if t0 + x in own)
            row.append(m)
        bits.append(row)
    return (torch.tensor(base, dtype=torch.long),
            torch.tensor(bits, dtype=torch.long))


def global_slot_masks(tr: Tree, rank: int, world: int, block: int):
    """The mutant of a sharded rank: the true local base, but the GLOBAL node
    index used as the local slot."""
    base, _ = shard_masks(tr, rank, world, block)
    own = set(shard_positions(rank, world, block))
    bits = [[sum(1 << j for j in ancestors(tr.parents[b], i)
                 if t0 + j in own) if i < c else 0 for i in range(tr.t)]
            for b, (t0, c) in enumerate(zip(tr.starts, tr.counts))]
    return base, torch.tensor(bits, dtype=torch.long)


def compare_to(tr: Tree, out, lse, ref_out, ref_lse, what: str = "") -> None:
    """needle_cases.compare at the kind's bars; a query that sees no key
    must be out = 0, lse = -inf (equal infinities compare close)."""
    try:
        nc.compare(out, lse, ref_out, ref_lse, tr.kind)
    except AssertionError as e:
        raise AssertionError(
            f"tree {tr.dtype} T={tr.t} starts {tr.starts} counts "
            f"{tr.counts} {what}\n{e}") from None


def compare(tr: Tree, out, lse, what: str = "") -> None:
    compare_to(tr, out, lse, tr.ref_out, tr.ref_lse, what)


def rejected(tr: Tree, out, lse, ref=None) -> bool:
    try:
        compare_to(tr, out, lse, *(ref or (tr.ref_out, tr.ref_lse)))
    except AssertionError:
        return True
    return False


def stream(tr: Tree):
    """What a session is fed, as bf16 tensors whose cast to the cache dtype
    gives back tr.k / tr.v bit for bit: (k, v) (B, Hkv, cap, D), whose
    [b, :, :starts[b]] is row b's prompt, and the nodes (B, Hkv, T, D)."""
    ks, vs = tr.k.float().bfloat16(), tr.v.float().bfloat16()
    kd = torch.stack([ks[b, :, s:s + tr.t] for b, s in enumerate(tr.starts)])
    vd = torch.stack([vs[b, :, s:s + tr.t] for b, s in enumerate(tr.starts)])
    return ks, vs, kd, vd


def committed(tr: Tree, paths, lens):
    """The streams after commit(paths, lens) on top of tr: row b's tokens
    starts[b] + i are its nodes paths[b][i], i < lens[b]; everything else is
    tr's. -> (k, v, new starts)."""
    k, v = tr.k.clone(), tr.v.clone()
    for b, (t0, n) in enumerate(zip(tr.starts, lens)):
        for i in range(n):
            assert paths[b][i] < tr.counts[b] and \
                tr.parents[b][paths[b][i]] == (paths[b][i - 1] if i else -1)
            k[b, :, t0 + i] = tr.k[b, :, t0 + paths[b][i]]
            v[b, :, t0 + i] = tr.v[b, :, t0 + paths[b][i]]
    return k, v, tuple(t0 + n for t0, n in zip(tr.starts, lens))


def parents_tensor(tr: Tree, device="cpu") -> torch.Tensor:
    return torch.tensor(tr.parents, dtype=torch.int32).to(device)
