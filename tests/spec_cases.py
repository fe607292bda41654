"""Speculative-verify needle inputs: T draft tokens per batch row, one
visible length per (row, query position).

The construction of tests/ragged_cases.py (docs/NEEDLE_TESTS.md): B = 4,
Hq = 8, Hkv = 2, D = 128 over a cache of capacity 1024 (two 512-key splits,
64- and 128-key tiles), the same K/V draw, gain and guard pattern. Sequence b
holds starts[b] tokens, takes counts[b] of T drafts and ends at lengths[b] =
starts[b] + counts[b]; query i of row b sees the local prefix of length

    vis[b, i] = starts[b] + min(i, counts[b] - 1) + 1   (counts[b] = 0:
                                                         starts[b])

(world size 1; n_local of a sharded session reduces to this). Every cache row
at or past lengths[b] holds a decoy K and a NaN V, so any limit that is too
long at the last draft poisons the output.

Starts put the drafts across the seams that matter: 510 (drafts straddle the
split seam 511 | 512), 62 (the 64-key tile seam), 126 (the 128-key tile and
page seam), 0 (the drafts are the whole sequence), and rows with count 0 (one
of them empty: out = 0, lse = -inf). T = 3 gives m_rows = 12, where
row % Tq is not row / G; T = 4 the full 16 MFMA rows; T = 6 two launches (4
query positions, then 2).

Query families, by the head's place g = h % G in its KV group:
  own  (g = 0, 3): gain * K of the query's own draft, the LAST visible key
                   (count 0: the last key of the prefix). A limit one short
                   loses it.
  next (g = 1):    gain * K of the next position, the FIRST masked key: draft
                   i + 1, or the guard row at the final length. A limit one
                   long reads it.
  seam (g = 2):    gain * K of a prefix key on a tile, page or split seam
                   (no prefix: own).

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
CHUNK = rc.CHUNK
DTYPES = rc.DTYPES
PER_CALL = 16 // G     # query positions one launch carries
# (T, starts, counts)
CASES = (
    (3, (510, 62, 126, 0), (3, 3, 3, 3)),
    (3, (510, 0, 126, 62), (3, 0, 1, 2)),    # row 1: empty and count 0
    (4, (510, 62, 126, 0), (4, 2, 0, 3)),
    (4, (126, 0, 510, 62), (4, 4, 4, 4)),
    (6, (510, 62, 126, 0), (6, 3, 6, 5)),
)
FAMILY = ("own", "next", "seam", "own")   # by h % G


def case_id(case) -> str:
    t, starts, counts = case
    return f"T{t}-{'_'.join(map(str, starts))}-{''.join(map(str, counts))}"


def vis_of(t: int, starts, counts) -> torch.Tensor:
    """(B, T) visible lengths at world size 1."""
    return torch.tensor(
        [[s + (min(i, c - 1) + 1 if c else 0) for i in range(t)]
         for s, c in zip(starts, counts)], dtype=torch.long)


@dataclass
class Spec:
    t: int
    starts: tuple
    counts: tuple
    lengths: tuple          # starts + counts
    dtype: str
    kind: str
    cap: int
    vis: torch.Tensor       # (B, T) int64
    k: torch.Tensor         # (B, Hkv, cap, D) storage dtype: row b's tokens
    v: torch.Tensor         # are [:lengths[b]], its drafts [starts[b]:][:T]
    q: torch.Tensor         # (B, Hq, T, D) bf16
    k_cache: torch.Tensor   # k / v with the guard pattern at and past each
    v_cache: torch.Tensor   # row's final length
    ref_out: torch.Tensor   # fp32 oracle (B, Hq, T, D)
    ref_lse: torch.Tensor   # (B, Hq, T); -inf where no key is visible


def _query_key(t0: int, c: int, b: int, h: int, i: int) -> int:
    """The key query (b, h, i) is gain times (see the module docstring)."""
    last = t0 + (min(i, c - 1) if c else -1)    # the last visible key
    fam = FAMILY[h % G]
    if fam == "seam":
        below = [s for s in rc.SEAMS if s < t0]
        if below:
            return below[(i + b + h // G) % len(below)]
        fam = "own"
    if fam == "next":
        return last + 1
    # nothing visible: point at stored data all the same (ragged_cases)
    return last if last >= 0 else h


def attend_limits(sp: "Spec", lim: torch.Tensor):
    """Attention of every query over the GUARDED cache with query (b, h, i)
    cut at lim[b, h, i] (clipped to [0, capacity]): the true limits give the
    oracle, any other limits a mutant. -> (out, lse) fp32."""
    from tree_attention_torch_amd.ops.reference import flash_res_lse

    out = torch.zeros(B, HQ, sp.t, D)
    lse = torch.full((B, HQ, sp.t), float("-inf"))
    kf, vf = sp.k_cache.float(), sp.v_cache.float()
    for b in range(B):
        for h in range(HQ):
            for i in range(sp.t):
                n = max(0, min(int(lim[b, h, i]), sp.cap))
                if n == 0:
                    continue
                kv = h // G
                o, l = flash_res_lse(sp.q[b:b + 1, h:h + 1, i:i + 1].float(),
                                     kf[b:b + 1, kv:kv + 1, :n],
                                     vf[b:b + 1, kv:kv + 1, :n])
                out[b, h, i], lse[b, h, i] = o[0, 0, 0], l[0, 0, 0]
    return out, lse


def per_head(vis: torch.Tensor) -> torch.Tensor:
    """(B, T) limits -> (B, Hq, T)."""
    return vis[:, None, :].expand(B, HQ, vis.shape[1])


@lru_cache(maxsize=None)
def build(case: tuple, dtype: str) -> Spec:
    t, starts, counts = case
    lengths = tuple(s + c for s, c in zip(starts, counts))
    k, v = rc.kv(dtype)
    qf = torch.empty(B, HQ, t, D)
    for b in range(B):
        for h in range(HQ):
            for i in range(t):
                key = _query_key(starts[b], counts[b], b, h, i)
                qf[b, h, i] = nc.needle_gain(D) * k[b, h // G, key].float()
    q = qf.to(torch.bfloat16).contiguous()
    assert torch.equal(q.float(), qf), "gain*K must be exact in bf16"
    k_cache, v_cache = rc.with_guards(k, v, q, lengths)
    sp = Spec(t, tuple(starts), tuple(counts), lengths, dtype, rc.KIND[dtype],
              CAP, vis_of(t, starts, counts), k, v, q, k_cache, v_cache, None,
              None)
    sp.ref_out, sp.ref_lse = attend_limits(sp, per_head(sp.vis))
    return sp


def mutant_limits(sp: Spec) -> dict:
    """The limit errors the inputs must expose -> (B, Hq, T) limits."""
    vis, t = sp.vis, sp.t
    # the limit taken by row / G in place of row % Tq, per launch of
    # PER_CALL query positions: row = g * n + (i - i0) of the group's n
    by_row = torch.empty(B, HQ, t, dtype=torch.long)
    for i0 in range(0, t, PER_CALL):
        n = min(PER_CALL, t - i0)
        for h in range(HQ):
            for i in range(i0, i0 + n):
                row = (h % G) * n + (i - i0)
                by_row[:, h, i] = vis[:, i0 + row // G]
    return {
        "vis+1": per_head(vis + 1),
        "vis-1": per_head(vis - 1),
        "no_causal": per_head(vis[:, -1:].expand(B, t)),
        "row/G": by_row,
        "row_b^1": per_head(vis[[b ^ 1 for b in range(B)]]),
        "chunk_down": per_head(vis // CHUNK * CHUNK),
        "chunk_up": per_head(-(-vis // CHUNK) * CHUNK),
    }


def compare(sp: Spec, out, lse, what: str = "") -> None:
    """needle_cases.compare at the kind's bars; a query that sees no key
    must be out = 0, lse = -inf (equal infinities compare close)."""
    try:
        nc.compare(out, lse, sp.ref_out, sp.ref_lse, sp.kind)
    except AssertionError as e:
        raise AssertionError(
            f"spec {sp.dtype} T={sp.t} starts {sp.starts} counts "
            f"{sp.counts} {what}\n{e}") from None


def rejected(sp: Spec, out, lse) -> bool:
    try:
        compare(sp, out, lse)
    except AssertionError:
        return True
    return False


def stream(sp: Spec):
    """What a session is fed, as bf16 tensors whose cast to the cache dtype
    gives back sp.k / sp.v bit for bit: (k, v) (B, Hkv, cap, D), whose
    [b, :, :starts[b]] is row b's prompt, and the drafts (B, Hkv, T, D)."""
    ks, vs = sp.k.float().bfloat16(), sp.v.float().bfloat16()
    kd = torch.stack([ks[b, :, s:s + sp.t] for b, s in enumerate(sp.starts)])
    vd = torch.stack([vs[b, :, s:s + sp.t] for b, s in enumerate(sp.starts)])
    return ks, vs, kd, vd
