"""Needle inputs: attention problems whose answer names the key that was read.

On ``randn`` Q/K/V the softmax is close to uniform over hundreds of keys, so
one key more or less, or two V rows exchanged, moves ``out`` and ``lse`` by
less than the suite's bars (docs/NEEDLE_TESTS.md has the table). Here every
query row is ``2 * K[target]``: with D=128 and scale 1/sqrt(D) the target
scores ~22.6, every other key ~N(0, 2), so ``out ~= V[target]`` (|.| up to ~4)
and ``lse ~= 22.6``. Reading the wrong key, or not reading the right one,
moves the answer by O(1). Rows with B > 1 hold different K/V (and targets)
in every batch; rows with a softmax scale of their own pick the gain from the
scale (needle_gain), and a kernel that ignores the scale shows in ``lse``.

The many-split rows (more than two splits of the split-KV decode kernels)
put a needle in every split and on both sides of every split seam; their
``pair`` family is ``gain * (K[t1] + K[t2])`` with the two targets in
different splits at weights between 0.67 / 0.33 and 0.82 / 0.18, so that the
combine has to weigh two live splits right.

This module is a plain helper (not a conftest). It holds

* the needle builders and the shared CASE TABLE,
* ``split_plan``, the binding's split heuristic for any length,
* an fp64 naive attention that can be MUTATED (the errors the suite must see),
* an fp64 SPLIT oracle (partials by ``split_plan``, merged by the stable
  algebra) and the split / combine mutants of it,
* ``guarded``: K/V views with decoy-K / NaN-V rows on both sides,
* ``compare``: the project's existing bars, used by BOTH the CPU sensitivity
  tests (tests/test_needle_sensitivity.py) and the GPU tests
  (tests/test_gpu_needles.py), so what is proven on the CPU is what runs on
  the GPU,
* the GPU runners (shared with the env-variant child processes).
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache

import torch

SEED = 20260920
CACHE_CAP = 1024
# seed offset per extra batch. Needles are a statistical construction: with
# B*Hq*Tq rows against hundreds of keys, some draws of K leave a row of a
# D = 32 or D = 64 case (lead ~9 / ~19 nats on average) short of one-hot, or
# a diffuse first_masked row of an e4m3-P kind too near its bar. With this
# offset every batched row meets the one-hot condition at <= 0.31 of its
# tolerance and the emulated kernels stay at <= 0.65 of their bars
# (tests/test_needle_sensitivity.py asserts both conditions).
BATCH_SALT = 37
GUARD_PRE, GUARD_POST = 2, 130  # > one 128-key tile of rows behind the view

_TD = {"bf16": torch.bfloat16, "fp16": torch.float16,
       "fp8": torch.float8_e4m3fn}

# (out bar, lse bar), rtol = atol, exactly the bars the suite already uses:
# half  - tests/test_gpu_kernels.py::_check_decode / _check_fp16
# fp8   - _check_fp8_decode (measured worst 0.0155 / 0.0213, x2.5)
# mx_*  - test_mx_decode_vs_oracle (tame-data branches, hw and dequant)
BARS = {
    "half": (2.5e-2, 1e-3),
    "fp8": (4e-2, 5e-2),
    "mx_hw": (4e-2, 3e-2),
    "mx_dequant": (2e-2, 1e-2),
}

PREFILL_ROUTES = ("prefill", "prefill_d64", "prefill_fp8", "prefill_mx")
CAUSAL_FAMILIES = ("diag", "first_masked", "below")


# --------------------------------------------------------------------------
# case table
# --------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    route: str      # which entry point / kernel (see run_kernel)
    dtype: str      # bf16 | fp16 | fp8 | mx
    hq: int
    hkv: int
    tkv: int
    tq: int
    families: tuple
    seams: tuple = ()      # key indices s where a tile/sub-block/split begins
    d: int = 128
    q_offset: int = -1     # -1: tkv - tq - 3 (three hidden keys at the end)
    guard: bool = False    # GPU also runs it on guarded K/V (B=1, Hkv=1)
    cuts: tuple = ()       # sharded routes: shard boundaries
    note: str = ""
    b: int = 1             # batch; every batch holds different K/V
    scale: float = 0.0     # softmax scale; 0: 1/sqrt(d)
    cap: int = 0           # cache rows: capacity; 0: CACHE_CAP
    tile: int = 0          # many-split rows: keys per tile of the kernel

    @property
    def softmax_scale(self) -> float:
        return self.scale if self.scale else 1.0 / math.sqrt(self.d)

    @property
    def qoff(self) -> int:
        return max(self.tkv - self.tq - 3, 0) if self.q_offset < 0 \
            else self.q_offset

    @property
    def kind(self) -> str:
        if self.route == "mx_dequant":
            return "mx_dequant"
        if self.dtype == "mx":
            return "mx_hw"
        return "fp8" if self.dtype == "fp8" else "half"

    @property
    def id(self) -> str:
        s = (f"{self.route}-{self.dtype}-h{self.hq}kv{self.hkv}-t{self.tkv}"
             f"q{self.tq}")
        if self.d != 128:
            s += f"-d{self.d}"
        if self.q_offset >= 0:
            s += f"-qo{self.q_offset}"
        if self.seams:
            sm = ".".join(map(str, self.seams[:4]))
            s += f"-seams{sm}" + ("+" if len(self.seams) > 4 else "")
        if self.b != 1:
            s += f"-b{self.b}"
        if self.scale:
            s += f"-s{self.scale:g}"
        if self.cap:
            s += f"-cap{self.cap}"
        return s

    @property
    def capacity(self) -> int:
        return self.cap or CACHE_CAP

    @property
    def plan(self):
        """(S, chunk) of the split-KV call this row makes (the cache kernel
        plans over its capacity, a spec row per query chunk); None for the
        routes that make no single split-KV call."""
        if self.route == "cache":
            return split_plan(self.b, self.hkv, self.capacity)
        if self.route.startswith("decode") or self.route in (
                "mx_hw", "mx_dequant", "spec"):
            return split_plan(self.b, self.hkv, self.tkv)
        return None

    @property
    def live_splits(self) -> int:
        """Splits that hold at least one live key."""
        return -(-self.tkv // self.plan[1])

    @property
    def combine_groups(self) -> int:
        """NG of fa_combine_kernel: 512 / partial width (narrow heads are
        padded to 128)."""
        return 8 if self.d == 64 else 4


SPLIT_TARGET = 512   # the binding's grid target with the env knob unset


def split_plan(b: int, hkv: int, tkv: int) -> tuple:
    """(S, chunk) of the split-KV decode kernels over tkv keys: pick_splits
    and plan_splits of ops/hip/bindings.cpp in full, for any length, with
    TREE_ATTN_SPLIT_BLOCKS unset (the GPU tests assert that). Chunks are no
    shorter than clamp(tkv / 64, 512, 2048) keys; the grid target is 512
    blocks when B*Hkv divides it and 768 otherwise; the chunk is rounded up
    to 128 keys and S recomputed from it (40000 keys: 64 -> 63 splits of
    640). Used to NAME the split seams a case targets and to cut the split
    oracle; pinned by a table in tests/test_needle_sensitivity.py."""
    min_chunk = min(max(tkv // 64, 512), 2048)
    max_s = -(-tkv // min_chunk)
    bh = b * hkv
    if bh <= SPLIT_TARGET and SPLIT_TARGET % bh == 0:
        s = SPLIT_TARGET // bh
    else:
        s = (SPLIT_TARGET * 3 // 2 + bh - 1) // bh
    s = max(1, min(s, max_s))
    chunk = (-(-tkv // s) + 127) // 128 * 128
    return -(-tkv // chunk), chunk


def assert_default_split_plan() -> None:
    """split_plan mirrors the binding only while its grid target is the
    default; a GPU test that relies on the seams says so loudly."""
    import os

    assert "TREE_ATTN_SPLIT_BLOCKS" not in os.environ, \
        "TREE_ATTN_SPLIT_BLOCKS is set: needle_cases.split_plan (and every " \
        "split seam the case table names) mirrors the default grid target"


def pick_seams(tkv: int, tile: int, rows: int, chunk: int = 0,
               sub: int = 0) -> tuple:
    """Seams of a kernel over tkv keys, most important first (split seams,
    then tile seams from both ends inwards, then sub-block seams), cut so
    that {0, tkv-1} plus both sides of every seam fit into `rows` targets."""
    out: list[int] = []

    def add(xs):
        for x in xs:
            if 0 < x < tkv and x not in out:
                out.append(x)

    if chunk:
        add(range(chunk, tkv, chunk))
    tiles = list(range(tile, tkv, tile))
    inter = []
    while tiles:
        inter.append(tiles.pop())       # last seam first: the tail tile
        if tiles:
            inter.append(tiles.pop(0))
    add(inter)
    if sub:
        add(range(sub, tkv, sub))
    return tuple(out[: max((rows - 2) // 2, 0)])


def seam_targets(case: Case) -> list[int]:
    t = case.tkv
    cand = [0, t - 1]
    for s in case.seams:
        cand += [s - 1, s]
    seen, out = set(), []
    for c in cand:
        if 0 <= c < t and c not in seen:
            seen.add(c)
            out.append(c)
    assert len(out) <= case.b * case.hq * case.tq, \
        f"{case.id}: {len(out)} seam targets do not fit the query rows"
    return out


def _decode_family(tkv: int, tq: int) -> tuple:
    if tkv - tq < 1:   # no hidden key can exist: first_masked impossible
        return ("seam", "diag")
    return ("seam", "diag", "first_masked")


def _build_table() -> list[Case]:
    cases: list[Case] = []

    def add(route, dtype, hq, hkv, tkv, tq, tile, *, d=128, sub=0, guard=False,
            chunk=True, families=None, q_offset=-1, cuts=(), note="", b=1,
            scale=0.0, many=False, seams=None):
        # a many-split row sizes its seam set by ALL its rows (B*Hq*Tq: the
        # rotation of family_targets runs on over the batches) and adds the
        # `pair` family; every other row keeps the seams it always had
        ch = split_plan(b, hkv, tkv)[1] if chunk else 0
        rows = (b if many else 1) * hq * tq
        if seams is None:
            seams = pick_seams(tkv, tile, rows, ch, sub)
        if cuts:
            seams = tuple(dict.fromkeys(tuple(cuts[1:-1]) + seams))[
                : (rows - 2) // 2]
        fam = families or _decode_family(tkv, tq)
        if many and route != "spec" and not cuts:
            fam = fam + ("pair",)
        cases.append(Case(route, dtype, hq, hkv, tkv, tq, fam, seams, d,
                          q_offset, guard and hkv == 1 and b == 1,
                          tuple(cuts), note, b, scale, 0,
                          tile if many else 0))

    # -- bf16/fp16 split-KV decode (fa_fwd_kernel): 64-key tiles, chunk a
    #    multiple of 128, second split above 512 keys (513 -> 384 + 129)
    for tkv in (1, 63, 64, 65, 513, 1000):
        add("decode", "bf16", 32, 32, tkv, 1, 64)               # G=1
        add("decode", "bf16", 16, 1, tkv, 1, 64, guard=True)    # G=16, Tq=1
        add("decode", "bf16", 8, 2, tkv, min(4, tkv), 64)       # G=4, Tq=4
        add("decode", "bf16", 4, 1, tkv, min(4, tkv), 64, guard=True)
    # G=2, Tq=8 causal, frontier ACROSS the split seam (384) of Tkv=513:
    # rows 380..383 leave the second split all-masked (lse_part = -inf)
    add("decode", "bf16", 2, 1, 513, 8, 64, guard=True, q_offset=380,
        note="frontier across split seam")
    add("decode", "fp16", 8, 2, 513, 4, 64)
    add("decode", "fp16", 16, 1, 1000, 1, 64, guard=True)
    add("decode", "fp16", 2, 1, 513, 8, 64, guard=True, q_offset=380)

    # -- other decode kernels: the same seam set on their 128-key tile
    for tkv in (1, 127, 128, 129, 513, 1000):
        add("decode_fp8", "fp8", 8, 2, tkv, min(4, tkv), 128)
        add("decode_fp8", "fp8", 16, 1, tkv, 1, 128, guard=True)
        add("decode_d64", "bf16", 8, 2, tkv, min(4, tkv), 128, d=64)
        for d in (32, 112):
            add("decode_narrow", "bf16", 8, 2, tkv, min(4, tkv), 128, d=d)
    add("decode_fp8", "fp8", 2, 1, 513, 8, 128, guard=True, q_offset=380)
    add("decode_d64", "fp16", 16, 1, 513, 1, 128, d=64, guard=True)
    for route in ("mx_hw", "mx_dequant"):
        for tkv in (64, 576):
            add(route, "mx", 8, 2, tkv, 4, 64)
            add(route, "mx", 16, 1, tkv, 1, 64)
        add(route, "mx", 2, 1, 576, 8, 64, q_offset=380)
        # causal frontier 17..32 and 81..96 keys into a 128-key tile: the
        # tail already reads block 1 of a V-scale window (interleaved 16s)
        add(route, "mx", 16, 1, 576, 1, 64, q_offset=535)   # tile 512: 24
        add(route, "mx", 8, 2, 576, 4, 64, q_offset=210)    # tile 128: 86

    # -- looped spec-decode route through local_attention
    add("spec", "bf16", 4, 4, 600, 17, 64)
    add("spec", "bf16", 8, 4, 600, 24, 64)

    # -- zero-copy cache kernel: cap 1024 (two 512-key splits), live length
    #    from device memory, guard pattern behind the live prefix
    for dt, tile in (("bf16", 64), ("fp8", 128)):
        for live in (1, 64, 65, 511, 512, 513, 1023, 1024):
            seams = pick_seams(live, tile, 32, 512)
            cases.append(Case("cache", dt, 8, 2, live, min(4, live),
                              ("seam",), seams))

    # -- prefill: 256-row q-blocks, 32-row waves, 128-key tiles, 32/64-key
    #    sub-blocks. ext.flash_attention is called directly: local_attention
    #    would loop the decode kernel at these sizes.
    pf = ("diag", "first_masked", "seam", "below")
    shapes = ((33, 36, -1), (257, 260, -1), (256, 384, 61), (300, 303, -1))
    for tq, tkv, qo in shapes:
        add("prefill", "bf16", 2, 2, tkv, tq, 128, sub=32, chunk=False,
            families=pf, q_offset=qo)
        add("prefill", "bf16", 4, 1, tkv, tq, 128, sub=32, chunk=False,
            families=pf, q_offset=qo, guard=True)          # GQA 4:1
        add("prefill", "fp16", 4, 1, tkv, tq, 128, sub=32, chunk=False,
            families=pf, q_offset=qo, guard=True)
        add("prefill_d64", "bf16", 4, 1, tkv, tq, 128, sub=32, chunk=False,
            families=pf, q_offset=qo, guard=True, d=64)
        add("prefill_fp8", "fp8", 4, 1, tkv, tq, 128, sub=32, chunk=False,
            families=pf, q_offset=qo, guard=True)
    for tq, tkv, qo in ((33, 64, -1), (257, 320, -1), (256, 384, 61),
                        (300, 320, -1)):
        add("prefill_mx", "mx", 4, 1, tkv, tq, 128, sub=32, chunk=False,
            families=pf, q_offset=qo)
    # (300, 320) leaves a 17-key tail under the first q-block's frontier;
    # this one an 84-key tail (V-scale window 1, block 1, without 96 keys)
    add("prefill_mx", "mx", 4, 1, 256, 100, 128, sub=32, chunk=False,
        families=pf, q_offset=112)

    # -- ranks emulated on one GPU: uneven cuts that are no tile multiples
    cuts = (0, 65, 193, 300)
    sf = ("seam", "diag", "first_masked")
    add("sharded", "bf16", 8, 8, 300, 1, 64, cuts=cuts, families=sf,
        q_offset=192, chunk=False)
    add("sharded", "bf16", 8, 2, 300, 4, 64, cuts=cuts, families=sf,
        q_offset=190, chunk=False)
    add("sharded", "bf16", 8, 4, 300, 300, 128, cuts=cuts, families=sf,
        q_offset=0, chunk=False, sub=32)
    mcuts = (0, 64, 192, 320)
    add("sharded_mx", "mx", 8, 8, 320, 1, 64, cuts=mcuts, families=sf,
        q_offset=191, chunk=False)
    add("sharded_mx", "mx", 8, 2, 320, 4, 64, cuts=mcuts, families=sf,
        q_offset=189, chunk=False)
    add("sharded_mx", "mx", 8, 4, 320, 300, 128, cuts=mcuts, families=sf,
        q_offset=0, chunk=False, sub=32)

    # ---------------------------------------------------------------------
    # batch > 1 (default scale, the route's full family set). Every batch
    # holds different K/V and different seam targets, so a wrong batch index
    # in a KV base, a partial offset or an output offset moves the answer by
    # O(1). 513 and 576 keys give two splits: partial offset s*B*Hq*Tq.
    # ---------------------------------------------------------------------
    for tkv in (129, 513):
        add("decode", "bf16", 8, 2, tkv, 4, 64, b=2)
        add("decode", "fp16", 8, 2, tkv, 4, 64, b=2)
        add("decode_fp8", "fp8", 8, 2, tkv, 4, 128, b=2)
        add("decode_d64", "bf16", 8, 2, tkv, 4, 128, d=64, b=2)
        for d in (32, 112):
            add("decode_narrow", "bf16", 8, 2, tkv, 4, 128, d=d, b=2)
    for route in ("mx_hw", "mx_dequant"):
        add(route, "mx", 8, 2, 576, 4, 64, b=2)
    # B*Hkv = 9 does not divide 512: the split heuristic's other branch
    add("decode", "bf16", 3, 3, 513, 4, 64, b=3)
    add("spec", "bf16", 4, 4, 600, 17, 64, b=2)
    for dt, tile in (("bf16", 64), ("fp8", 128)):
        for live in (513, 1024):
            cases.append(Case("cache", dt, 8, 2, live, 4, ("seam",),
                              pick_seams(live, tile, 32, 512), b=2))

    # prefill: (B, Hq, Hkv). gen7/gen9 take the XCD remap when B*Hq % 8 == 0:
    #   1, 8, 2   B*Hq = 8   remap, b = 0
    #   2, 4, 1   B*Hq = 8   remap, one 8-group = both batches
    #   2, 12, 3  B*Hq = 24  remap, the middle 8-group straddles the batches
    #   3, 4, 2   B*Hq = 12  no remap, B > 1
    pf_kinds = (("prefill", "bf16", 128), ("prefill", "fp16", 128),
                ("prefill_d64", "bf16", 64), ("prefill_fp8", "fp8", 128),
                ("prefill_mx", "mx", 128))
    for route, dt, d in pf_kinds:
        for tq, tkv, qo in ((257, 260, -1), (256, 384, 61)):
            if dt == "mx" and tkv == 260:
                tkv = 320
            for b, hq, hkv in ((1, 8, 2), (2, 4, 1), (2, 12, 3), (3, 4, 2)):
                add(route, dt, hq, hkv, tkv, tq, 128, sub=32, chunk=False,
                    families=pf, q_offset=qo, d=d, b=b)
    add("sharded", "bf16", 8, 2, 300, 4, 64, cuts=cuts, families=sf,
        q_offset=190, chunk=False, b=2)
    add("sharded", "bf16", 8, 4, 300, 300, 128, cuts=cuts, families=sf,
        q_offset=0, chunk=False, sub=32, b=2)
    # B = 2 MX shard slices are strided views with stride(0) ==
    # stride(1) * Hkv: the zero-copy route of fa_decode_fp8_mx_kernel
    add("sharded_mx", "mx", 8, 2, 320, 4, 64, cuts=mcuts, families=sf,
        q_offset=189, chunk=False, b=2)
    add("sharded_mx", "mx", 8, 4, 320, 300, 128, cuts=mcuts, families=sf,
        q_offset=0, chunk=False, sub=32, b=2)

    # ---------------------------------------------------------------------
    # softmax scale != 1/sqrt(D) (B = 1), one row per kernel kind and scale.
    # No first_masked: its correct answer is diffuse, the scale shows in the
    # one-hot families' lse (~25.6 at 0.05, ~D at 1.0 against 22.6 / 32).
    # ---------------------------------------------------------------------
    sd, sp = ("seam", "diag"), ("seam", "diag", "below")
    for sc in (0.05, 1.0):
        add("decode", "bf16", 8, 2, 513, 4, 64, families=sd, scale=sc)
        add("decode", "fp16", 8, 2, 513, 4, 64, families=sd, scale=sc)
        add("decode_fp8", "fp8", 8, 2, 513, 4, 128, families=sd, scale=sc)
        add("decode_d64", "bf16", 8, 2, 513, 4, 128, d=64, families=sd,
            scale=sc)
        for d in (32, 112):
            add("decode_narrow", "bf16", 8, 2, 513, 4, 128, d=d, families=sd,
                scale=sc)
        for route in ("mx_hw", "mx_dequant"):
            add(route, "mx", 8, 2, 576, 4, 64, families=sd, scale=sc)
        for dt, tile in (("bf16", 64), ("fp8", 128)):
            cases.append(Case("cache", dt, 8, 2, 513, 4, ("seam",),
                              pick_seams(513, tile, 32, 512), scale=sc))
        add("spec", "bf16", 4, 4, 600, 17, 64, families=sd, scale=sc)
        for route, dt, d in pf_kinds:
            add(route, dt, 4, 1, 320 if dt == "mx" else 260, 257, 128,
                sub=32, chunk=False, families=sp, d=d, guard=dt != "mx",
                scale=sc)
    # both at once, on the shape whose 8-group straddles the batches
    for route, dt, d in pf_kinds:
        add(route, dt, 12, 3, 320 if dt == "mx" else 260, 257, 128, sub=32,
            chunk=False, families=sp, d=d, b=2, scale=0.05)

    # ---------------------------------------------------------------------
    # DecodeSession(2, 2, 128) at world size 1: the KV enters through the
    # session's own prefill/append; on the GPU the oracle's K/V is what the
    # session STORED (tests/test_gpu_needles.py). attend() has no mask. 576
    # tokens: the MX session holds nine quantized windows; 600: also a 24-
    # token bf16 staging tail, merged by the lse algebra (seam 576). The
    # bf16/fp8 caches have capacity 1024 = two 512-key splits; the MX prefix
    # view splits at 384.
    # ---------------------------------------------------------------------
    for dt, tile in (("bf16", 64), ("fp8", 128), ("mx", 64)):
        for tkv in (576, 600):
            if dt == "mx":
                seams = ((576,) if tkv > 576 else ()) + \
                    pick_seams(576, tile, 30, split_plan(2, 2, 576)[1])
            else:
                seams = pick_seams(tkv, tile, 32, 512)
            for sc in (0.0, 0.05):
                cases.append(Case("session", dt, 8, 2, tkv, 4, ("seam",),
                                  seams, b=2, scale=sc))
    # ---------------------------------------------------------------------
    # many splits (S > 2): needles in every split, both sides of every split
    # seam, and the `pair` family (two live splits weighted by the combine).
    # fa_combine_kernel reduces `for (s = g; s < S; s += NG)` with NG = 4 at
    # width 128 (narrow heads are padded to it) and 8 at D = 64: S = NG + 1
    # and 2 NG + 1 make that loop take a second and a third step. Each row
    # is the shortest length that reaches its (S, chunk); split seams come
    # first in pick_seams, tile seams fill what rows are left.
    # ---------------------------------------------------------------------
    def frontier(route, dtype, tile, tkv, qo, note):
        # G = 2, Tq = 8 causal; B = 2 gives the 32 rows nine splits need
        add(route, dtype, 2, 1, tkv, 8, tile, q_offset=qo, b=2, many=True,
            note=note)

    def many_40000(route, dtype, tile):
        # 63 splits of 640 keys, 64 rows (at most 16 rows G*Tq fit per KV
        # head): both sides of the 31 odd seams plus keys 0 and 39999
        add(route, dtype, 32, 2, 40000, 1, tile, b=2, many=True,
            seams=tuple(range(640, 40000, 1280)),
            note="64 rows: every one of the 63 splits holds a target, both "
                 "sides of the 31 odd split seams are targets, the even "
                 "seams have no row left")

    add("decode", "bf16", 8, 2, 1100, 4, 64, many=True)    # S=3, chunk 384
    add("decode", "bf16", 8, 2, 2049, 4, 64, many=True)    # S=5, 1-key tail
    add("decode", "bf16", 8, 2, 2560, 4, 64, many=True)    # S=5, full
    add("decode", "bf16", 8, 2, 4097, 4, 64, many=True)    # S=9 = 2 NG + 1
    # (2554: at 2555..2559 the draw leaves one diag row 0.051 off its
    # target's V row, past the 0.05 the one-hot condition asks)
    frontier("decode", "bf16", 64, 4097, 2554,
             "frontier 2554..2561 inside split 5: splits 6..8 all-masked "
             "for every row, split 5 for rows 0..5")
    add("decode", "bf16", 3, 3, 2049, 4, 64, b=3, many=True)  # bh = 9
    add("decode", "fp16", 8, 2, 2049, 4, 64, many=True)
    many_40000("decode", "bf16", 64)
    add("decode_fp8", "fp8", 8, 2, 2049, 4, 128, many=True)
    add("decode_fp8", "fp8", 8, 2, 4097, 4, 128, many=True)
    frontier("decode_fp8", "fp8", 128, 4097, 2554, "as the bf16 row")
    many_40000("decode_fp8", "fp8", 128)
    add("decode_d64", "bf16", 8, 2, 4097, 4, 128, d=64, many=True)  # NG + 1
    add("decode_d64", "bf16", 8, 2, 8193, 4, 128, d=64, b=2, many=True,
        note="S = 17 = 2 NG + 1: 64 rows for 33 split targets")
    add("decode_d64", "fp16", 8, 2, 4097, 4, 128, d=64, many=True)
    for d in (80, 96, 112):
        for tkv in (2049, 4097):
            add("decode_narrow", "bf16", 8, 2, tkv, 4, 128, d=d, many=True)
    # every narrow instantiation has a needle row (D = 32 / 48 needles are
    # not sharp enough at thousands of keys: docs/NEEDLE_TESTS.md)
    for d in (48, 80, 96):
        for tkv in (129, 513):
            add("decode_narrow", "bf16", 8, 2, tkv, 4, 128, d=d, b=2)
    for route in ("mx_hw", "mx_dequant"):
        add(route, "mx", 8, 2, 2112, 4, 64, many=True)     # S=5, 64-key tail
        add(route, "mx", 8, 2, 4160, 4, 64, many=True)     # S=9, 64-key tail
        add(route, "mx", 2, 1, 2112, 8, 64, q_offset=1556, many=True,
            note="frontier 1556..1563: a 21..28-key tail inside split 3, "
                 "split 4 all-masked")
    add("spec", "bf16", 4, 4, 2100, 17, 64, many=True)     # S=5 per chunk
    # cache of capacity 4608 = nine 512-key splits: trailing splits are
    # EMPTY by the live length, at positions below and at or above NG
    for dt, tile in (("bf16", 64), ("fp8", 128)):
        for live in (1, 513, 2048, 2049, 4097, 4608):
            b = 2 if live in (2049, 4608) else 1
            tq = min(4, live)
            # 513 live keys leave a one-key second split: no choice of t2
            fam = ("seam", "pair") if live >= 2048 else ("seam",)
            cases.append(Case("cache", dt, 8, 2, live, tq, fam,
                              pick_seams(live, tile, b * 8 * tq, 512), b=b,
                              cap=4608, tile=tile))
    # two shards of five splits each, the second with kv_offset = 2049
    cuts2 = (0, 2049, 4150)
    add("sharded", "bf16", 8, 2, 4150, 4, 64, cuts=cuts2, families=sf,
        q_offset=3000, chunk=False, many=True,
        seams=(512, 1024, 1536, 2048) + tuple(range(2561, 4150, 512)),
        note="frontier 3000..3003 in the second shard; seams: the cut and "
             "each shard's own split seams")

    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), "duplicate case ids"
    return cases


CASES = _build_table()


# --------------------------------------------------------------------------
# needle builders
# --------------------------------------------------------------------------
@dataclass
class Needle:
    case: Case
    family: str
    causal: bool
    q_offset: int
    kv_offset: int
    scale: float
    targets: torch.Tensor      # (B, Hq, Tq) local key each row attends
    q: torch.Tensor            # storage dtype (bf16/fp16), CPU
    k: torch.Tensor | None     # storage dtype; None for MX
    v: torch.Tensor | None
    mx: tuple | None           # (k8, ks, v8, vs) for MX
    ref_q: torch.Tensor        # fp32 views the oracle sees
    ref_k: torch.Tensor
    ref_v: torch.Tensor
    targets2: torch.Tensor | None = None   # `pair`: the second target


def family_targets(case: Case, family: str) -> torch.Tensor:
    """(B, Hq, Tq) local key index every query row attends."""
    b, hq, tq, t = case.b, case.hq, case.tq, case.tkv
    pos = (case.qoff + torch.arange(tq))[None, None, :].expand(b, hq, tq)
    if family == "diag":
        tg = pos.clone()
    elif family == "first_masked":
        # a row whose first hidden key would lie past the KV keeps its diag
        tg = torch.where(pos + 1 < t, pos + 1, pos)
    elif family in ("seam", "below", "pair"):   # pair: the FIRST target
        cand = seam_targets(case)
        tg = torch.empty(b, hq, tq, dtype=torch.long)
        for i in range(b):
            for h in range(hq):
                for r in range(tq):
                    c = cand if family != "below" else \
                        [x for x in cand if x <= case.qoff + r]
                    # shift by one after every full cycle, so that the map
                    # is not symmetric under a (head, row) transposition;
                    # the batch continues the rotation, so batches differ
                    j = (i * hq + h) * tq + r
                    tg[i, h, r] = c[(j + j // len(c)) % len(c)]
    else:
        raise ValueError(family)
    assert int(tg.min()) >= 0 and int(tg.max()) < t, (case.id, family)
    return tg


def take_rows(x: torch.Tensor, case: Case, idx: torch.Tensor) -> torch.Tensor:
    """x (B, Hkv, T, D) at key idx (B, Hq, Tq) of each query head's KV head
    -> (B, Hq, Tq, D)."""
    kvh = torch.arange(case.hq) // (case.hq // case.hkv)
    bi = torch.arange(x.shape[0])
    return x[bi[:, None, None], kvh[None, :, None], idx]


def session_stored(k: torch.Tensor, v: torch.Tensor, dtype: str):
    """What DecodeSession keeps of a K/V stream, as fp32: bf16/fp8 rounding,
    or for MX the stream rounded to bf16, its closed 64-token windows
    quantized and the rest left in the bf16 staging tail."""
    from tree_attention_torch_amd.quant import (dequantize_k_mx,
                                                dequantize_v_mx,
                                                quantize_k_mx, quantize_v_mx)

    if dtype != "mx":
        return k.to(_TD[dtype]).float(), v.to(_TD[dtype]).float()
    kb, vb = k.bfloat16().float(), v.bfloat16().float()
    n = k.shape[2] // 64 * 64
    kq = dequantize_k_mx(*quantize_k_mx(kb[:, :, :n].contiguous()))
    vq = dequantize_v_mx(*quantize_v_mx(vb[:, :, :n].contiguous()))
    return torch.cat([kq, kb[:, :, n:]], 2), torch.cat([vq, vb[:, :, n:]], 2)


@lru_cache(maxsize=None)
def _kv(case: Case):
    """K/V for a case: randn rounded to the case's dtype, fixed seed, every
    batch different. Shared (and left unchanged) between the families and
    tests of one case. A session row keeps the bf16 stream the session is
    fed as k/v and what the session stores of it as the fp32 views."""
    from tree_attention_torch_amd.quant import (dequantize_k_mx,
                                                dequantize_v_mx,
                                                quantize_k_mx, quantize_v_mx)

    # the batch enters the seed too: rows that differ only in B (and so in
    # what their B*Hq decodes to) do not share their first batch
    g = torch.Generator().manual_seed(SEED + case.tkv * 7 + case.hkv
                                      + BATCH_SALT * (case.b - 1))
    k = torch.randn(case.b, case.hkv, case.tkv, case.d, generator=g)
    v = torch.randn(case.b, case.hkv, case.tkv, case.d, generator=g)
    if case.route == "session":
        k, v = k.bfloat16(), v.bfloat16()
        return (k, v, None) + session_stored(k, v, case.dtype)
    if case.dtype == "mx":
        k8, ks = quantize_k_mx(k)
        v8, vs = quantize_v_mx(v)
        return None, None, (k8, ks, v8, vs), \
            dequantize_k_mx(k8, ks), dequantize_v_mx(v8, vs)
    ks_, vs_ = k.to(_TD[case.dtype]), v.to(_TD[case.dtype])
    return ks_, vs_, None, ks_.float(), vs_.float()


def needle_gain(d: int, scale: float = 0.0) -> float:
    """q = gain * K[target]. The target scores gain*|k|^2/sqrt(D), any other
    key gain*|k|*N(0,1)/sqrt(D), so the target leads the largest of ~1000
    others (z ~ 3.3) by gain*(sqrt(D) - 3.3) nats: 16 at D=128 with gain 2.
    Narrow heads need gain 4 for the same lead (D=32: 9.4, D=64: 18.8). A
    power of two keeps the product exact in every dtype.

    With a softmax scale of its own (scale != 0) the gain is the power of
    two that brings the target's score gain*D*scale nearest 25.6, but never
    below 1: at scale 0.05 that is 4 (D=128, 112), 8 (D=64), 16 (D=32) and
    a score of 22.4..25.6; at scale 1.0 it is 1 and the score is D, against
    N(0, D) for any other key (lead D - 3.3 sqrt(D): 90 at D=128, 13 at 32).
    """
    if not scale:
        return 2.0 if d >= 112 else 4.0
    return max(1.0, 2.0 ** round(math.log2(25.6 / (d * scale))))


def build_from(case: Case, family: str, k, v, mx, kf, vf) -> Needle:
    """The needle of (case, family) over the given K/V: k/v/mx as a kernel
    is handed them, kf/vf the same values in fp32."""
    tg = family_targets(case, family)
    gain = needle_gain(case.d, case.scale)
    qf = gain * take_rows(kf, case, tg)          # (B, Hq, Tq, D)
    qdt = torch.float16 if case.dtype == "fp16" else torch.bfloat16
    q = qf.to(qdt)
    assert torch.equal(q.float(), qf), "gain*K must be exact in the query dtype"
    tg2 = None
    if family == "pair":
        tg2, q = pair_query(case, tg, kf, gain, qdt)
    if family == "first_masked" and case.kind in ("fp8", "mx_hw"):
        # ANCHORED first-masked for the kernels that quantize P to e4m3: a
        # query on a hidden key alone leaves a diffuse softmax over the
        # visible keys, and e4m3's 2^-4 relative step on a p ~ 0.5 is
        # 0.06 * |v| ~ 0.1 of output error - past the 4e-2 bar by the
        # format's own precision. Adding the diagonal key keeps the correct
        # answer one-hot (p = 1 is exact in e4m3): q = 4 K[pos] + 6 K[pos+1].
        # The diagonal scores ~45 against N(0, 7.2^2) others; the hidden key
        # would score ~68, so a mask that admits it hands it the row (dO =
        # |V[pos] - V[pos+1]|, dLSE ~ 22). The sum rounds to the query
        # dtype; the oracle reads the rounded query. Both properties are
        # proven per row of the table in tests/test_needle_sensitivity.py.
        assert not case.scale
        pos = (case.qoff + torch.arange(case.tq))[None, None, :].expand_as(tg)
        hidden = (tg != pos)[:, :, :, None]
        anchored = 3.0 * qf + 4.0 * take_rows(kf, case, pos)
        if case.kind == "fp8":
            # both fp8 kernels cast Q to e4m3. gain * K is exact there (K is
            # e4m3), this sum is not: the cast moves every score by ~0.26
            # nats rms, and on a row whose diagonal key has a visible rival
            # within a few nats that is 0.14..0.34 of output error (B > 1
            # prefill rows; the CPU emulation with an e4m3 Q reproduces the
            # kernel's worst rows to 0.01, docs/NEEDLE_TESTS.md). So the sum
            # is rounded to e4m3 HERE, and kernel and oracle read one query.
            anchored = anchored.to(torch.float8_e4m3fn).float()
        q = torch.where(hidden, anchored, qf).to(qdt)
    if case.kind == "mx_hw":
        ref_q = q.float().to(torch.float8_e4m3fn).float()  # in-kernel e4m3 Q
        ref_k, ref_v = kf, vf
    elif case.kind == "mx_dequant":
        ref_q, ref_k, ref_v = q.float(), kf.bfloat16().float(), \
            vf.bfloat16().float()
    else:
        ref_q, ref_k, ref_v = q.float(), kf, vf
    causal = family in CAUSAL_FAMILIES
    return Needle(case, family, causal, case.qoff if causal else 0, 0,
                  case.softmax_scale, tg, q, k, v, mx, ref_q, ref_k, ref_v, tg2)


PAIR_NATS = (0.7, 1.5)   # |score(t1) - score(t2)| of a `pair` row


def pair_query(case: Case, tg: torch.Tensor, kf: torch.Tensor, gain: float,
               qdt: torch.dtype):
    """The `pair` family: row r is gain * (K[t1] + K[t2]) with t1 the row's
    seam target and t2 a key of the PARTNER split (split(t1) + ceil(S/2))
    % S, S the splits that hold live keys. Each split's partial stays
    one-hot (p = 1 in its own split, exact in e4m3), and the two partials
    meet in the fp32 combine at weights between 0.82 / 0.18 and 0.67 / 0.33:
    t2 is the key of the partner split that brings the two scores nearest
    1.1 nats apart (brute force; a drawn t2 leaves a median minor weight of
    0.04). The sum is rounded to the query dtype, for the e4m3-Q kinds to
    e4m3 first (the anchored first_masked precedent); the oracle reads the
    rounded query. -> (t2 (B, Hq, Tq), q)."""
    s_live = case.live_splits
    assert s_live >= 2, f"{case.id}: a pair needs two live splits"
    g = case.hq // case.hkv
    t2 = torch.empty_like(tg)
    q = torch.empty(*tg.shape, case.d, dtype=qdt)
    for i in range(case.b):
        for h in range(case.hq):
            for r in range(case.tq):
                t2[i, h, r], q[i, h, r] = pair_key(
                    kf[i, h // g, :case.tkv], int(tg[i, h, r]), s_live,
                    case.plan[1], gain, case.softmax_scale,
                    case.kind != "half", qdt, what=(case.id, i, h, r))
    return t2, q


def pair_key(keys: torch.Tensor, t1: int, s_live: int, chunk: int,
             gain: float, scale: float, e4m3_q: bool, qdt: torch.dtype,
             what=""):
    """The second target of one `pair` row over `keys` (T, D) fp32, the live
    keys of its KV head, and the row's query: -> (t2, q (D,) in qdt)."""
    k1, kall = keys[t1], keys.double()
    # a partner split of one or a few keys (the tail of 2049) may hold no
    # key in range: then the next split serves
    for step in range(s_live - 1):
        sp = (t1 // chunk + (s_live + 1) // 2 + step) % s_live
        if sp == t1 // chunk:
            continue
        lo, hi = sp * chunk, min((sp + 1) * chunk, keys.shape[0])
        kc = keys[lo:hi]
        qc = gain * (k1[None, :] + kc)
        if e4m3_q:
            qc = _e4m3(qc)
        qc = qc.to(qdt)
        s1 = (qc.double() * k1.double()).sum(-1) * scale
        s2 = (qc.double() * kc.double()).sum(-1) * scale
        nats = (s1 - s2).abs()
        # nearest 1.1 nats first; a candidate whose sum query lifts a third
        # key past 0.5 % of the weight (one row in 64 at 40000 keys) gives
        # way to the next
        for j in (nats - sum(PAIR_NATS) / 2).abs().argsort():
            j = int(j)
            if not PAIR_NATS[0] <= float(nats[j]) <= PAIR_NATS[1]:
                break
            sc = (kall @ qc[j].double()) * scale
            two = torch.logsumexp(torch.stack([s1[j], s2[j]]), 0)
            if float(torch.exp(two - torch.logsumexp(sc, 0))) >= 0.995:
                return lo + j, qc[j]
    raise AssertionError(f"no second target for {what}")


@lru_cache(maxsize=None)
def build(case: Case, family: str) -> Needle:
    return build_from(case, family, *_kv(case))


def guard_rows(nd: Needle, n: int):
    """n guard rows per KV head: decoy K = 4 * (direction of a query of that
    head's group, rotating over its rows) and V = NaN. A kernel that admits
    one gives it ~4x the target's score and a NaN output; one that merely
    multiplies it by p = 0 still gets NaN."""
    c = nd.case
    g = c.hq // c.hkv
    j = torch.arange(n)
    heads = torch.arange(c.hkv)[:, None] * g + (j % g)[None, :]   # (Hkv, n)
    rows = ((j // g) % c.tq)[None, :].expand(c.hkv, n)
    gk = 2.0 * nd.q.float()[:, heads, rows]             # twice the query
    gv = torch.full_like(gk, float("nan"))
    return gk, gv


def guarded(t: torch.Tensor, T: int, pre: int, post: int,
            fill: torch.Tensor) -> torch.Tensor:
    """A length-T view of `t`'s rows inside a larger buffer whose `pre` rows
    before and `post` rows after hold `fill` (rotating). B = 1, Hkv = 1: the
    size-1 dims hide the strides, so the view is is_contiguous() and passes
    the bindings' checks without a copy."""
    assert t.shape[0] == 1 and t.shape[1] == 1 and t.shape[2] == T
    n = pre + T + post
    buf = torch.empty(1, 1, n, t.shape[3], dtype=t.dtype, device=t.device)
    f = fill.to(device=t.device)
    nf = f.shape[2]
    buf[:, :, :pre] = f[:, :, torch.arange(pre) % nf].to(t.dtype)
    buf[:, :, pre + T:] = f[:, :, torch.arange(post) % nf].to(t.dtype)
    buf[:, :, pre:pre + T] = t
    view = buf[:, :, pre:pre + T]
    assert view.is_contiguous() and view.data_ptr() != buf.data_ptr()
    return view


# --------------------------------------------------------------------------
# fp64 oracle, mutable
# --------------------------------------------------------------------------
def _e4m3(x: torch.Tensor) -> torch.Tensor:
    return x.float().to(torch.float8_e4m3fn).float()


def _round_p(p: torch.Tensor, how: str) -> torch.Tensor:
    if how == "e4m3":      # the fp8 kernels quantize 448 * P
        return (p * 448.0).float().to(torch.float8_e4m3fn).double() / 448.0
    return p.float().to(_TD[how]).double()


def oracle(q, k, v, *, causal=False, q_offset=0, kv_offset=0, scale=None,
           mutant=None, guard=None, p_round=None, q_round=None):
    """Naive fp64 attention -> (out, lse), optionally MUTATED:

    "mask+1" / "mask-1"    causal mask admits one key too many / hides the
                           diagonal key
    "kvoff+1" / "kvoff-1"  kv_offset off by one
    "drop_last"            last key dropped (tail off-by-one)
    "past_end"             one key past the end admitted (`guard` = the rows
                           that lie there: (gk, gv))
    ("vswap", a, b)        V rows a and b exchanged
    "gqa_mod"              GQA head map h % Hkv instead of h // G
    "row_transpose"        (head, row) order of the G*Tq row batch transposed
    "batch_kv0"            every batch reads batch 0's K/V
    "batch_out_swap"       out and lse of batches i and i^1 exchanged
    "bh_transposed"        the block at flat index b*Hq + h works on the pair
                           (idx % B, idx / B) and stores where (b, h) belongs
    "scale_ignored"        1/sqrt(D) used whatever scale is passed
    "scale_sqrt128"        1/sqrt(128) used
    """
    if q_round == "e4m3":   # the fp8 and MX kernels cast Q once
        q = _e4m3(q)
    elif q_round is not None:
        raise ValueError(q_round)
    q, k, v = q.double(), k.double(), v.double()
    b, hq, tq, d = q.shape
    hkv = k.shape[1]
    g = hq // hkv
    scale = 1.0 / math.sqrt(d) if scale is None else scale
    shift = 0
    if mutant == "mask+1":
        shift = 1
    elif mutant == "mask-1":
        shift = -1
    elif mutant == "kvoff+1":
        kv_offset += 1
    elif mutant == "kvoff-1":
        kv_offset -= 1
    elif mutant == "drop_last":
        k, v = k[:, :, :-1], v[:, :, :-1]
    elif mutant == "past_end":
        k = torch.cat([k, guard[0][:, :, :1].double()], 2)
        v = torch.cat([v, guard[1][:, :, :1].double()], 2)
    elif isinstance(mutant, tuple) and mutant[0] == "vswap":
        v = v.clone()
        v[:, :, [mutant[1], mutant[2]]] = v[:, :, [mutant[2], mutant[1]]]
    elif mutant == "row_transpose":
        q = q.reshape(b, hkv, tq, g, d).transpose(2, 3).reshape(b, hq, tq, d)
    elif mutant == "batch_kv0":
        k, v = k[:1].expand_as(k), v[:1].expand_as(v)
    elif mutant == "scale_ignored":
        scale = 1.0 / math.sqrt(d)
    elif mutant == "scale_sqrt128":
        scale = 1.0 / math.sqrt(128)
    elif mutant not in (None, "gqa_mod", "batch_out_swap", "bh_transposed"):
        raise ValueError(mutant)
    tk = k.shape[2]
    if tk == 0:
        return (torch.zeros(b, hq, tq, d, dtype=torch.float64),
                torch.full((b, hq, tq), float("-inf"), dtype=torch.float64))
    if mutant == "gqa_mod":
        kvh = torch.arange(hq) % hkv
        k, v, grp = k[:, kvh], v[:, kvh], 1
    else:
        grp = g     # head h reads KV head h // g: G heads share one matmul
    # (B, Hq, Tq, .) <-> (B, Hq/grp, grp*Tq, .): K/V are never expanded
    fold = lambda x: x.reshape(b, hq // grp, grp * tq, x.shape[-1])
    s = torch.matmul(fold(q), k.transpose(-1, -2)).reshape(b, hq, tq, tk) \
        * scale
    if causal:
        qpos = q_offset + torch.arange(tq)
        kpos = kv_offset + torch.arange(tk)
        s = s.masked_fill(kpos[None, :] > qpos[:, None] + shift,
                          float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    m = s.amax(dim=-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(s - m)
    den = p.sum(dim=-1, keepdim=True)
    den = torch.where(den == 0, torch.ones_like(den), den)
    if p_round:
        p = _round_p(p, p_round)
    out = torch.matmul(fold(p), v).reshape(b, hq, tq, d) / den
    if mutant == "batch_out_swap":
        src = torch.arange(b) ^ 1
        src = torch.where(src < b, src, torch.arange(b))
        out, lse = out[src], lse[src]
    elif mutant == "bh_transposed":
        idx = torch.arange(b * hq)
        src = (idx % b) * hq + idx // b
        out = out.reshape(b * hq, tq, d)[src].reshape(b, hq, tq, d)
        lse = lse.reshape(b * hq, tq)[src].reshape(b, hq, tq)
    return out, lse


def mutants(case: Case) -> list:
    """Every mutant that applies to a case's family set. mask+1 / kvoff-1
    need a hidden key to admit (first_masked); mask-1 / kvoff+1 need a
    diagonal (diag); the length and V-placement mutants need the non-causal
    seam family, where every key is visible."""
    fam, out = case.families, []
    if "first_masked" in fam:
        out += ["mask+1", "kvoff-1"]
    if "diag" in fam:
        out += ["mask-1", "kvoff+1"]
    if "seam" in fam:
        out += ["drop_last", "past_end"]
        if case.tkv > 1:
            out.append(("vswap", 0, case.tkv - 1))
        out += [("vswap", s - 1, s) for s in case.seams]
    g = case.hq // case.hkv
    if g > 1 and case.hkv > 1:
        out.append("gqa_mod")
    if g > 1 and case.tq > 1:
        out.append("row_transpose")
    if case.b > 1:
        out += ["batch_kv0", "batch_out_swap", "bh_transposed"]
    if case.scale:
        out.append("scale_ignored")
    if case.d != 128:
        out.append("scale_sqrt128")
    return out


def emulation_q_round(case: Case):
    """fa_fwd_fp8_kernel, fa_prefill2_fp8_kernel<MX> and
    fa_decode_fp8_mx_kernel cast Q to e4m3 (an MX row's ref_q already is)."""
    return "e4m3" if case.kind in ("fp8", "mx_hw") else None


def emulation_p_round(case: Case) -> str:
    if case.kind in ("fp8", "mx_hw"):
        return "e4m3"
    return "fp16" if case.dtype == "fp16" else "bf16"


@lru_cache(maxsize=None)
def reference(case: Case, family: str):
    """The fp32 oracle (ops/reference.flash_res_lse) every test compares
    with; computed once per (case, family) and shared."""
    from tree_attention_torch_amd.ops.reference import flash_res_lse

    nd = build(case, family)
    return flash_res_lse(nd.ref_q, nd.ref_k, nd.ref_v, nd.scale, nd.causal,
                         nd.q_offset, nd.kv_offset)


# --------------------------------------------------------------------------
# fp64 split oracle: per-split partials by split_plan, merged by the stable
# algebra; the split and combine errors are mutations of it
# --------------------------------------------------------------------------
SEAM_KEYS = 128    # seam_twice / seam_skipped move the first 128 keys


def many_split_cases() -> list:
    """The rows whose split-KV call has more than two splits."""
    return [c for c in CASES if c.plan is not None and c.plan[0] > 2]


def merge_partials(outs: torch.Tensor, lses: torch.Tensor):
    """Stable merge over dim 0 in the dtype given: m = max lse, w =
    exp(lse - m), out = sum w out / sum w, lse = m + log sum w; an all-masked
    row gives out = 0, lse = -inf."""
    m = lses.amax(0)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    w = torch.exp(lses - m)              # exp(-inf) = 0 for a masked partial
    den = w.sum(0)
    safe = torch.where(den == 0, torch.ones_like(den), den)
    out = (outs * w.unsqueeze(-1)).sum(0) / safe.unsqueeze(-1)
    lse = torch.where(den == 0, torch.full_like(den, float("-inf")),
                      m + torch.log(safe))
    return out, lse


@dataclass
class SplitParts:
    """fp64 partials of every split of a case's plan, each in two pieces:
    `head` over the split's first SEAM_KEYS keys and `rest` over the others;
    (S, B, Hq, Tq, D) and (S, B, Hq, Tq). A split past the live length is
    empty: out = 0, lse = -inf."""
    case: Case
    head_o: torch.Tensor
    head_l: torch.Tensor
    rest_o: torch.Tensor
    rest_l: torch.Tensor

    def whole(self):
        return merge_partials(torch.stack([self.head_o, self.rest_o]),
                              torch.stack([self.head_l, self.rest_l]))


def split_parts(nd: Needle, *, length: int | None = None, p_round=None,
                q_round=None) -> SplitParts:
    """Partials of nd over the splits of its case's plan. `length` cuts the
    KV at another live length than the case's (cache rows): keys past the
    case's own come from the guard pattern. p_round / q_round emulate the
    kernel's arithmetic PER SPLIT, as the kernels round P against the
    running max of their own split."""
    c = nd.case
    s_all, chunk = c.plan
    k, v = nd.ref_k, nd.ref_v
    n = c.tkv if length is None else length
    if n > c.tkv:
        gk, gv = guard_rows(nd, n)
        k = torch.cat([k, gk[:, :, c.tkv:]], 2)
        v = torch.cat([v, gv[:, :, c.tkv:]], 2)
    pieces = ([], [], [], [])
    for s in range(s_all):
        lo, hi = s * chunk, min((s + 1) * chunk, n)
        mid = min(lo + SEAM_KEYS, hi)
        for j, (a, b) in enumerate(((lo, mid), (mid, hi))):
            o, l = oracle(nd.ref_q, k[:, :, a:max(a, b)], v[:, :, a:max(a, b)],
                          causal=nd.causal, q_offset=nd.q_offset,
                          kv_offset=nd.kv_offset + a, scale=nd.scale,
                          p_round=p_round, q_round=q_round)
            pieces[2 * j].append(o)
            pieces[2 * j + 1].append(l)
    return SplitParts(c, *(torch.stack(p) for p in pieces))


def split_oracle(nd: Needle, **kw):
    """Attention through the split plan: per-split partials, merged."""
    return merge_partials(*split_parts(nd, **kw).whole())


def split_mutants(case: Case) -> list:
    """The split and combine errors a many-split row must expose."""
    s_live, chunk = case.live_splits, case.plan[1]
    half = (s_live + 1) // 2
    out = [("split_drop", s) for s in range(s_live)]
    out += [("split_oswap", s, (s + half) % s_live) for s in range(s_live)
            if s_live > 1]
    if s_live > case.combine_groups:
        out.append("combine_first_group")
    if s_live > 1:
        out += ["combine_mean", "lse_row_shift"]
    if "pair" in case.families:
        out.append("weight_base2")
    # the seam mutants move the first keys of split s: seen where the row
    # targets key s * chunk (every split seam, but for the 63-split rows,
    # whose 64 rows reach the odd seams). Counting a one-hot key twice
    # leaves `out` alone and adds ln 2 to lse, inside the lse bars of the
    # e4m3-P kinds (5e-2 and 3e-2 of ~23): there the pair family sees it,
    # and the one row of those kinds without one (fp8 cache, 513 live keys)
    # cannot
    named = [s for s in range(1, s_live) if s * chunk in case.seams]
    if "pair" in case.families or case.kind not in ("fp8", "mx_hw"):
        out += [("seam_twice", s) for s in named]
    out += [("seam_skipped", s) for s in [0] + named]
    if 0 < case.tkv - (s_live - 1) * chunk < case.tile and s_live > 1:
        out.append("tail_split_empty")
    if case.route == "cache" and case.tkv % chunk:
        out += [("len_rounds_to_chunk", "down"), ("len_rounds_to_chunk", "up")]
    return out


def split_mutant(nd: Needle, parts: SplitParts, mut):
    """(out, lse) of the split oracle with one error built in:

    ("split_drop", s)         split s never reaches the combine
    ("split_oswap", s, t)     out partials of s and t exchanged, lse kept
    "combine_first_group"     only the first NG splits reduced (NG of
                              fa_combine_kernel: 4, or 8 at D = 64)
    "combine_mean"            unweighted mean of the non-empty out partials,
                              final lse right
    "weight_base2"            w = 2^(l - m), final lse right
    "lse_row_shift"           weights of row r taken from row r ^ 1, final
                              lse right
    ("seam_twice", s)         the first 128 keys of split s also counted in
                              split s - 1
    ("seam_skipped", s)       ... counted in neither
    "tail_split_empty"        a last split shorter than one tile dropped
    ("len_rounds_to_chunk", "down" | "up")
                              live length rounded to a chunk boundary (up:
                              into the guard pattern)
    """
    c = nd.case
    name = mut if isinstance(mut, str) else mut[0]
    if name == "len_rounds_to_chunk":
        chunk = c.plan[1]
        n = c.tkv // chunk * chunk + (chunk if mut[1] == "up" else 0)
        return split_oracle(nd, length=n)
    o, l = parts.whole()
    true_out, true_lse = merge_partials(o, l)
    if name == "split_drop" or name == "tail_split_empty":
        s = mut[1] if name == "split_drop" else c.live_splits - 1
        keep = [i for i in range(o.shape[0]) if i != s]
        return merge_partials(o[keep], l[keep])
    if name == "split_oswap":
        idx = list(range(o.shape[0]))
        idx[mut[1]], idx[mut[2]] = mut[2], mut[1]
        return merge_partials(o[idx], l)
    if name == "combine_first_group":
        ng = c.combine_groups
        return merge_partials(o[:ng], l[:ng])
    if name == "seam_twice":
        s = mut[1]
        o, l = o.clone(), l.clone()
        o[s - 1], l[s - 1] = merge_partials(
            torch.stack([o[s - 1], parts.head_o[s]]),
            torch.stack([l[s - 1], parts.head_l[s]]))
        return merge_partials(o, l)
    if name == "seam_skipped":
        s = mut[1]
        o, l = o.clone(), l.clone()
        o[s], l[s] = parts.rest_o[s], parts.rest_l[s]
        return merge_partials(o, l)
    # the weight mutants: the final lse stays right
    m = l.amax(0)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    if name == "combine_mean":
        w = torch.isfinite(l).double()
    elif name == "weight_base2":
        w = torch.exp2(l - m)
    elif name == "lse_row_shift":
        flat = torch.exp(l - m).reshape(l.shape[0], -1)
        src = torch.arange(flat.shape[1]) ^ 1
        src = torch.where(src < flat.shape[1], src, src ^ 1)
        w = flat[:, src].reshape(l.shape)
    else:
        raise ValueError(mut)
    den = w.sum(0)
    den = torch.where(den == 0, torch.ones_like(den), den)
    return (o * w.unsqueeze(-1)).sum(0) / den.unsqueeze(-1), true_lse


# --------------------------------------------------------------------------
# the one comparison
# --------------------------------------------------------------------------
def compare(out, lse, ref_out, ref_lse, kind: str) -> None:
    """assert_close at the project's bars for `kind`. `lse=None` compares
    `out` alone (graph replay hands back no lse)."""
    ob, lb = BARS[kind]
    torch.testing.assert_close(out.detach().float().cpu(),
                               ref_out.detach().float().cpu(),
                               rtol=ob, atol=ob)
    if lse is not None:
        torch.testing.assert_close(lse.detach().float().cpu(),
                                   ref_lse.detach().float().cpu(),
                                   rtol=lb, atol=lb)


def rejected(out, lse, ref_out, ref_lse, kind: str) -> bool:
    try:
        compare(out, lse, ref_out, ref_lse, kind)
    except AssertionError:
        return True
    return False


def check(nd: Needle, out, lse, what: str = "", ref=None) -> None:
    """compare() against the shared reference (or `ref`, for needles built
    over K/V read back from a session); on failure name the worst row's
    batch, head, target, the seam it sits at and the family."""
    ref_out, ref_lse = ref or reference(nd.case, nd.family)
    try:
        compare(out, lse, ref_out, ref_lse, nd.case.kind)
    except AssertionError as e:
        o = out.detach().float().cpu()
        ob = BARS[nd.case.kind][0]
        err = (o - ref_out).abs().nan_to_num(nan=float("inf"))
        out_failed = bool((err > ob + ob * ref_out.abs()).any())
        err = err.amax(-1)
        if lse is not None and not out_failed:   # then it was lse
            err = (lse.detach().float().cpu() - ref_lse).abs().nan_to_num(
                nan=float("inf"))
        i, hr = divmod(int(err.argmax()), err.shape[1] * err.shape[2])
        h, r = divmod(hr, err.shape[2])
        tgt = int(nd.targets[i, h, r])
        near = min(nd.case.seams or (0,), key=lambda s: abs(s - tgt))
        raise AssertionError(
            f"{nd.case.id} [{nd.family}] {what}: worst row batch {i} of "
            f"{nd.case.b} head {h} row {r} "
            f"(position {nd.q_offset + r}) target key {tgt}, nearest seam "
            f"{near}, seams {nd.case.seams}, cuts {nd.case.cuts}\n{e}"
        ) from None


# --------------------------------------------------------------------------
# GPU runners (also used by the env-variant child processes)
# --------------------------------------------------------------------------
def _kv_dev(nd: Needle, use_guard: bool):
    k, v = nd.k.cuda(), nd.v.cuda()
    if use_guard:
        gk, gv = guard_rows(nd, GUARD_PRE + GUARD_POST)
        k = guarded(k, nd.case.tkv, GUARD_PRE, GUARD_POST, gk)
        v = guarded(v, nd.case.tkv, GUARD_PRE, GUARD_POST, gv)
    return k, v


def run_kernel(nd: Needle, use_guard: bool = False):
    """One (case, family) through the real entry point of its route."""
    from tree_attention_torch_amd.ops import flash

    ext = flash._load_extension()
    assert ext is not None, "HIP extension must be built in-tree"
    c, q = nd.case, nd.q.cuda()
    args = (nd.scale, nd.causal, nd.q_offset, nd.kv_offset)
    if c.route in ("mx_hw", "mx_dequant"):
        return flash.local_attention_mx(q, *(t.cuda() for t in nd.mx), *args)
    if c.route == "prefill_mx":
        return ext.flash_attention_fp8_mx(q, *(t.cuda() for t in nd.mx),
                                          *args)
    k, v = _kv_dev(nd, use_guard)
    if c.route in PREFILL_ROUTES:
        assert c.tq > 16 // (c.hq // c.hkv)     # the binding's prefill side
        return ext.flash_attention(q, k, v, *args)
    if c.route == "spec":
        assert flash.decode_loop_chunks(c.tq, c.hq // c.hkv, c.b, c.hq) > 1
    else:
        assert c.route.startswith("decode"), c.route
        assert c.tq * (c.hq // c.hkv) <= 16
    return flash.local_attention(q, k, v, *args)


def cache_buffers(nd: Needle):
    """(B, Hkv, capacity, D) K/V caches: the needle's keys as the live
    prefix, the guard pattern (decoy K, NaN V) in every row at and past
    it."""
    c = nd.case
    gk, gv = guard_rows(nd, c.capacity)
    kc, vc = gk.to(nd.k.dtype).cuda(), gv.to(nd.v.dtype).cuda()
    kc[:, :, :c.tkv] = nd.k.cuda()
    vc[:, :, :c.tkv] = nd.v.cuda()
    return kc, vc


def run_cache(nd: Needle):
    from tree_attention_torch_amd.ops import flash

    ext = flash._load_extension()
    kc, vc = cache_buffers(nd)
    len_dev = torch.full((1,), nd.case.tkv, dtype=torch.long, device="cuda")
    return ext.flash_attention_cache(nd.q.cuda(), kc, vc, len_dev, nd.scale)


def run_sharded(nd: Needle):
    """Per-shard partials with the global q_offset and the shard's
    kv_offset, merged by combine_partials; plus the unsharded call."""
    from tree_attention_torch_amd.ops import flash
    from tree_attention_torch_amd.parallel.combine import combine_partials

    c, q = nd.case, nd.q.cuda()
    outs, lses = [], []
    for lo, hi in zip(c.cuts[:-1], c.cuts[1:]):
        if c.dtype == "mx":
            k8, ks, v8, vs = (t.cuda() for t in nd.mx)
            o, l = flash.local_attention_mx(
                q, k8[:, :, lo:hi], ks[:, :, lo:hi], v8[:, :, lo:hi],
                vs[:, :, lo // 32:hi // 32], nd.scale, nd.causal,
                nd.q_offset, lo)
        else:
            o, l = flash.local_attention(
                q, nd.k.cuda()[:, :, lo:hi], nd.v.cuda()[:, :, lo:hi],
                nd.scale, nd.causal, nd.q_offset, lo)
        outs.append(o)
        lses.append(l)
    merged = combine_partials(torch.stack(outs), torch.stack(lses))
    if c.dtype == "mx":
        whole = flash.local_attention_mx(q, *(t.cuda() for t in nd.mx),
                                         nd.scale, nd.causal, nd.q_offset, 0)
    else:
        whole = flash.local_attention(q, nd.k.cuda(), nd.v.cuda(), nd.scale,
                                      nd.causal, nd.q_offset, 0)
    return merged, whole


def variant_cases() -> list[Case]:
    """The prefill rows the env-latched bf16 variants run."""
    return [c for c in CASES if c.route == "prefill" and c.dtype == "bf16"]


def remap_cases() -> list[Case]:
    """The bf16 gen7 rows that also run with TREE_ATTN_REMAP=0: B*Hq >= 8,
    i.e. the rows of both remap branches with B > 1 or Hq = 8."""
    return [c for c in variant_cases() if c.b * c.hq >= 8]


def run_variant_rows() -> None:
    """Child-process body of the env-latched variant test: every bf16
    prefill row of the table, every family, plain and guarded."""
    n = 0
    for c in variant_cases():
        for fam in c.families:
            nd = build(c, fam)
            for use_guard in ((False, True) if c.guard else (False,)):
                out, lse = run_kernel(nd, use_guard)
                check(nd, out, lse, "guarded" if use_guard else "plain")
                n += 1
    torch.cuda.synchronize()
    print(f"NEEDLES_OK {n}")
