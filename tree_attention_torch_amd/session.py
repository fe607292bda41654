"""Serving-style decode session: a preallocated, sequence-sharded KV cache.

The reference computes attention over freshly-generated random tensors each
run (/root/reference/model.py:145-150); a deployment decodes token by token,
appending each new token's K/V to a cache. This module provides that loop
MI355X-style:

* the cache is preallocated in HBM3E (288 GB/GPU: a 2M-token GQA fp8 cache
  is ~2 GB) and sharded across ranks round-robin by BLOCKS of tokens, so
  every rank's shard stays contiguous for the flash kernel and growth does
  not reshuffle data;
* each decode step appends to exactly ONE rank's shard and runs
  tree_attention over all shards (the stable combine handles ragged shard
  lengths — lse weighting is exact for any split);
* causal correctness across shards comes from per-shard global position
  offsets, maintained here.

Block-cyclic layout: token t lives on rank (t // block) % world at local
position block*((t // block) // world) + t % block.
"""

from __future__ import annotations

import math

import torch
import torch.distributed as dist

from .ops.flash import local_attention
from .parallel.combine import combine_partials, tree_combine

__all__ = ["DecodeSession", "RaggedDecodeSession", "PagedDecodeSession"]

_DTYPES = {
    "bf16": torch.bfloat16,
    "fp16": torch.float16,
    "fp32": torch.float32,
    "fp8": torch.float8_e4m3fn,
}


def _rank_world(group) -> tuple[int, int]:
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(group), dist.get_world_size(group)
    return 0, 1


def _local_cap(max_tokens: int, block: int, world: int) -> int:
    """Positions max_tokens asks of one rank's shard: whole blocks, one
    spare."""
    blocks_total = (max_tokens + block - 1) // block + 1
    return ((blocks_total + world - 1) // world) * block


def _scale(softmax_scale: float | None, q: torch.Tensor) -> float:
    return (softmax_scale if softmax_scale is not None
            else 1.0 / math.sqrt(q.shape[-1]))


def _place(t: int, block: int, world: int) -> tuple[int, int]:
    """(owning rank, local position) of global token t: the block-cyclic
    formula of the module docstring. kv_append_kernel (ops/hip) computes the
    same two numbers on the device."""
    blk = t // block
    return blk % world, block * (blk // world) + t % block


def _n_local(t: int, block: int, rank: int, world: int) -> int:
    """How many of the first t global tokens of a sequence `rank` owns: the
    count _place implies, and local_len after t contiguous appends. A shard's
    local positions are ordered by global position, so "sees global
    positions < t" is "sees the local prefix of length _n_local(t)"
    (kv_append_n_kernel computes the same number on the device)."""
    full = t // block
    return (block * ((full + world - 1 - rank) // world)
            + (t % block if full % world == rank else 0))


def _tree_masks(t0: int, cnt: int, parents: list[int], t: int, block: int,
                rank: int, world: int) -> tuple[int, list[int]]:
    """(base, masks) of one row of a tree append, as kv_append_tree_kernel
    leaves them: base = _n_local(t0); bit s of masks[i] is set when the
    draft node at local slot s (local position base + s) is query i's own
    node or one of its ancestors and `rank` owns it. The walk i ->
    parents[i] -> ... clamps every step into [-1, node - 1], so it ends
    whatever the table holds; queries at or past cnt get 0."""
    base = _n_local(t0, block, rank, world)
    masks = []
    for i in range(t):
        m, n = 0, (i if i < cnt else -1)
        while n >= 0:
            if _place(t0 + n, block, world)[0] == rank:
                m |= 1 << (_n_local(t0 + n + 1, block, rank, world) - 1
                           - base)
            n = min(max(int(parents[n]), -1), n - 1)
        masks.append(m)
    return base, masks


def _empty_partial(q: torch.Tensor):
    """The partial of a shard that holds no key: out = 0, lse = -inf."""
    b, hq, tq, d = q.shape
    out_l = torch.zeros(b, hq, tq, d, dtype=torch.float32, device=q.device)
    lse_l = torch.full((b, hq, tq), float("-inf"), dtype=torch.float32,
                       device=q.device)
    return out_l, lse_l


def _zero_copy_ok(q: torch.Tensor, k: torch.Tensor,
                  any_tq: bool = False) -> bool:
    """Whether the zero-copy cache kernels take q over the KV store k (a
    cache slab or a page pool: only its dtype, head count and head_dim are
    read). Mirrors the TORCH_CHECKs of bindings.cpp cache_decode: D=128; q
    bf16/fp16; KV dtype == q dtype or fp8 KV under a bf16 q; (Hq/Hkv)*Tq <=
    16 (MFMA-M batching). any_tq: the visible-length bindings
    (cache_decode_qlen) loop over groups of query positions, so only Hq/Hkv
    <= 16 is asked."""
    return (
        q.device.type == "cuda"
        and k.size(3) == 128
        and q.dtype in (torch.bfloat16, torch.float16)
        and (
            k.dtype == q.dtype
            or (k.dtype == torch.float8_e4m3fn and q.dtype == torch.bfloat16)
        )
        and (q.shape[1] // k.shape[1]) * (1 if any_tq else q.shape[2]) <= 16
    )


def _capture(fn):
    """Warm fn up on a side stream (allocator + kernels), then capture it
    into a hipGraph -> (graph, what fn returned under capture)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fn()
    return graph, out


class DecodeSession:
    """Token-by-token decode over a sharded, growable KV cache."""

    def __init__(
        self,
        batch: int,
        kv_heads: int,
        head_dim: int,
        max_tokens: int,
        device: torch.device | str = "cuda",
        kv_dtype: str | torch.dtype = "bf16",
        block: int = 256,
        group: dist.ProcessGroup | None = None,
    ) -> None:
        self.device = torch.device(device)
        self.rank, self.world = _rank_world(group)
        self.group = group
        self.block = block
        self.mx = isinstance(kv_dtype, str) and kv_dtype in ("mx", "fp8_mx")
        local_cap = _local_cap(max_tokens, block, self.world)
        if self.mx:
            # MX block-scaled fp8 cache (quant.py layout): e4m3 payload +
            # per-block E8M0 scales, quantized in closed 64-token WINDOWS
            # (the scale-block granularity). Tokens land in a bf16 staging
            # tail first; each full window quantizes into the main cache.
            # attend() merges the quantized-prefix partial (hardware
            # mfma_scale decode kernel, ZERO-COPY strided views of this
            # preallocated cache) with the tail partial (bf16 kernel) via
            # the standard lse algebra — so per-token accuracy of the
            # newest <=63 tokens is full bf16 and the long prefix streams
            # at fp8 bandwidth with outlier-robust block scales.
            if head_dim != 128:
                raise ValueError("MX KV cache requires head_dim=128")
            if block % 64:
                raise ValueError("MX KV cache requires block % 64 == 0")
            self.k = torch.empty(batch, kv_heads, local_cap, head_dim,
                                 dtype=torch.float8_e4m3fn,
                                 device=self.device)
            self.v = torch.empty_like(self.k)
            self.ks = torch.empty(batch, kv_heads, local_cap, 4,
                                  dtype=torch.uint8, device=self.device)
            self.vs = torch.empty(batch, kv_heads, local_cap // 32,
                                  head_dim, dtype=torch.uint8,
                                  device=self.device)
            self.k_tail = torch.empty(batch, kv_heads, 64, head_dim,
                                      dtype=torch.bfloat16,
                                      device=self.device)
            self.v_tail = torch.empty_like(self.k_tail)
            self.q_len = 0     # quantized prefix length (multiple of 64)
            self.tail_len = 0  # bf16 staging-tail tokens (< 64)
        else:
            td = _DTYPES[kv_dtype] if isinstance(kv_dtype, str) else kv_dtype
            self.k = torch.empty(batch, kv_heads, local_cap, head_dim,
                                 dtype=td, device=self.device)
            self.v = torch.empty_like(self.k)
        self.total = 0       # global tokens appended so far
        self.local_len = 0   # tokens in THIS rank's shard

    def _owner(self, t: int) -> int:
        return (t // self.block) % self.world

    def append(self, k_new: torch.Tensor, v_new: torch.Tensor) -> None:
        """Append one token's K/V (B, Hkv, 1, D). Every rank calls this with
        the same tensors; only the owning rank stores them."""
        if self._owner(self.total) == self.rank:
            if self.local_len >= self.k.size(2):
                # without this check the slice assignment below would be an
                # EMPTY slice and a size-1 source legally expands to 0 rows:
                # the append would silently drop the token
                raise RuntimeError(
                    f"DecodeSession capacity exceeded: local shard full at "
                    f"{self.local_len} tokens (grow max_tokens)"
                )
            if self.mx:
                self._store_mx(k_new, v_new)
            else:
                self.k[:, :, self.local_len : self.local_len + 1] = \
                    k_new.to(self.k.dtype)
                self.v[:, :, self.local_len : self.local_len + 1] = \
                    v_new.to(self.v.dtype)
            self.local_len += 1
        self.total += 1

    def _store_mx(self, kc: torch.Tensor, vc: torch.Tensor) -> None:
        """Store owned tokens (B, Hkv, n, D) into the MX cache: fill the
        bf16 tail, quantize each full 64-token window (bulk windows
        quantize directly when the tail is empty)."""
        from .quant import quantize_k_mx, quantize_v_mx

        n, i = kc.shape[2], 0
        while i < n:
            if self.tail_len > 0 or n - i < 64:
                m = min(64 - self.tail_len, n - i)
                self.k_tail[:, :, self.tail_len : self.tail_len + m] = \
                    kc[:, :, i : i + m].to(torch.bfloat16)
                self.v_tail[:, :, self.tail_len : self.tail_len + m] = \
                    vc[:, :, i : i + m].to(torch.bfloat16)
                self.tail_len += m
                i += m
                if self.tail_len == 64:
                    k8w, ksw = quantize_k_mx(self.k_tail.float())
                    v8w, vsw = quantize_v_mx(self.v_tail.float())
                    q0 = self.q_len
                    self.k[:, :, q0 : q0 + 64] = k8w
                    self.ks[:, :, q0 : q0 + 64] = ksw
                    self.v[:, :, q0 : q0 + 64] = v8w
                    self.vs[:, :, q0 // 32 : q0 // 32 + 2] = vsw
                    self.q_len += 64
                    self.tail_len = 0
            else:
                m = (n - i) // 64 * 64
                # round through bf16 first so bulk-prefilled windows
                # quantize the SAME stream as tail-flushed ones (appends
                # stage in the bf16 tail before quantization)
                k8w, ksw = quantize_k_mx(
                    kc[:, :, i : i + m].to(torch.bfloat16).float())
                v8w, vsw = quantize_v_mx(
                    vc[:, :, i : i + m].to(torch.bfloat16).float())
                q0 = self.q_len
                self.k[:, :, q0 : q0 + m] = k8w
                self.ks[:, :, q0 : q0 + m] = ksw
                self.v[:, :, q0 : q0 + m] = v8w
                self.vs[:, :, q0 // 32 : (q0 + m) // 32] = vsw
                self.q_len += m
                i += m

    def _local_partial_mx(self, q: torch.Tensor,
                          softmax_scale: float | None):
        """MX-cache local partial: quantized-prefix partial (hardware MX
        decode kernel on GPU / dequantized oracle on CPU) merged with the
        bf16 staging-tail partial through the stable lse algebra."""
        parts = []
        if self.q_len > 0:
            if q.device.type == "cuda":
                from .ops.flash import local_attention_mx

                parts.append(local_attention_mx(
                    q, self.k[:, :, : self.q_len],
                    self.ks[:, :, : self.q_len],
                    self.v[:, :, : self.q_len],
                    self.vs[:, :, : self.q_len // 32], softmax_scale))
            else:
                from .quant import dequantize_k_mx, dequantize_v_mx

                kd = dequantize_k_mx(self.k[:, :, : self.q_len].contiguous(),
                                     self.ks[:, :, : self.q_len].contiguous())
                vd = dequantize_v_mx(
                    self.v[:, :, : self.q_len].contiguous(),
                    self.vs[:, :, : self.q_len // 32].contiguous())
                parts.append(local_attention(q.float(), kd, vd,
                                             softmax_scale))
        if self.tail_len > 0:
            kt = self.k_tail[:, :, : self.tail_len].contiguous()
            vt = self.v_tail[:, :, : self.tail_len].contiguous()
            if q.device.type == "cuda":
                parts.append(local_attention(q, kt.to(q.dtype),
                                             vt.to(q.dtype), softmax_scale))
            else:
                parts.append(local_attention(q.float(), kt.float(),
                                             vt.float(), softmax_scale))
        if not parts:
            return _empty_partial(q)
        if len(parts) == 1:
            return parts[0]
        return combine_partials(torch.stack([p[0] for p in parts]),
                                torch.stack([p[1] for p in parts]))

    def _local_partial(self, q: torch.Tensor, softmax_scale: float | None):
        if self.mx:
            return self._local_partial_mx(q, softmax_scale)
        # anything the zero-copy kernel does not take falls through to the
        # generic slice + local_attention path, which handles those cases
        if _zero_copy_ok(q, self.k):
            # zero-copy cache path: the kernel takes the cache's head stride
            # and reads the LIVE length from a device scalar, so this call
            # is hipGraph-capturable (graphed_attend) and never copies KV.
            from .ops.flash import _load_extension

            ext = _load_extension()
            if ext is not None:
                # NOTE: the length fill lives in sync_len(), NOT here — this
                # function body is hipGraph-captured by graphed_attend, and a
                # captured fill_ would freeze the capture-time length into
                # every replay.
                if not hasattr(self, "_len_dev"):
                    self._len_dev = torch.zeros(1, dtype=torch.long,
                                                device=self.device)
                return ext.flash_attention_cache(
                    q.contiguous(), self.k, self.v, self._len_dev,
                    _scale(softmax_scale, q))
        if self.local_len > 0:
            k = self.k[:, :, : self.local_len].contiguous()
            v = self.v[:, :, : self.local_len].contiguous()
            return local_attention(q, k, v, softmax_scale)
        return _empty_partial(q)

    def attend(self, q: torch.Tensor, softmax_scale: float | None = None,
               combine: str = "auto") -> torch.Tensor:
        """Attention of q (B, Hq, 1, D) over every cached token.

        All cached tokens precede the query (decode semantics), so no causal
        mask is needed; the block-cyclic placement therefore needs no
        position bookkeeping inside the kernel — only the shard contents
        matter, and the combine is permutation-invariant.
        """
        assert self.total > 0, "attend() before any append()"
        self.sync_len()
        out_l, lse_l = self._local_partial(q, softmax_scale)
        out, _ = tree_combine(out_l, lse_l, strategy=combine, group=self.group)
        return out

    def graphed_attend(self, q_static: torch.Tensor,
                       softmax_scale: float | None = None,
                       combine: str = "auto"):
        """Capture the decode-attend into a hipGraph.

        Returns (replay, out): write the query into q_static, keep
        self._len_dev fresh via sync_len(), call replay() -> output tensor.
        The kernel reads the live KV length from device memory, so ONE
        captured graph serves the whole growing sequence — no recapture.

        world_size 1: the whole step replays from the graph and ``out`` is
        the static output buffer. world_size > 1: the LOCAL partial replays
        from the graph (launch-bound part of the step) and the cross-rank
        combine collective runs eagerly per call — RCCL collectives are not
        capturable into a per-rank local graph, but they are a single
        latency-bound call on a ~16 KB payload; ``out`` is None and
        replay()'s return value is the fresh combined output.
        """
        assert self.device.type == "cuda"
        if self.mx:
            raise NotImplementedError(
                "graphed_attend: the MX cache path is two kernels + a "
                "python merge with per-call allocations; use eager "
                "attend() (the MX decode kernel itself is ~0.2 ms at "
                "128K — not launch-bound)")
        graph, (out_l, lse_l) = _capture(
            lambda: self._local_partial(q_static, softmax_scale))
        self._graph = graph  # keep alive

        if self.world == 1:
            def replay() -> torch.Tensor:
                graph.replay()
                return out_l

            return replay, out_l

        def replay_dist() -> torch.Tensor:
            graph.replay()
            out, _ = tree_combine(out_l, lse_l, strategy=combine,
                                  group=self.group)
            return out

        return replay_dist, None

    def sync_len(self) -> None:
        """Refresh the device-side length after append()s (graphed path)."""
        if hasattr(self, "_len_dev"):
            self._len_dev.fill_(self.local_len)
        elif self.device.type == "cuda":
            self._len_dev = torch.full((1,), self.local_len, dtype=torch.long,
                                       device=self.device)

    def prefill(self, k_seq: torch.Tensor, v_seq: torch.Tensor) -> None:
        """Bulk-append a prompt's K/V (B, Hkv, T, D), preserving the
        block-cyclic ownership (chunks split at global block boundaries)."""
        t_total = k_seq.shape[2]
        t = 0
        while t < t_total:
            n = min(self.block - self.total % self.block, t_total - t)
            if self._owner(self.total) == self.rank:
                if self.local_len + n > self.k.size(2):
                    raise RuntimeError(
                        f"DecodeSession capacity exceeded during prefill at "
                        f"{self.local_len}+{n} tokens (grow max_tokens)"
                    )
                if self.mx:
                    self._store_mx(k_seq[:, :, t : t + n],
                                   v_seq[:, :, t : t + n])
                else:
                    self.k[:, :, self.local_len : self.local_len + n] = \
                        k_seq[:, :, t : t + n].to(self.k.dtype)
                    self.v[:, :, self.local_len : self.local_len + n] = \
                        v_seq[:, :, t : t + n].to(self.v.dtype)
                self.local_len += n
            self.total += n
            t += n


# --------------------------------------------------------------------------
# ragged batch: one length per sequence
# --------------------------------------------------------------------------
class RaggedDecodeSession:
    """Token-by-token decode of a BATCH whose sequences have their own
    lengths, over the same block-cyclic sharded cache as DecodeSession.

    Sequences join (prefill, or fork from another sequence's prefix), grow
    (append with an ``active`` mask) and leave (reset) independently. The lengths live twice: ``total_dev`` /
    ``local_len_dev`` (B,) int64 on the device are what the kernels read, so
    a whole step (append kernel, cache kernel, split combine) replays from
    one hipGraph; ``totals`` / ``local_lens`` are the host mirror, advanced
    by the same formula. The host decides which rows are active, so the
    mirror is always exact, and capacity is checked on it before any launch.

    ``max_tokens`` is per sequence. attend() takes one query row per
    sequence; a speculative verify step takes up to 16 draft tokens per
    sequence, as a chain (append_many, attend_many, truncate,
    graphed_step_many) or as a token tree (append_tree, attend_tree, commit,
    graphed_step_tree). No MX
    cache (its 64-token quantization windows are host-side state per
    sequence).

    Where a local position lives is the subclass seam: the methods under
    "storage" below are all that PagedDecodeSession replaces.
    """

    def __init__(
        self,
        batch: int,
        kv_heads: int,
        head_dim: int,
        max_tokens: int,
        device: torch.device | str = "cuda",
        kv_dtype: str | torch.dtype = "bf16",
        block: int = 256,
        group: dist.ProcessGroup | None = None,
    ) -> None:
        td, local_cap = self._setup(batch, max_tokens, device, kv_dtype,
                                    block, group)
        self.k = torch.empty(batch, kv_heads, local_cap, head_dim, dtype=td,
                             device=self.device)
        self.v = torch.empty_like(self.k)

    def _setup(self, batch, max_tokens, device, kv_dtype, block, group):
        """Everything but the KV storage: rank and world, the lengths on
        host and device. Returns (storage dtype, positions per row that
        max_tokens asks of this rank's shard)."""
        name = type(self).__name__
        if isinstance(kv_dtype, str) and kv_dtype in ("mx", "fp8_mx"):
            raise ValueError(
                f"{name}: the MX cache keeps host-side window "
                "state per sequence and is not supported; use bf16, fp16, "
                "fp32 or fp8")
        if isinstance(kv_dtype, str) and kv_dtype not in _DTYPES:
            raise ValueError(f"{name}: unknown kv_dtype "
                             f"{kv_dtype!r}")
        self.device = torch.device(device)
        self.rank, self.world = _rank_world(group)
        self.group = group
        self.block = block
        self.batch = batch
        td = _DTYPES[kv_dtype] if isinstance(kv_dtype, str) else kv_dtype
        self.total_dev = torch.zeros(batch, dtype=torch.long,
                                     device=self.device)
        self.local_len_dev = torch.zeros_like(self.total_dev)
        self.totals = [0] * batch       # global tokens of each sequence
        self.local_lens = [0] * batch   # of them, in THIS rank's shard
        self._mask_cache: dict[tuple, torch.Tensor] = {}
        # multi-token verify: (B, T) visible lengths per T (static buffers:
        # a captured graph reads them), the device copies of counts seen,
        # and (T, host vis, totals) after the last append_many: stale once
        # the totals have moved on
        self._vis_bufs: dict[int, torch.Tensor] = {}
        self._counts_cache: dict[tuple, torch.Tensor] = {}
        self._spec: tuple[int, list[list[int]], tuple] | None = None
        # tree-shaped drafts: (base (B,) int64, mask (B, T) int32) static
        # buffers per T, and the pending tree of the last append_tree (its
        # cast drafts, counts, parents, the totals before and after). Every
        # method that moves a length drops it; the totals are compared as
        # well, as for _spec
        self._tree_bufs: dict[int, tuple[torch.Tensor, torch.Tensor]] = {}
        self._tree: dict | None = None
        return td, _local_cap(max_tokens, block, self.world)

    # ---- storage: a (B, Hkv, capacity, D) slab ----
    _graph_refusal = (
        "graphed_step: the zero-copy cache kernel does not take this "
        "session (needs head_dim 128, a bf16/fp16 query, a cache of "
        "the query's dtype or fp8 under bf16, and Hq/Hkv <= 16)")

    @property
    def _kv(self) -> torch.Tensor:
        """The K storage: its dtype, head count and head_dim are the
        session's."""
        return self.k

    @property
    def capacity(self) -> int:
        return self.k.size(2)

    def _reserve(self, ends: dict[int, int]) -> None:
        """ends[b]: local positions row b is about to hold. The slab holds
        every position up to capacity already."""

    def _store(self, b: int, pos: int, k_rows: torch.Tensor,
               v_rows: torch.Tensor) -> None:
        """Host store of (Hkv, n, D) rows of sequence b at local positions
        [pos, pos + n), cast to the storage dtype."""
        n = k_rows.shape[1]
        self.k[b, :, pos : pos + n] = k_rows.to(self.k.dtype)
        self.v[b, :, pos : pos + n] = v_rows.to(self.v.dtype)

    def _rows(self, b: int, n: int):
        """Row b's first n local positions as contiguous (1, Hkv, n, D) K
        and V."""
        return (self.k[b : b + 1, :, :n].contiguous(),
                self.v[b : b + 1, :, :n].contiguous())

    def _fallback_rows(self, q: torch.Tensor, b: int, n: int):
        """_rows as local_attention takes them under query q."""
        return self._rows(b, n)

    def _launch_append(self, ext, k_new, v_new, active_dev) -> None:
        # the cast to the cache dtype (fp8 included) stays a torch op; the
        # kernel copies bytes
        ext.kv_cache_append(
            self.k, self.v, k_new.to(self.k.dtype).contiguous(),
            v_new.to(self.v.dtype).contiguous(), self.total_dev,
            self.local_len_dev, active_dev, self.block, self.rank,
            self.world)

    def _launch_attend(self, ext, q, scale: float):
        # one launch for the whole ragged batch: every block clips its
        # chunk to its own row's length, read from local_len_dev
        return ext.flash_attention_cache(q.contiguous(), self.k, self.v,
                                         self.local_len_dev, scale)

    def _launch_append_n(self, ext, k_new, v_new, counts_dev, vis_dev) -> None:
        ext.kv_cache_append_n(
            self.k, self.v, k_new.to(self.k.dtype).contiguous(),
            v_new.to(self.v.dtype).contiguous(), self.total_dev,
            self.local_len_dev, counts_dev, vis_dev, self.block, self.rank,
            self.world)

    def _launch_attend_many(self, ext, q, scale: float, vis_dev):
        return ext.flash_attention_cache_qlen(
            q.contiguous(), self.k, self.v, self.local_len_dev, vis_dev,
            scale)

    def _launch_append_tree(self, ext, k_new, v_new, counts_dev, parents_dev,
                            base_dev, mask_dev) -> None:
        # k_new / v_new arrive cast and contiguous (_cast_new)
        ext.kv_cache_append_tree(
            self.k, self.v, k_new, v_new, self.total_dev, self.local_len_dev,
            counts_dev, parents_dev, base_dev, mask_dev, self.block,
            self.rank, self.world)

    def _launch_attend_tree(self, ext, q, scale: float, base_dev, mask_dev):
        return ext.flash_attention_cache_tree(
            q.contiguous(), self.k, self.v, self.local_len_dev, base_dev,
            mask_dev, scale)

    def _launch_commit(self, ext, k_new, v_new, counts_dev, path_dev,
                       lens_dev) -> None:
        ext.kv_cache_commit_path(
            self.k, self.v, k_new, v_new, self.total_dev, self.local_len_dev,
            counts_dev, path_dev, lens_dev, self.block, self.rank,
            self.world)

    def _release(self, b: int) -> None:
        """Row b's local length shrank: give back what it no longer needs.
        The slab keeps every position."""

    def _share(self, src: int, dst: int, n_local: int) -> None:
        """Row dst (empty) comes to hold row src's first n_local local
        positions. The slab shares nothing: a device copy of the rows."""
        if n_local:
            self.k[dst, :, :n_local].copy_(self.k[src, :, :n_local])
            self.v[dst, :, :n_local].copy_(self.v[src, :, :n_local])

    # ---- host mirror ----
    def _mask(self, active) -> list[bool]:
        if active is None:
            return [True] * self.batch
        if isinstance(active, torch.Tensor):
            active = active.tolist()
        mask = [bool(a) for a in active]
        if len(mask) != self.batch:
            raise ValueError(f"active has {len(mask)} entries for a batch of "
                             f"{self.batch}")
        return mask

    def _mask_dev(self, mask: list[bool]) -> torch.Tensor:
        """The mask as a (B,) uint8 device tensor. Masks seen before come
        from a small cache: a host-to-device copy from pageable memory makes
        the host wait for the stream, once per step, which is what a
        launch-bound decode step cannot afford."""
        key = tuple(mask)
        dev = self._mask_cache.get(key)
        if dev is None:
            if len(self._mask_cache) >= 256:
                self._mask_cache.clear()
            dev = torch.tensor(mask, dtype=torch.uint8).to(self.device)
            self._mask_cache[key] = dev
        return dev

    def _step_ends(self, mask: list[bool]) -> dict[int, int]:
        """Capacity check of one append step, naming the row, before
        anything is reserved, launched or stored; then the rows this rank
        stores a token for -> the local positions they will hold."""
        ends, cap = {}, self.capacity
        for b, on in enumerate(mask):
            if not on:
                continue
            owner, pos = _place(self.totals[b], self.block, self.world)
            if owner != self.rank:
                continue
            if pos >= cap:
                raise RuntimeError(
                    f"{type(self).__name__} capacity exceeded: row {b} local "
                    f"shard full at {self.local_lens[b]} tokens (grow "
                    f"max_tokens)")
            ends[b] = pos + 1
        return ends

    def _advance(self, mask: list[bool]) -> None:
        for b, on in enumerate(mask):
            if not on:
                continue
            owner, pos = _place(self.totals[b], self.block, self.world)
            if owner == self.rank:
                self.local_lens[b] = pos + 1
            self.totals[b] += 1

    def _push_lengths(self, b: int) -> None:
        self.total_dev[b : b + 1].fill_(self.totals[b])
        self.local_len_dev[b : b + 1].fill_(self.local_lens[b])

    def _append_kernel_ok(self) -> bool:
        row_bytes = self._kv.size(3) * self._kv.element_size()
        return self.device.type == "cuda" and row_bytes % 4 == 0

    @classmethod
    def _ext(cls):
        from .ops.flash import _load_extension

        ext = _load_extension()
        if ext is None:
            raise RuntimeError(
                f"{cls.__name__}: the gfx950 HIP extension "
                "_tree_attn_hip is not built but the session is on a GPU")
        return ext

    # ---- cache updates ----
    def prefill(self, b: int, k_seq: torch.Tensor, v_seq: torch.Tensor) -> None:
        """Bulk-load the prompt of sequence b, (Hkv, T, D) or (1, Hkv, T, D),
        behind what it already holds; chunks split at that sequence's own
        block boundaries (DecodeSession.prefill's ownership rule)."""
        if k_seq.dim() == 4:
            k_seq, v_seq = k_seq[0], v_seq[0]
        t_total = k_seq.shape[1]
        chunks = []   # (source offset, n, local position) of the owned ones
        total, t = self.totals[b], 0
        while t < t_total:
            n = min(self.block - total % self.block, t_total - t)
            owner, pos = _place(total, self.block, self.world)
            if owner == self.rank:
                if pos + n > self.capacity:
                    raise RuntimeError(
                        f"{type(self).__name__} capacity exceeded during "
                        f"prefill: row {b} at {pos}+{n} tokens (grow "
                        f"max_tokens)")
                chunks.append((t, n, pos))
            total += n
            t += n
        if chunks:
            self._reserve({b: max(pos + n for _, n, pos in chunks)})
        self._tree = None
        for t, n, pos in chunks:
            self._store(b, pos, k_seq[:, t : t + n], v_seq[:, t : t + n])
            self.local_lens[b] = pos + n
        self.totals[b] = total
        self._push_lengths(b)

    def append(self, k_new: torch.Tensor, v_new: torch.Tensor,
               active=None) -> None:
        """Append one token's K/V (B, Hkv, 1, D) to every ACTIVE sequence
        (host bool sequence or CPU tensor of length B; None: all). Every
        rank calls this with the same arguments; only a token's owning rank
        stores it."""
        mask = self._mask(active)
        ends = self._step_ends(mask)
        self._reserve(ends)
        self._tree = None
        if self._append_kernel_ok():
            self._launch_append(self._ext(), k_new, v_new,
                                self._mask_dev(mask))
            self._advance(mask)
            return
        for b, end in ends.items():
            self._store(b, end - 1, k_new[b], v_new[b])
        self._advance(mask)
        self.total_dev.copy_(torch.tensor(self.totals, dtype=torch.long))
        self.local_len_dev.copy_(torch.tensor(self.local_lens,
                                              dtype=torch.long))

    def reset(self, b: int) -> None:
        """Free slot b for a new sequence: its lengths go to 0 on host and
        device; nothing is cleared."""
        self._tree = None
        self.totals[b] = 0
        self.local_lens[b] = 0
        self._push_lengths(b)

    def fork(self, src: int, dst: int, tokens: int | None = None) -> None:
        """Slot dst becomes a sequence holding the first ``tokens`` global
        tokens of sequence src (None: all of them); whatever dst held is
        dropped as by reset(dst). Every rank calls this with the same
        arguments. A paged session shares src's pages by reference and copies
        a shared tail page before the first write into it; the slab copies
        the rows. The lengths go to the device, so a step captured before
        the fork replays correctly after it."""
        for name, slot in (("src", src), ("dst", dst)):
            if not 0 <= slot < self.batch:
                raise ValueError(f"fork: {name} = {slot} is outside "
                                 f"[0, {self.batch})")
        if src == dst:
            raise ValueError(f"fork: src and dst are both row {src}")
        if tokens is None:
            tokens = self.totals[src]
        if not 0 <= tokens <= self.totals[src]:
            raise ValueError(
                f"fork: row {src} holds {self.totals[src]} tokens, cannot "
                f"fork its first {tokens}")
        self.reset(dst)
        self._spec = None
        n_local = _n_local(tokens, self.block, self.rank, self.world)
        self._share(src, dst, n_local)
        self.totals[dst] = tokens
        self.local_lens[dst] = n_local
        self._push_lengths(dst)

    # ---- multi-token verify step: cache updates ----
    def _counts(self, counts, t: int) -> list[int]:
        if counts is None:
            return [t] * self.batch
        if isinstance(counts, torch.Tensor):
            counts = counts.tolist()
        counts = [int(c) for c in counts]
        if len(counts) != self.batch:
            raise ValueError(f"counts has {len(counts)} entries for a batch "
                             f"of {self.batch}")
        for b, c in enumerate(counts):
            if not 0 <= c <= t:
                raise ValueError(f"counts[{b}] = {c} is outside [0, {t}]")
        return counts

    def _counts_dev(self, counts: list[int]) -> torch.Tensor:
        """counts as a (B,) int32 device tensor, from a small cache
        (_mask_dev)."""
        key = tuple(counts)
        dev = self._counts_cache.get(key)
        if dev is None:
            if len(self._counts_cache) >= 256:
                self._counts_cache.clear()
            dev = torch.tensor(counts, dtype=torch.int32).to(self.device)
            self._counts_cache[key] = dev
        return dev

    def _vis_dev(self, t: int) -> torch.Tensor:
        """The (B, t) int64 device buffer of visible lengths: one per t, so
        a captured graph and the eager calls share it."""
        buf = self._vis_bufs.get(t)
        if buf is None:
            buf = torch.zeros(self.batch, t, dtype=torch.long,
                              device=self.device)
            self._vis_bufs[t] = buf
        return buf

    def _check_many(self, k_new: torch.Tensor, v_new: torch.Tensor,
                    who: str = "append_many") -> int:
        kv = self._kv
        if (k_new.dim() != 4 or k_new.shape != v_new.shape
                or k_new.shape[0] != self.batch
                or k_new.shape[1] != kv.size(1)
                or k_new.shape[3] != kv.size(3)
                or not 1 <= k_new.shape[2] <= 16):
            raise ValueError(
                f"{who}: k_new / v_new must be (B, Hkv, T, D) = "
                f"({self.batch}, {kv.size(1)}, T, {kv.size(3)}) with T in "
                f"1..16, got {tuple(k_new.shape)} / {tuple(v_new.shape)}")
        return k_new.shape[2]

    def _many_ends(self, counts: list[int]) -> dict[int, int]:
        """_step_ends for counts[b] tokens per row: the capacity check, then
        the rows whose shard grows -> the local positions they will hold."""
        ends, cap = {}, self.capacity
        for b, c in enumerate(counts):
            end = _n_local(self.totals[b] + c, self.block, self.rank,
                           self.world)
            if end == self.local_lens[b]:
                continue
            if end > cap:
                raise RuntimeError(
                    f"{type(self).__name__} capacity exceeded: row {b} local "
                    f"shard full at {self.local_lens[b]} tokens (grow "
                    f"max_tokens)")
            ends[b] = end
        return ends

    def _advance_many(self, counts: list[int], t: int) -> None:
        """The mirror after counts[b] of t tokens per row, and the visible
        lengths kv_append_n_kernel leaves: query i of row b sees the tokens
        before this step and drafts 0..min(i, counts[b] - 1)."""
        vis = []
        for b, c in enumerate(counts):
            t0 = self.totals[b]
            vis.append([
                _n_local(t0 + (min(i, c - 1) + 1 if c else 0), self.block,
                         self.rank, self.world) for i in range(t)])
            if c:
                self.local_lens[b] = _n_local(t0 + c, self.block, self.rank,
                                              self.world)
            self.totals[b] = t0 + c
        self._spec = (t, vis, tuple(self.totals))

    def append_many(self, k_new: torch.Tensor, v_new: torch.Tensor,
                    counts=None) -> None:
        """Append up to T draft tokens per sequence, (B, Hkv, T, D): row b
        takes its first counts[b] (host ints in [0, T]; None: T for every
        row). Every rank calls this with the same arguments; only a token's
        owning rank stores it. attend_many() then verifies the drafts and
        truncate() takes the rejected ones back out."""
        t = self._check_many(k_new, v_new)
        counts = self._counts(counts, t)
        self._reserve(self._many_ends(counts))
        self._tree = None
        vis_dev = self._vis_dev(t)
        if self._append_kernel_ok():
            self._launch_append_n(self._ext(), k_new, v_new,
                                  self._counts_dev(counts), vis_dev)
            self._advance_many(counts, t)
            return
        for b, c in enumerate(counts):
            for i in range(c):
                owner, pos = _place(self.totals[b] + i, self.block,
                                    self.world)
                if owner == self.rank:
                    self._store(b, pos, k_new[b, :, i : i + 1],
                                v_new[b, :, i : i + 1])
        self._advance_many(counts, t)
        self.total_dev.copy_(torch.tensor(self.totals, dtype=torch.long))
        self.local_len_dev.copy_(torch.tensor(self.local_lens,
                                              dtype=torch.long))
        vis_dev.copy_(torch.tensor(self._spec[1], dtype=torch.long))

    def truncate(self, b: int, total: int) -> None:
        """Cut sequence b back to its first `total` tokens (the rejected
        drafts of a verify step): lengths on host and device; nothing is
        cleared. A paged session hands back the pages past the new length."""
        if not 0 <= total <= self.totals[b]:
            raise ValueError(
                f"truncate: row {b} holds {self.totals[b]} tokens, cannot "
                f"cut to {total}")
        self._tree = None
        self.totals[b] = total
        self.local_lens[b] = _n_local(total, self.block, self.rank,
                                      self.world)
        self._push_lengths(b)
        self._release(b)

    # ---- tree-shaped drafts: append, verify, keep the accepted path ----
    def _tree_dev(self, t: int) -> tuple[torch.Tensor, torch.Tensor]:
        """The (B,) int64 base and (B, t) int32 mask device buffers: one
        pair per t, so a captured graph and the eager calls share them
        (_vis_dev)."""
        bufs = self._tree_bufs.get(t)
        if bufs is None:
            bufs = (torch.zeros(self.batch, dtype=torch.long,
                                device=self.device),
                    torch.zeros(self.batch, t, dtype=torch.int32,
                                device=self.device))
            self._tree_bufs[t] = bufs
        return bufs

    def _cast_new(self, k_new: torch.Tensor, v_new: torch.Tensor):
        """The drafts as the cache stores them: what the append and the
        commit kernels copy from."""
        dtype = self._kv.dtype
        return k_new.to(dtype).contiguous(), v_new.to(dtype).contiguous()

    def _node_table(self, who: str, name: str, table, t: int, check,
                    pad: int = -1) -> tuple[torch.Tensor, list | None]:
        """`table` (parents or paths) as a (B, t) int32 device tensor plus
        its host rows when it came as a nested list; a list is validated row
        by row with check(b, row) and padded to t with `pad`."""
        if isinstance(table, torch.Tensor):
            if (table.dtype != torch.int32
                    or table.device != self.total_dev.device
                    or tuple(table.shape) != (self.batch, t)):
                raise ValueError(
                    f"{who}: {name} must be a (B, T) = ({self.batch}, {t}) "
                    f"int32 tensor on {self.device}, got "
                    f"{tuple(table.shape)} {table.dtype} on {table.device}")
            return table.contiguous(), None
        rows = [[int(p) for p in row] for row in table]
        if len(rows) != self.batch:
            raise ValueError(f"{who}: {name} has {len(rows)} rows for a "
                             f"batch of {self.batch}")
        for b, row in enumerate(rows):
            if len(row) > t:
                raise ValueError(f"{who}: {name}[{b}] has {len(row)} entries "
                                 f"for T = {t}")
            check(b, row)
        host = [row + [pad] * (t - len(row)) for row in rows]
        dev = torch.tensor(host, dtype=torch.int32).to(self.device)
        return dev, host

    def _fresh_tree(self, who: str) -> dict:
        tree = self._tree
        if tree is None or tree["totals"] != tuple(self.totals):
            raise RuntimeError(
                f"{who}: no append_tree since the lengths last moved")
        return tree

    def _tree_parents(self, tree: dict) -> list[list[int]]:
        if tree["parents"] is None:
            tree["parents"] = tree["parents_dev"].tolist()
        return tree["parents"]

    def _advance_tree(self, counts: list[int], t: int, k_c, v_c,
                      parents_dev, parents_host) -> None:
        t0 = list(self.totals)
        self._advance_many(counts, t)
        self._spec = None
        self._tree = {"t": t, "k": k_c, "v": v_c, "counts": counts, "t0": t0,
                      "totals": tuple(self.totals),
                      "parents_dev": parents_dev, "parents": parents_host}

    def append_tree(self, k_new: torch.Tensor, v_new: torch.Tensor, parents,
                    counts=None) -> None:
        """Append up to T draft NODES of a token tree per sequence, (B, Hkv,
        T, D) in topological order: row b takes its first counts[b] (host
        ints; None: T). ``parents`` is a (B, T) int32 tensor on the
        session's device (a sampler's output goes straight through, no host
        copy) or a nested list, which is validated; parents[b][j] in [-1, j
        - 1] is node j's parent, -1 the last committed token. attend_tree()
        then verifies every node against its own ancestors and commit()
        keeps the accepted root-to-node path."""
        t = self._check_many(k_new, v_new, "append_tree")
        counts = self._counts(counts, t)

        def check(b, row):
            if len(row) < counts[b]:
                raise ValueError(
                    f"append_tree: parents[{b}] has {len(row)} entries for "
                    f"counts[{b}] = {counts[b]}")
            for j, p in enumerate(row):
                if not -1 <= p < j:
                    raise ValueError(
                        f"append_tree: parents[{b}][{j}] = {p} is outside "
                        f"[-1, {j - 1}] (row {b})")

        parents_dev, parents_host = self._node_table(
            "append_tree", "parents", parents, t, check)
        self._reserve(self._many_ends(counts))
        k_c, v_c = self._cast_new(k_new, v_new)
        base_dev, mask_dev = self._tree_dev(t)
        if self._append_kernel_ok():
            self._launch_append_tree(self._ext(), k_c, v_c,
                                     self._counts_dev(counts), parents_dev,
                                     base_dev, mask_dev)
            self._advance_tree(counts, t, k_c, v_c, parents_dev,
                               parents_host)
            return
        for b, c in enumerate(counts):
            for i in range(c):
                owner, pos = _place(self.totals[b] + i, self.block,
                                    self.world)
                if owner == self.rank:
                    self._store(b, pos, k_c[b, :, i : i + 1],
                                v_c[b, :, i : i + 1])
        self._advance_tree(counts, t, k_c, v_c, parents_dev, parents_host)
        self.total_dev.copy_(torch.tensor(self.totals, dtype=torch.long))
        self.local_len_dev.copy_(torch.tensor(self.local_lens,
                                              dtype=torch.long))
        bases, masks = self._tree_host(self._tree)
        base_dev.copy_(torch.tensor(bases, dtype=torch.long))
        mask_dev.copy_(torch.tensor(masks, dtype=torch.int32))

    def _tree_host(self, tree: dict):
        """(bases, masks) of the pending tree on the host: _tree_masks per
        row."""
        parents = self._tree_parents(tree)
        rows = [_tree_masks(tree["t0"][b], c, parents[b], tree["t"],
                            self.block, self.rank, self.world)
                for b, c in enumerate(tree["counts"])]
        return [r[0] for r in rows], [r[1] for r in rows]

    def _local_partial_tree(self, q: torch.Tensor, tree: dict,
                            softmax_scale: float | None):
        t = tree["t"]
        if _zero_copy_ok(q, self._kv, any_tq=True):
            base_dev, mask_dev = self._tree_dev(t)
            return self._launch_attend_tree(
                self._ext(), q, _scale(softmax_scale, q), base_dev, mask_dev)
        # per row and per run of query positions with one mask: gather the
        # visible local rows (the prefix plus the owned ancestors)
        bases, masks = self._tree_host(tree)
        outs, lses = [], []
        for b in range(self.batch):
            base, row_o, row_l, i = bases[b], [], [], 0
            while i < t:
                m, j = masks[b][i], i + 1
                while j < t and masks[b][j] == m:
                    j += 1
                qb = q[b : b + 1, :, i:j]
                slots = [s for s in range(16) if (m >> s) & 1]
                n = base + len(slots)
                if n > 0:
                    last = base + slots[-1] + 1 if slots else base
                    k, v = self._fallback_rows(qb, b, last)
                    if slots != list(range(len(slots))):
                        idx = torch.tensor(
                            list(range(base)) + [base + s for s in slots],
                            dtype=torch.long, device=k.device)
                        k = k.index_select(2, idx)
                        v = v.index_select(2, idx)
                    if q.device.type == "cuda" and k.dtype == torch.float32:
                        # the GPU kernels take no fp32 K/V
                        k, v = k.to(q.dtype), v.to(q.dtype)
                    o, l = local_attention(qb, k, v, softmax_scale)
                else:
                    o, l = _empty_partial(qb)
                row_o.append(o)
                row_l.append(l)
                i = j
            outs.append(torch.cat(row_o, dim=2))
            lses.append(torch.cat(row_l, dim=2))
        return torch.cat(outs), torch.cat(lses)

    def attend_tree(self, q: torch.Tensor, softmax_scale: float | None = None,
                    combine: str = "auto") -> torch.Tensor:
        """Verify the nodes of the last append_tree: q (B, Hq, T, D) -> (B,
        Hq, T, D). Query i < counts[b] of sequence b attends the tokens b
        held before that append plus node i and its ancestors, never a
        sibling; a query at or past counts[b] only the tokens before the
        append. A row with nothing to see yields zeros."""
        tree = self._fresh_tree("attend_tree")
        t = tree["t"]
        if q.dim() != 4 or q.shape[0] != self.batch or q.shape[2] != t:
            raise ValueError(
                f"attend_tree: q must be (B, Hq, T, D) with B = {self.batch} "
                f"and the T = {t} of the last append_tree, got "
                f"{tuple(q.shape)}")
        out_l, lse_l = self._local_partial_tree(q, tree, softmax_scale)
        out, _ = tree_combine(out_l, lse_l, strategy=combine, group=self.group)
        return out

    def commit(self, paths, lens) -> None:
        """Keep, per sequence, the accepted root-to-node path of the last
        append_tree and drop the other drafts: nodes paths[b][:lens[b]]
        become the sequence's next lens[b] tokens. ``paths`` is a (B, T)
        int32 device tensor or a nested list, which is checked against the
        parents to be a path from a root; ``lens`` are host ints in [0,
        counts[b]] (0 rejects every draft), so the host mirror stays exact.
        A paged session hands back the pages past the new lengths."""
        tree = self._fresh_tree("commit")
        t, counts = tree["t"], tree["counts"]
        if isinstance(lens, torch.Tensor):
            lens = lens.tolist()
        lens = [int(n) for n in lens]
        if len(lens) != self.batch:
            raise ValueError(f"commit: lens has {len(lens)} entries for a "
                             f"batch of {self.batch}")
        for b, n in enumerate(lens):
            if not 0 <= n <= counts[b]:
                raise ValueError(f"commit: lens[{b}] = {n} is outside "
                                 f"[0, {counts[b]}] (row {b})")

        def check(b, row):
            if len(row) < lens[b]:
                raise ValueError(f"commit: paths[{b}] has {len(row)} entries "
                                 f"for lens[{b}] = {lens[b]}")
            parents, prev = self._tree_parents(tree)[b], -1
            for i, node in enumerate(row[: lens[b]]):
                if not 0 <= node < counts[b] or parents[node] != prev:
                    raise ValueError(
                        f"commit: paths[{b}][{i}] = {node} does not continue "
                        f"a path from the root of row {b}'s tree")
                prev = node

        path_dev, path_host = self._node_table("commit", "paths", paths, t,
                                               check, pad=0)
        # no copy-on-write here: the positions re-stored are ones the
        # preceding append_tree wrote, so its _reserve made their pages
        # exclusive, and fork() drops the pending tree
        if self._append_kernel_ok():
            self._launch_commit(self._ext(), tree["k"], tree["v"],
                                self._counts_dev(counts), path_dev,
                                self._counts_dev(lens))
        else:
            if path_host is None:
                path_host = path_dev.tolist()
            for b, n in enumerate(lens):
                for i in range(n):
                    src = min(max(path_host[b][i], 0), t - 1)
                    owner, pos = _place(tree["t0"][b] + i, self.block,
                                        self.world)
                    if owner == self.rank:
                        self._store(b, pos, tree["k"][b, :, src : src + 1],
                                    tree["v"][b, :, src : src + 1])
        for b, n in enumerate(lens):
            self.totals[b] = tree["t0"][b] + n
            self.local_lens[b] = _n_local(self.totals[b], self.block,
                                          self.rank, self.world)
        if not self._append_kernel_ok():
            self.total_dev.copy_(torch.tensor(self.totals, dtype=torch.long))
            self.local_len_dev.copy_(torch.tensor(self.local_lens,
                                                  dtype=torch.long))
        for b in range(self.batch):
            self._release(b)
        self._tree = None

    # ---- attention ----
    def _local_partial(self, q: torch.Tensor, softmax_scale: float | None):
        if _zero_copy_ok(q, self._kv):
            return self._launch_attend(self._ext(), q,
                                       _scale(softmax_scale, q))
        outs, lses = [], []
        for b, n in enumerate(self.local_lens):
            qb = q[b : b + 1]
            if n > 0:
                k, v = self._fallback_rows(qb, b, n)
                o, l = local_attention(qb, k, v, softmax_scale)
            else:
                o, l = _empty_partial(qb)
            outs.append(o)
            lses.append(l)
        return torch.cat(outs), torch.cat(lses)

    def _check_shared(self, q: torch.Tensor) -> None:
        """Whether this session takes shared=True under query q."""
        raise ValueError(
            f"{type(self).__name__}: shared=True needs a PagedDecodeSession; "
            "the slab shares nothing between rows")

    def _local_partial_shared(self, q: torch.Tensor,
                              softmax_scale: float | None):
        self._check_shared(q)

    def attend(self, q: torch.Tensor, softmax_scale: float | None = None,
               combine: str = "auto", shared: bool = False) -> torch.Tensor:
        """Attention of q (B, Hq, 1, D), row b over sequence b's cached
        tokens -> (B, Hq, 1, D). A sequence that holds no token yields an
        all-zero row. ``shared`` (PagedDecodeSession only): rows that hold
        the same leading full pages attend them in one KV stream per group
        (shared_plan) and their remainders on their own; same result."""
        if shared:
            out_l, lse_l = self._local_partial_shared(q, softmax_scale)
        else:
            out_l, lse_l = self._local_partial(q, softmax_scale)
        out, _ = tree_combine(out_l, lse_l, strategy=combine, group=self.group)
        return out

    def _local_partial_many(self, q: torch.Tensor, vis: list[list[int]],
                            softmax_scale: float | None):
        if _zero_copy_ok(q, self._kv, any_tq=True):
            return self._launch_attend_many(
                self._ext(), q, _scale(softmax_scale, q),
                self._vis_dev(q.shape[2]))
        # per row and per run of query positions with one visible length
        t = q.shape[2]
        outs, lses = [], []
        for b in range(self.batch):
            row_o, row_l, i = [], [], 0
            while i < t:
                n, j = vis[b][i], i + 1
                while j < t and vis[b][j] == n:
                    j += 1
                qb = q[b : b + 1, :, i:j]
                if n > 0:
                    k, v = self._fallback_rows(qb, b, n)
                    if q.device.type == "cuda" and k.dtype == torch.float32:
                        # the GPU kernels take no fp32 K/V
                        k, v = k.to(q.dtype), v.to(q.dtype)
                    o, l = local_attention(qb, k, v, softmax_scale)
                else:
                    o, l = _empty_partial(qb)
                row_o.append(o)
                row_l.append(l)
                i = j
            outs.append(torch.cat(row_o, dim=2))
            lses.append(torch.cat(row_l, dim=2))
        return torch.cat(outs), torch.cat(lses)

    def attend_many(self, q: torch.Tensor,
                    softmax_scale: float | None = None,
                    combine: str = "auto") -> torch.Tensor:
        """Verify the drafts of the last append_many: q (B, Hq, T, D) ->
        (B, Hq, T, D). Query i of sequence b attends the tokens b held
        before that append plus drafts 0..min(i, counts[b] - 1): rows at or
        past counts[b] see what the last draft sees, a row with count 0 the
        whole sequence. A sequence that holds no token yields zeros."""
        spec = self._spec
        if spec is None or spec[2] != tuple(self.totals):
            raise RuntimeError(
                "attend_many: no append_many since the lengths last moved")
        t, vis, _ = spec
        if q.dim() != 4 or q.shape[0] != self.batch or q.shape[2] != t:
            raise ValueError(
                f"attend_many: q must be (B, Hq, T, D) with B = {self.batch} "
                f"and the T = {t} of the last append_many, got "
                f"{tuple(q.shape)}")
        out_l, lse_l = self._local_partial_many(q, vis, softmax_scale)
        out, _ = tree_combine(out_l, lse_l, strategy=combine, group=self.group)
        return out

    def graphed_step(self, q_static: torch.Tensor, k_static: torch.Tensor,
                     v_static: torch.Tensor,
                     softmax_scale: float | None = None,
                     combine: str = "auto", shared: bool = False):
        """Capture one decode step — append kernel, cache kernel, split
        combine, one linear chain — into a hipGraph. Returns ``replay``.
        ``shared`` (PagedDecodeSession only): the chain is append kernel,
        prefix pass, suffix pass, combine (attend(shared=True)); replay()
        brings the device copy of shared_plan() up to date first, so a fork,
        reset or truncate after the capture replays correctly.

        Write the step's query and new K/V (B, Hkv, 1, D) into the static
        tensors, then ``replay(active=None)`` checks capacity on the host
        mirror, reserves what the step will hold (a paged session assigns
        its new pages here, eagerly: the page table is a static buffer, so
        the replay sees the new entries), advances the mirror, copies the
        mask into the static device buffer the capture reads, replays, and
        returns the output: the static buffer at world size 1; at world
        size > 1 the local partial replays from the graph and the collective
        runs eagerly (graphed_attend).
        """
        if shared:
            self._check_shared(q_static)
        if self.device.type != "cuda":
            raise ValueError("graphed_step needs a GPU session")
        # never capture the per-row fallback: it would freeze the
        # capture-time lengths (and pages) into every replay
        if not _zero_copy_ok(q_static, self._kv):
            raise ValueError(self._graph_refusal)
        if not self._append_kernel_ok():
            raise ValueError("graphed_step: the append kernel needs cache "
                             "rows of a multiple of 4 bytes")
        ext = self._ext()
        active_dev = torch.zeros(self.batch, dtype=torch.uint8,
                                 device=self.device)
        scale = _scale(softmax_scale, q_static)
        hq = q_static.shape[1]
        # static buffers: the capture reads them, replay() refreshes them
        tables = self._shared_tables(hq) if shared else None

        def step():
            self._launch_append(ext, k_static, v_static, active_dev)
            if shared:
                return self._launch_attend_shared(ext, q_static, scale,
                                                  tables)
            return self._launch_attend(ext, q_static, scale)

        # the warm-up runs under the all-zero mask, so no length moves
        graph, (out_l, lse_l) = _capture(step)
        self._graph = graph  # keep alive
        self._active_dev = active_dev

        in_buffer = [[False] * self.batch]   # what active_dev holds now

        def replay(active=None) -> torch.Tensor:
            mask = self._mask(active)
            self._reserve(self._step_ends(mask))
            self._tree = None
            self._advance(mask)
            if mask != in_buffer[0]:   # a steady mask costs no copy at all
                active_dev.copy_(self._mask_dev(mask))
                in_buffer[0] = mask
            if shared:   # the plan of the lengths the step will leave
                self._shared_tables(hq)
            graph.replay()
            if self.world == 1:
                return out_l
            out, _ = tree_combine(out_l, lse_l, strategy=combine,
                                  group=self.group)
            return out

        return replay

    def graphed_step_many(self, q_static: torch.Tensor,
                          k_static: torch.Tensor, v_static: torch.Tensor,
                          softmax_scale: float | None = None,
                          combine: str = "auto"):
        """graphed_step for a verify step of T tokens per row: the
        multi-token append kernel, the visible-length cache kernel(s) and
        the split combine, one linear chain, captured under an all-zero
        ``counts``. Returns ``replay``.

        Write the queries (B, Hq, T, D) and the drafts' K/V (B, Hkv, T, D)
        into the static tensors, then ``replay(counts=None)`` checks
        capacity on the host mirror, reserves, advances the mirror, copies
        ``counts`` into the static device buffer when they changed, replays
        and returns the output as graphed_step does. truncate() between
        replays is legal: the lengths are device buffers the replay reads.
        """
        if self.device.type != "cuda":
            raise ValueError("graphed_step needs a GPU session")
        if not _zero_copy_ok(q_static, self._kv, any_tq=True):
            raise ValueError(self._graph_refusal)
        if not self._append_kernel_ok():
            raise ValueError("graphed_step: the append kernel needs cache "
                             "rows of a multiple of 4 bytes")
        t = self._check_many(k_static, v_static)
        if q_static.dim() != 4 or q_static.shape[0] != self.batch or \
                q_static.shape[2] != t:
            raise ValueError(
                f"graphed_step_many: q_static must be (B, Hq, T, D) with "
                f"B = {self.batch} and the T = {t} of k_static, got "
                f"{tuple(q_static.shape)}")
        ext = self._ext()
        counts_dev = torch.zeros(self.batch, dtype=torch.int32,
                                 device=self.device)
        vis_dev = self._vis_dev(t)
        scale = _scale(softmax_scale, q_static)

        def step():
            self._launch_append_n(ext, k_static, v_static, counts_dev,
                                  vis_dev)
            return self._launch_attend_many(ext, q_static, scale, vis_dev)

        # the warm-up runs under all-zero counts, so no length moves
        graph, (out_l, lse_l) = _capture(step)
        self._graph_many = graph  # keep alive
        self._counts_static = counts_dev

        in_buffer = [[0] * self.batch]   # what counts_dev holds now

        def replay(counts=None) -> torch.Tensor:
            counts = self._counts(counts, t)
            self._reserve(self._many_ends(counts))
            self._tree = None
            self._advance_many(counts, t)
            if counts != in_buffer[0]:
                counts_dev.copy_(self._counts_dev(counts))
                in_buffer[0] = counts
            graph.replay()
            if self.world == 1:
                return out_l
            out, _ = tree_combine(out_l, lse_l, strategy=combine,
                                  group=self.group)
            return out

        return replay

    def graphed_step_tree(self, q_static: torch.Tensor,
                          k_static: torch.Tensor, v_static: torch.Tensor,
                          parents_static: torch.Tensor,
                          softmax_scale: float | None = None,
                          combine: str = "auto"):
        """graphed_step_many for a tree of T draft nodes per row: the tree
        append kernel, the ancestor-mask cache kernel(s) and the split
        combine, one linear chain, captured under an all-zero ``counts``.
        Returns ``replay``.

        Write the queries (B, Hq, T, D), the nodes' K/V (B, Hkv, T, D) and
        their parents (B, T) int32 into the static tensors, then
        ``replay(counts=None)`` does what graphed_step_many's does and
        leaves the step as the pending tree. commit() after a replay is an
        eager launch and is legal between replays, as truncate() is.
        """
        if self.device.type != "cuda":
            raise ValueError("graphed_step needs a GPU session")
        if not _zero_copy_ok(q_static, self._kv, any_tq=True):
            raise ValueError(self._graph_refusal)
        if not self._append_kernel_ok():
            raise ValueError("graphed_step: the append kernel needs cache "
                             "rows of a multiple of 4 bytes")
        t = self._check_many(k_static, v_static, "graphed_step_tree")
        if q_static.dim() != 4 or q_static.shape[0] != self.batch or \
                q_static.shape[2] != t:
            raise ValueError(
                f"graphed_step_tree: q_static must be (B, Hq, T, D) with "
                f"B = {self.batch} and the T = {t} of k_static, got "
                f"{tuple(q_static.shape)}")
        if not isinstance(parents_static, torch.Tensor):
            raise ValueError("graphed_step_tree: parents_static must be a "
                             "(B, T) int32 device tensor")
        parents_dev, _ = self._node_table("graphed_step_tree",
                                          "parents_static", parents_static, t,
                                          None)
        if parents_dev is not parents_static:
            raise ValueError("graphed_step_tree: parents_static must be "
                             "contiguous")
        ext = self._ext()
        counts_dev = torch.zeros(self.batch, dtype=torch.int32,
                                 device=self.device)
        base_dev, mask_dev = self._tree_dev(t)
        scale = _scale(softmax_scale, q_static)

        def step():
            # the cast drafts are what commit() copies from after a replay
            k_c, v_c = self._cast_new(k_static, v_static)
            self._launch_append_tree(ext, k_c, v_c, counts_dev, parents_dev,
                                     base_dev, mask_dev)
            return k_c, v_c, self._launch_attend_tree(ext, q_static, scale,
                                                      base_dev, mask_dev)

        # the warm-up runs under all-zero counts, so no length moves; it
        # does rewrite the shared base / mask buffers of this T, so a tree
        # pending from an eager append_tree ends here
        self._tree = None
        graph, (k_c, v_c, (out_l, lse_l)) = _capture(step)
        self._graph_tree = graph  # keep alive
        self._counts_static_tree = counts_dev

        in_buffer = [[0] * self.batch]   # what counts_dev holds now

        def replay(counts=None) -> torch.Tensor:
            counts = self._counts(counts, t)
            self._reserve(self._many_ends(counts))
            self._advance_tree(counts, t, k_c, v_c, parents_dev, None)
            if counts != in_buffer[0]:
                counts_dev.copy_(self._counts_dev(counts))
                in_buffer[0] = counts
            graph.replay()
            if self.world == 1:
                return out_l
            out, _ = tree_combine(out_l, lse_l, strategy=combine,
                                  group=self.group)
            return out

        return replay


# --------------------------------------------------------------------------
# ragged batch over a paged pool: memory follows the live lengths
# --------------------------------------------------------------------------
_PAGE_SIZES = (128, 256, 512, 1024)


class PagedDecodeSession(RaggedDecodeSession):
    """RaggedDecodeSession over a page pool instead of a (B, Hkv, capacity,
    D) slab: same surface, same block-cyclic sharding, same lengths on host
    and device, but a sequence holds only the pages its live length needs.

    ``k_pool`` / ``v_pool`` are (n_pages, Hkv, page, D) and ``page_table``
    is (B, max_pages) int32 on the device: entry [b, j] is the physical page
    of local positions [j * page, (j + 1) * page) of sequence b on this
    rank's shard (ops/hip/ta_abi.h PageArgs). ``max_tokens`` is the
    per-sequence ceiling and fixes the table's width; ``pool_tokens`` sizes
    this rank's pool for all sequences together.

    Pages come from a host-side free list. The host mirror of the lengths is
    exact, so before each step the host knows which rows land on a new page:
    it takes the page and writes that one table entry with a stream-ordered
    device fill (no pageable host-to-device copy, no device-side
    allocation). reset(b) hands row b's pages back. fork() shares pages
    between rows by reference: a per-page count says how many rows name a
    page, a row copies a shared tail page before its first write into it
    (_reserve), and a page returns to the free list when its last holder
    lets go. A pool that runs out and
    a row at its ceiling both raise RuntimeError naming the row, before
    anything is launched or stored.
    """

    def __init__(
        self,
        batch: int,
        kv_heads: int,
        head_dim: int,
        max_tokens: int,
        pool_tokens: int,
        page: int = 256,
        device: torch.device | str = "cuda",
        kv_dtype: str | torch.dtype = "bf16",
        block: int = 256,
        group: dist.ProcessGroup | None = None,
    ) -> None:
        if page not in _PAGE_SIZES:
            raise ValueError(f"PagedDecodeSession: page must be one of "
                             f"{_PAGE_SIZES}, got {page!r}")
        td, local_cap = self._setup(batch, max_tokens, device, kv_dtype,
                                    block, group)
        self._page = page
        max_pages = (local_cap + page - 1) // page
        n_pages = max(1, (pool_tokens + page - 1) // page)
        self.k_pool = torch.empty(n_pages, kv_heads, page, head_dim, dtype=td,
                                  device=self.device)
        self.v_pool = torch.empty_like(self.k_pool)
        # entries past a row's live pages are never read
        self.page_table = torch.zeros(batch, max_pages, dtype=torch.int32,
                                      device=self.device)
        self._pages: list[list[int]] = [[] for _ in range(batch)]
        self._free = list(range(n_pages - 1, -1, -1))   # pop() takes page 0
        # rows that name each page (fork shares pages): on _free exactly
        # when 0
        self._refs = [0] * n_pages
        # shared-prefix decode: _page_moves counts the pages that changed
        # hands (with each row's number of full pages it tells whether
        # shared_plan() can have changed); per Hq the plan last uploaded and
        # its device tables (static buffers: a captured graph reads them)
        self._page_moves = 0
        self._shared: dict[int, dict] = {}
        self.shared_plan_uploads = 0

    @property
    def page(self) -> int:
        return self._page

    @property
    def n_pages(self) -> int:
        return self.k_pool.size(0)

    @property
    def free_pages(self) -> int:
        return len(self._free)

    @property
    def shared_pages(self) -> int:
        """Pages that more than one row holds."""
        return sum(1 for r in self._refs if r > 1)

    # ---- storage: (n_pages, Hkv, page, D) pools behind the page table ----
    _graph_refusal = (
        "graphed_step: the paged cache kernel does not take this "
        "session (needs head_dim 128, a bf16/fp16 query, a pool of "
        "the query's dtype or fp8 under bf16, and Hq/Hkv <= 16)")

    @property
    def _kv(self) -> torch.Tensor:
        return self.k_pool

    @property
    def capacity(self) -> int:
        """Local positions one sequence can hold: the table's width."""
        return self.page_table.size(1) * self._page

    def _reserve(self, ends: dict[int, int]) -> None:
        """Raise if the pool cannot give every row its pages (nothing is
        taken then); else take them and write their table entries.

        Copy-on-write: row b writes at [local_lens[b], ends[b]), and
        _release has handed back every page past its live length, so the
        one page it can share with another row (fork) is the partial page
        holding local_lens[b]. While another row names that page, b takes a
        fresh one and the live rows are copied over, all rows' copies in
        one launch, before this returns: ahead of the append launch or the
        graph replay."""
        page, left = self._page, len(self._free)
        cow: dict[int, int] = {}     # row -> index of its shared tail page
        going: dict[int, int] = {}   # page -> rows leaving it in this call
        for b, end in ends.items():
            need = max((end + page - 1) // page - len(self._pages[b]), 0)
            at = self.local_lens[b]
            if end > at and at % page:
                pid = self._pages[b][at // page]
                if self._refs[pid] - going.get(pid, 0) > 1:
                    going[pid] = going.get(pid, 0) + 1
                    cow[b] = at // page
                    need += 1
            if need > left:
                raise RuntimeError(
                    f"PagedDecodeSession pool exhausted: row {b} needs "
                    f"{need} more page(s) of {page} tokens, {left} of "
                    f"{self.n_pages} free (grow pool_tokens or reset a row)")
            left -= need
        copies = []   # (shared page, the row's own page, live rows)
        for b, end in ends.items():
            if b in cow:
                j = cow[b]
                old, pid = self._pages[b][j], self._take()
                self._refs[old] -= 1
                self._pages[b][j] = pid
                self.page_table[b, j : j + 1].fill_(pid)
                copies.append((old, pid, self.local_lens[b] % page))
            while len(self._pages[b]) * page < end:
                pid = self._take()
                j = len(self._pages[b])
                self._pages[b].append(pid)
                self.page_table[b, j : j + 1].fill_(pid)
        if copies:
            self._copy_pages(copies)

    def _take(self) -> int:
        pid = self._free.pop()
        self._refs[pid] = 1
        self._page_moves += 1
        return pid

    def _drop(self, pids: list[int]) -> None:
        """One row lets go of pids: a page no row names any more goes back
        to the free list, the last of pids first (the next handed out)."""
        self._page_moves += len(pids)
        for pid in reversed(pids):
            self._refs[pid] -= 1
            if self._refs[pid] == 0:
                self._free.append(pid)

    def _copy_pages(self, copies: list[tuple[int, int, int]]) -> None:
        """The first `rows` rows of every head of page src into page dst,
        K and V, for each (src, dst, rows)."""
        if self._append_kernel_ok():
            self._ext().kv_pool_copy_rows(
                self.k_pool, self.v_pool, [c[0] for c in copies],
                [c[1] for c in copies], [c[2] for c in copies])
            return
        for src, dst, rows in copies:
            self.k_pool[dst, :, :rows] = self.k_pool[src, :, :rows]
            self.v_pool[dst, :, :rows] = self.v_pool[src, :, :rows]

    def _share(self, src: int, dst: int, n_local: int) -> None:
        """Row dst (empty) takes the pages of row src's first n_local local
        positions by reference: no KV byte moves and no page leaves the
        free list. The table entries go device to device, in stream order."""
        n = (n_local + self._page - 1) // self._page
        self._pages[dst] = self._pages[src][:n]
        self._page_moves += n
        for pid in self._pages[dst]:
            self._refs[pid] += 1
        if n:
            self.page_table[dst, :n].copy_(self.page_table[src, :n])

    def _store(self, b: int, pos: int, k_rows: torch.Tensor,
               v_rows: torch.Tensor) -> None:
        # page by page; _reserve has assigned every page touched
        t, n = 0, k_rows.shape[1]
        while t < n:
            off = pos % self._page
            m = min(n - t, self._page - off)
            pid = self._pages[b][pos // self._page]
            self.k_pool[pid, :, off : off + m] = \
                k_rows[:, t : t + m].to(self.k_pool.dtype)
            self.v_pool[pid, :, off : off + m] = \
                v_rows[:, t : t + m].to(self.v_pool.dtype)
            t, pos = t + m, pos + m

    def _rows(self, b: int, n: int):
        """Row b's first n local positions gathered from its pages into
        contiguous (1, Hkv, n, D) K and V."""
        idx = torch.tensor(self._pages[b][: (n + self._page - 1) // self._page],
                           dtype=torch.long, device=self.device)
        out = []
        for pool in (self.k_pool, self.v_pool):
            pages = pool.index_select(0, idx)          # (np, Hkv, page, D)
            rows = pages.permute(1, 0, 2, 3).reshape(
                1, pool.size(1), -1, pool.size(3))
            out.append(rows[:, :, :n].contiguous())
        return out

    def _fallback_rows(self, q: torch.Tensor, b: int, n: int):
        k, v = self._rows(b, n)
        if q.device.type == "cuda" and k.dtype == torch.float32:
            # the GPU kernels take no fp32 K/V: the gathered copy goes in
            # the query's dtype
            k, v = k.to(q.dtype), v.to(q.dtype)
        return k, v

    def _launch_append(self, ext, k_new, v_new, active_dev) -> None:
        ext.kv_pool_append(
            self.k_pool, self.v_pool, self.page_table,
            k_new.to(self.k_pool.dtype).contiguous(),
            v_new.to(self.v_pool.dtype).contiguous(), self.total_dev,
            self.local_len_dev, active_dev, self.block, self.rank,
            self.world)

    def _launch_attend(self, ext, q, scale: float):
        return ext.flash_attention_paged(
            q.contiguous(), self.k_pool, self.v_pool, self.page_table,
            self.local_len_dev, scale)

    # ---- shared-prefix decode ----
    def _check_shared(self, q: torch.Tensor) -> None:
        hkv = self.k_pool.size(1)
        if q.dim() != 4 or q.shape[0] != self.batch or q.shape[2] != 1:
            raise ValueError(
                f"shared=True takes one query per row: q must be (B, Hq, 1, "
                f"D) with B = {self.batch}, got {tuple(q.shape)}")
        if q.shape[1] % hkv or q.shape[1] // hkv > 16:
            raise ValueError(
                f"shared=True needs Hq a multiple of Hkv = {hkv} and Hq/Hkv "
                f"<= 16, got Hq = {q.shape[1]}")

    def shared_plan(self, q_heads: int | None = None
                    ) -> list[tuple[list[int], int]]:
        """The groups of attend(shared=True) under ``q_heads`` query heads
        (None: one per KV head): a list of (rows, prefix) in which every row
        appears exactly once. The rows of a group hold the same pages for
        their first ``prefix`` local tokens, whole pages all of them, and the
        group's first row is the one whose page table the prefix is read
        through. Host-side and per rank: it is over this rank's local pages.

        Page j of row b is full when local_lens[b] >= (j + 1) * page. Rows
        without a full page are groups of their own with prefix 0. The others
        fall into families by the id of their page 0; a family is sorted by
        (ids of the row's leading full pages that another row holds too, row
        index), so rows with long common runs are neighbours, and cut into
        groups of at most 16 / (Hq / Hkv) rows. A group's prefix is the
        longest run of leading full pages all its members name, times the
        page size; a group of one has prefix 0.

        A full page that two rows name is never written: the first write
        into a shared page replaces its id in the writer's list (_reserve).
        """
        hkv = self.k_pool.size(1)
        hq = hkv if q_heads is None else q_heads
        if hq <= 0 or hq % hkv or hq // hkv > 16:
            raise ValueError(f"shared_plan: q_heads = {hq} must be a "
                             f"multiple of Hkv = {hkv} with Hq/Hkv <= 16")
        per = 16 // (hq // hkv)
        full = [n // self._page for n in self.local_lens]
        families: dict[int, list[int]] = {}
        groups: list[tuple[list[int], int]] = []
        for b in range(self.batch):
            if full[b]:
                families.setdefault(self._pages[b][0], []).append(b)
            else:
                groups.append(([b], 0))

        def shared_run(b: int) -> list[int]:
            run = []
            for pid in self._pages[b][: full[b]]:
                if self._refs[pid] < 2:
                    break
                run.append(pid)
            return run

        for fam in families.values():
            fam.sort(key=lambda b: (shared_run(b), b))
            for i in range(0, len(fam), per):
                rows = fam[i : i + per]
                n = 0
                if len(rows) > 1:
                    lead = self._pages[rows[0]]
                    n = min(full[b] for b in rows)
                    for b in rows[1:]:
                        m = 0
                        while m < n and self._pages[b][m] == lead[m]:
                            m += 1
                        n = m
                groups.append((rows, n * self._page))
        groups.sort(key=lambda g: min(g[0]))
        return groups

    def _shared_tables(self, hq: int) -> dict:
        """The device copy of shared_plan(hq): members (B, 16) int32, counts
        (B,) int32, prefix (B,) int64 (one entry per group, B at the most;
        the unused groups have count 0) and start (B,) int64, each row's
        first key outside its group's prefix. Uploaded only when the plan
        differs from the one the buffers hold; the plan itself is recomputed
        only after a page changed hands or a row's number of full pages
        moved, so a steady decode step costs one tuple comparison."""
        t = self._shared.get(hq)
        if t is None:
            dev, b = self.device, self.batch
            t = self._shared[hq] = {
                "key": None, "plan": None,
                "members": torch.zeros(b, 16, dtype=torch.int32, device=dev),
                "counts": torch.zeros(b, dtype=torch.int32, device=dev),
                "prefix": torch.zeros(b, dtype=torch.long, device=dev),
                "start": torch.zeros(b, dtype=torch.long, device=dev),
            }
        key = (self._page_moves,
               tuple(n // self._page for n in self.local_lens))
        if key == t["key"]:
            return t
        t["key"] = key
        plan = self.shared_plan(hq)
        if plan == t["plan"]:
            return t
        t["plan"] = plan
        members = torch.zeros(self.batch, 16, dtype=torch.int32)
        counts = torch.zeros(self.batch, dtype=torch.int32)
        prefix = torch.zeros(self.batch, dtype=torch.long)
        start = torch.zeros(self.batch, dtype=torch.long)
        for g, (rows, n) in enumerate(plan):
            members[g, : len(rows)] = torch.tensor(rows, dtype=torch.int32)
            counts[g] = len(rows)
            prefix[g] = n
            start[rows] = n
        for name, host in (("members", members), ("counts", counts),
                           ("prefix", prefix), ("start", start)):
            t[name].copy_(host)
        self.shared_plan_uploads += 1
        return t

    def _launch_attend_shared(self, ext, q, scale: float, tables: dict):
        return ext.flash_attention_paged_shared(
            q.contiguous(), self.k_pool, self.v_pool, self.page_table,
            self.local_len_dev, tables["members"], tables["counts"],
            tables["prefix"], tables["start"], scale)

    def _local_partial_shared(self, q: torch.Tensor,
                              softmax_scale: float | None):
        self._check_shared(q)
        tables = self._shared_tables(q.shape[1])
        if _zero_copy_ok(q, self._kv):
            return self._launch_attend_shared(
                self._ext(), q, _scale(softmax_scale, q), tables)
        # the same two passes in torch: per group the prefix rows gathered
        # once for all members' queries, per row the remainder, one merge
        out_p, lse_p = _empty_partial(q)
        out_s, lse_s = _empty_partial(q)
        for rows, n in tables["plan"]:
            if n:
                k, v = self._fallback_rows(q[:1], rows[0], n)
                o, l = local_attention(
                    q[rows], k.expand(len(rows), -1, -1, -1),
                    v.expand(len(rows), -1, -1, -1), softmax_scale)
                out_p[rows], lse_p[rows] = o, l
            for b in rows:
                if self.local_lens[b] > n:
                    qb = q[b : b + 1]
                    k, v = self._fallback_rows(qb, b, self.local_lens[b])
                    out_s[b : b + 1], lse_s[b : b + 1] = local_attention(
                        qb, k[:, :, n:], v[:, :, n:], softmax_scale)
        return combine_partials(torch.stack([out_p, out_s]),
                                torch.stack([lse_p, lse_s]))

    def _launch_append_n(self, ext, k_new, v_new, counts_dev, vis_dev) -> None:
        ext.kv_pool_append_n(
            self.k_pool, self.v_pool, self.page_table,
            k_new.to(self.k_pool.dtype).contiguous(),
            v_new.to(self.v_pool.dtype).contiguous(), self.total_dev,
            self.local_len_dev, counts_dev, vis_dev, self.block, self.rank,
            self.world)

    def _launch_attend_many(self, ext, q, scale: float, vis_dev):
        return ext.flash_attention_paged_qlen(
            q.contiguous(), self.k_pool, self.v_pool, self.page_table,
            self.local_len_dev, vis_dev, scale)

    def _launch_append_tree(self, ext, k_new, v_new, counts_dev, parents_dev,
                            base_dev, mask_dev) -> None:
        ext.kv_pool_append_tree(
            self.k_pool, self.v_pool, self.page_table, k_new, v_new,
            self.total_dev, self.local_len_dev, counts_dev, parents_dev,
            base_dev, mask_dev, self.block, self.rank, self.world)

    def _launch_attend_tree(self, ext, q, scale: float, base_dev, mask_dev):
        return ext.flash_attention_paged_tree(
            q.contiguous(), self.k_pool, self.v_pool, self.page_table,
            self.local_len_dev, base_dev, mask_dev, scale)

    def _launch_commit(self, ext, k_new, v_new, counts_dev, path_dev,
                       lens_dev) -> None:
        ext.kv_pool_commit_path(
            self.k_pool, self.v_pool, self.page_table, k_new, v_new,
            self.total_dev, self.local_len_dev, counts_dev, path_dev,
            lens_dev, self.block, self.rank, self.world)

    def _release(self, b: int) -> None:
        """The row lets go of the pages past ceil(local_len / page): those
        no other row holds go back to the free list, the next ones handed
        out and in reset()'s order; their stale table entries are never
        read."""
        keep = (self.local_lens[b] + self._page - 1) // self._page
        self._drop(self._pages[b][keep:])
        del self._pages[b][keep:]

    def reset(self, b: int) -> None:
        """Free slot b for a new sequence: its lengths go to 0 on host and
        device and its pages, where no other row holds them, back to the
        free list (the next ones handed out); nothing is cleared."""
        super().reset(b)
        self._drop(self._pages[b])
        self._pages[b] = []
