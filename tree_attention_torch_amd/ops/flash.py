"""Local attention partial — dispatch between the CDNA4 HIP kernels and the
CPU oracle.

On a GPU (ROCm) device the hand-written gfx950 kernels in ops/hip/ are the
ONLY path: if the compiled extension is missing we raise instead of silently
falling back to eager PyTorch — a silent fallback would fake GPU test passes
without exercising native code. On CPU tensors the fp32 oracle
(ops/reference.py) runs, which is what the no-GPU CI tier exercises.

Reference parity: this layer replaces ``flash_res_lse``'s "simulated" flash
attention (/root/reference/model.py:60-83) with a real flash kernel — the
thing the reference's README admits it never integrated (README.md:21).
"""

from __future__ import annotations

import math
import os

import torch

from . import reference
from ..quant import MLA_FP8_ROW, dequantize_mla_fp8, quantize_mla_fp8

_EXT = None
_EXT_ERR: Exception | None = None


def _load_extension():
    """Import the in-tree compiled HIP extension (ops/hip/_tree_attn_hip.so)."""
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    try:
        from .hip import _tree_attn_hip  # type: ignore

        _EXT = _tree_attn_hip
    except ImportError as e:  # pragma: no cover - GPU-box path
        _EXT_ERR = e
    return _EXT


def hip_available() -> bool:
    return _load_extension() is not None


def decode_loop_chunks(tq: int, g: int, b: int, hq: int) -> int:
    """Spec-decode routing decision (pure; pinned by tests/test_routing.py).

    Returns the number of decode-kernel query chunks to loop over, or 0 when
    a single extension dispatch is right (plain decode Tq*G <= 16 — the
    extension routes that to the split-KV decode kernel — or a prefill-sized
    batch that fills the 512-block grid).

    Cost model (measured sweep, H=32 @ 32K/128K KV): each decode chunk is
    one full-bandwidth KV stream; the underfilled prefill launch costs
    about (512/blocks) streams. Loop while n_chunks is under that.
    Tq=17..32: 0.72 vs 9.62 ms at 128K; Tq=128: 2.65 vs 9.62; crossover
    measured at Tq≈256 (prefill 1.47 vs loop 1.61 at 32K) = the n_chunks
    == 512/blocks point, so strict <.
    """
    if g > 16:
        # MFMA-M batching packs G query heads per KV head into the 16-row
        # M dimension; G > 16 (e.g. MQA Hq=32, Hkv=1) does not fit one tile.
        raise ValueError(
            f"tree_attention: GQA group size Hq/Hkv = {g} exceeds the native "
            "kernel limit of 16 (MFMA-M batching). Replicate KV heads so "
            "that Hq/Hkv <= 16."
        )
    tq_per = 16 // g
    n_chunks = -(-tq // tq_per)
    prefill_blocks = b * hq * (-(-tq // 256))
    max_chunks = max(4, 512 // max(prefill_blocks, 1))
    if tq_per < tq and n_chunks < max_chunks and prefill_blocks < 512:
        return n_chunks
    return 0


def _dispatch_hip(ext, q, k, v, softmax_scale, is_causal, q_offset, kv_offset):
    """Route between the split-KV decode kernel and the prefill kernel.

    The extension itself routes Tq*G <= 16 to decode (MFMA-M batching) and
    everything else to prefill (256-row q-blocks). For SMALL query batches
    just past 16 rows — speculative decode: Tq 17..64 against a long KV —
    the prefill grid is only B*Hq blocks (vs the 512 the chip wants) with
    no KV split, so instead loop the decode kernel over query chunks: each
    chunk launches the full split-KV grid (decode_loop_chunks above).
    """
    tq = q.shape[2]
    g = q.shape[1] // k.shape[1]
    if decode_loop_chunks(tq, g, q.shape[0], q.shape[1]) > 0:
        tq_per = 16 // g
        outs, lses = [], []
        for lo in range(0, tq, tq_per):
            hi = min(tq, lo + tq_per)
            o, l = ext.flash_attention(
                q[..., lo:hi, :].contiguous(), k, v,
                float(softmax_scale), bool(is_causal),
                int(q_offset + lo), int(kv_offset),
            )
            outs.append(o)
            lses.append(l)
        return torch.cat(outs, dim=-2), torch.cat(lses, dim=-1)
    return ext.flash_attention(
        q, k, v, float(softmax_scale), bool(is_causal),
        int(q_offset), int(kv_offset),
    )


def local_attention(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    softmax_scale: float | None = None,
    is_causal: bool = False,
    q_offset: int = 0,
    kv_offset: int = 0,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Compute the local flash-attention partial (out, lse) on q's device.

    Shapes: q (B, Hq, Tq, D); k, v (B, Hkv, Tk, D) with Hkv | Hq (GQA).
    Returns out (B, Hq, Tq, D) fp32 and lse (B, Hq, Tq) fp32.
    """
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(q.shape[-1])
    if q.device.type == "cuda":
        ext = _load_extension()
        if ext is None:
            if os.environ.get("TREE_ATTN_ALLOW_EAGER_GPU") == "1":
                return reference.flash_res_lse(
                    q, k, v, softmax_scale, is_causal, q_offset, kv_offset
                )
            raise RuntimeError(
                "tree_attention: the gfx950 HIP extension _tree_attn_hip is not "
                "built but a GPU tensor was passed. Build it with "
                "`python setup.py build_ext --inplace` (or __graft_entry__.build()). "
                f"Import error: {_EXT_ERR}"
            )
        d = q.shape[-1]
        halfish = k.dtype in (torch.bfloat16, torch.float16)
        # D=64 is native for bf16/fp16 (decode and prefill kernels);
        # D in {32,48,80,96,112} is native for bf16/fp16 DECODE (the
        # zero-padded-LDS narrow-head kernel — no global pad copies).
        native_d64 = d == 64 and halfish
        g = q.shape[1] // k.shape[1]
        tq = q.shape[2]
        # will the extension run the prefill kernel (vs decode/spec-loop)?
        will_prefill = tq * g > 16 and \
            decode_loop_chunks(tq, g, q.shape[0], q.shape[1]) == 0
        narrow_decode = (halfish and not will_prefill
                         and d in (32, 48, 80, 96, 112))
        if d < 128 and not native_d64 and not narrow_decode:
            # exact zero-padding fallback: padded dims add 0 to every q.k
            # score and the padded output columns are sliced off.
            # (softmax_scale above was computed from the REAL D.) Pad to the
            # SMALLEST natively supported dim, not always 128.
            import torch.nn.functional as F

            if halfish:
                supported = ((64, 128) if will_prefill
                             else (32, 48, 64, 80, 96, 112, 128))
            else:
                supported = (128,)
            target = next(s for s in supported if s >= d)
            pad = target - d

            def _pad(t):
                if t.dtype == torch.float8_e4m3fn:  # F.pad lacks fp8 support
                    return F.pad(t.view(torch.uint8), (0, pad)).view(
                        torch.float8_e4m3fn).contiguous()
                return F.pad(t, (0, pad)).contiguous()

            out, lse = _dispatch_hip(
                ext, _pad(q), _pad(k), _pad(v),
                softmax_scale, is_causal, q_offset, kv_offset,
            )
            return out[..., :d].contiguous(), lse
        return _dispatch_hip(
            ext, q.contiguous(), k.contiguous(), v.contiguous(),
            softmax_scale, is_causal, q_offset, kv_offset,
        )
    return reference.flash_res_lse(q, k, v, softmax_scale, is_causal, q_offset, kv_offset)


def mx_decode_shaped(hq: int, hkv: int, tq: int) -> bool:
    """MX route decision (pure; pinned by tests/test_routing.py): group
    rows G*Tq <= 16 fit one MFMA-M batch, so the split-KV hardware-scale
    DECODE kernel runs (zero-copy-capable, per-head byte strides);
    anything larger goes to the MX prefill kernel (packed tensors)."""
    return (hq // hkv) * tq <= 16


def _rows_contig(t: "torch.Tensor") -> bool:
    """Per-head rows packed (stride(3)==1, stride(2)==row length) with a
    free head stride — the layout the MX decode kernel binds ZERO-COPY
    (sliced views of a preallocated DecodeSession cache)."""
    return (t.stride(3) == 1 and t.stride(2) == t.shape[3]
            and t.stride(0) == t.stride(1) * t.shape[1])


def local_attention_mx(
    q: torch.Tensor,
    k8: torch.Tensor,
    ks: torch.Tensor,
    v8: torch.Tensor,
    vs: torch.Tensor,
    softmax_scale: float | None = None,
    is_causal: bool = False,
    q_offset: int = 0,
    kv_offset: int = 0,
) -> tuple[torch.Tensor, torch.Tensor]:
    """MX block-scaled fp8 attention: K/V are e4m3 plus per-block E8M0
    scales from quant.quantize_k_mx / quantize_v_mx. The hardware applies
    the scales inside mfma_scale_f32_32x32x64_f8f6f4 (block semantics
    pinned on silicon — tools/check_mx_scales.py), so a KV cache with
    outlier channels/tokens quantizes at full e4m3 relative precision
    where plain fp8 saturates to NaN. GPU-only (no CPU oracle dispatch:
    use quant.dequantize_*_mx + ops.reference for oracles)."""
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(q.shape[-1])
    ext = _load_extension()
    if ext is None:
        raise RuntimeError("MX fp8 attention requires the HIP extension")
    if q.dtype == torch.float16:
        # the MX kernels quantize Q to e4m3 in-prologue; a bf16 round-trip
        # of an fp16 query is lossless relative to that quantization
        q = q.to(torch.bfloat16)
    decode_shaped = mx_decode_shaped(q.shape[1], k8.shape[1], q.shape[2])
    if not (decode_shaped and all(map(_rows_contig, (k8, ks, v8, vs)))):
        # the prefill kernel wants packed tensors; the decode kernel takes
        # per-head byte strides, so session-cache VIEWS pass zero-copy
        k8, ks = k8.contiguous(), ks.contiguous()
        v8, vs = v8.contiguous(), vs.contiguous()
    return ext.flash_attention_fp8_mx(
        q.contiguous(), k8, ks, v8, vs, float(softmax_scale),
        bool(is_causal), int(q_offset), int(kv_offset),
    )


MLA_D_QK = 576   # 512 latent + 64 rotary columns of a cache row
MLA_D_V = 512    # V is the first 512 columns of the row that K is
MLA_MAX_HEADS = 128


def mla_decode(
    q: torch.Tensor,
    ckv: torch.Tensor,
    kv_lens: torch.Tensor | None = None,
    softmax_scale: float | None = None,
    splits: int | None = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """Multi-head latent attention decode partial over a shared latent cache.

    q is (B, Hq, 1, 576) with the up-projections absorbed, ckv (B, 1, Tkv,
    576) of the same dtype: one row per token, read by every head; K is the
    row and V its first 512 columns. ckv may be a view along the key axis of
    a larger preallocated buffer. kv_lens: optional (B,) int64 on q's device,
    the live rows of each batch row (a row of length 0 gives out = 0, lse =
    -inf). splits forces the split-KV count (None: the plan).

    Returns out (B, Hq, 1, 512) fp32 and lse (B, Hq, 1) fp32: a partial that
    combine_partials / tree_combine merge like any other.
    """
    if q.dim() != 4 or ckv.dim() != 4:
        raise ValueError("mla_decode: q is (B, Hq, Tq, 576), ckv (B, 1, Tkv, 576)")
    if q.shape[-1] != MLA_D_QK or ckv.shape[-1] != MLA_D_QK:
        raise ValueError(
            f"mla_decode: (d_qk, d_v) = ({MLA_D_QK}, {MLA_D_V}) is the only "
            f"supported pair (got q width {q.shape[-1]}, ckv width "
            f"{ckv.shape[-1]})")
    if q.shape[2] != 1:
        raise NotImplementedError(
            f"mla_decode: Tq = {q.shape[2]}; only Tq = 1 (plain decode) is "
            "implemented")
    if ckv.shape[1] != 1 or ckv.shape[0] != q.shape[0]:
        raise ValueError("mla_decode: ckv must be (B, 1, Tkv, 576) with q's B")
    if q.shape[1] > MLA_MAX_HEADS:
        raise ValueError(
            f"mla_decode: Hq = {q.shape[1]} exceeds the native limit of "
            f"{MLA_MAX_HEADS} heads per launch")
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(MLA_D_QK)
    if q.device.type != "cuda":
        return reference.mla_reference(q, ckv, kv_lens, softmax_scale)
    ext = _load_extension()
    if ext is None:
        raise RuntimeError(
            "mla_decode: the gfx950 HIP extension _tree_attn_hip is not built "
            "but a GPU tensor was passed. Build it with "
            f"__graft_entry__.build(). Import error: {_EXT_ERR}")
    if q.dtype not in (torch.bfloat16, torch.float16) or ckv.dtype != q.dtype:
        raise ValueError("mla_decode: q and ckv must both be bf16 or both fp16")
    b, hq = q.shape[0], q.shape[1]
    if ckv.shape[2] == 0:  # no key at all: nothing to launch
        return (q.new_zeros((b, hq, 1, MLA_D_V), dtype=torch.float32),
                q.new_full((b, hq, 1), float("-inf"), dtype=torch.float32))
    if ckv.stride(3) != 1 or ckv.stride(2) != MLA_D_QK:
        ckv = ckv.contiguous()
    if kv_lens is not None:
        kv_lens = kv_lens.to(device=q.device, dtype=torch.int64).contiguous()
    return ext.flash_attention_mla(q.contiguous(), ckv, kv_lens,
                                   float(softmax_scale), int(splits or 0))


MLA_PAGE_SIZES = (128, 256, 512, 1024)
MLA_MAX_TQ = 16


def mla_chain_vis(kv_lens: torch.Tensor, tq: int) -> torch.Tensor:
    """The chain mask of a verify step whose tq drafts are the last tq rows
    of each sequence: vis[b, i] = max(kv_lens[b] - (tq - 1 - i), 0)."""
    back = torch.arange(tq - 1, -1, -1, device=kv_lens.device)
    return (kv_lens.to(torch.int64)[:, None] - back[None, :]).clamp(min=0)


def mla_decode_paged(
    q: torch.Tensor,
    pool: torch.Tensor,
    page_table: torch.Tensor,
    kv_lens: torch.Tensor,
    vis: torch.Tensor | None = None,
    softmax_scale: float | None = None,
    splits: int = 0,
    tree: tuple[torch.Tensor, torch.Tensor] | None = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """MLA decode partial over a PAGED latent pool, Tq query positions per
    row (a multi-token verify step).

    q is (B, Hq, Tq, 576) with Tq in 1..16, pool (n_pages, 1, page, 576) of
    q's dtype, or the "fp8_block" store (n_pages, 1, page, 656) uint8 of
    quant.quantize_mla_fp8 under a bf16 q (656 B per token instead of 1152;
    K and V are read exactly, the block scales go onto the fp32 scores and
    onto P), with page in 128 / 256 / 512 / 1024, page_table (B, max_pages)
    int32: entry [b, j] is the page of row b's positions [j * page, (j + 1) *
    page), clamped into the pool; only entries j < ceil(kv_lens[b] / page)
    are read. kv_lens (B,) is each row's length (at most max_pages * page).
    vis (B, Tq) int64: query position i of row b sees the keys below
    min(vis[b, i], kv_lens[b]); None is the chain mask mla_chain_vis. splits
    forces the split-KV count (0: the plan).

    tree = (base, mask), instead of vis, is the ancestor mask of a verify
    step over a draft TREE (ops/hip/ta_abi.h TreeArgs): base (B,) int64 is
    the length of row b's committed prefix and mask (B, Tq) int32, both on
    q's device; the key at position p is masked for query i iff p >= base[b]
    and bit p - base[b] of mask[b, i] is clear (the drafts are the at most 16
    rows behind the prefix; higher bits are ignored).
    PagedMlaSession.append_tree leaves both.

    Returns out (B, Hq, Tq, 512) fp32 and lse (B, Hq, Tq) fp32; a query that
    sees no key has out = 0 and lse = -inf.
    """
    if tree is not None:
        if vis is not None:
            raise ValueError("mla_decode_paged: vis and tree exclude each "
                             "other")
        base, mask = tree
        b, tq = q.shape[0], q.shape[2] if q.dim() == 4 else 0
        if (tuple(base.shape) != (b,) or base.dtype != torch.int64
                or tuple(mask.shape) != (b, tq) or mask.dtype != torch.int32
                or base.device != q.device or mask.device != q.device):
            raise ValueError(
                f"mla_decode_paged: tree is (base (B,) int64, mask (B, Tq) "
                f"int32) = (({b},), ({b}, {tq})) on q's device, got "
                f"{tuple(base.shape)} {base.dtype} / {tuple(mask.shape)} "
                f"{mask.dtype}")
        tree = (base.contiguous(), mask.contiguous())
    return _mla_paged("mla_decode_paged", False, q, pool, page_table,
                      kv_lens, vis, softmax_scale, splits, tree)


def mla_prefill_paged(
    q: torch.Tensor,
    pool: torch.Tensor,
    page_table: torch.Tensor,
    kv_lens: torch.Tensor,
    vis: torch.Tensor | None = None,
    softmax_scale: float | None = None,
    splits: int = 0,
    compute: str | None = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    """MLA chunked prefill over a PAGED latent pool: mla_decode_paged's
    arguments, masks and results for ANY number T >= 1 of query positions per
    row, q (B, Hq, T, 576), e.g. the T new tokens of a prompt whose prefix the
    pool already holds (vis=None: the chain mask over the row's last T rows).

    On the GPU this is fa_mla_prefill_kernel: blocks of 64 (position, head)
    rows that stream the pool once per block, where a loop of mla_decode_paged
    streams it once per 16 positions: 1.3x - 5.3x faster than that loop at T
    256 and 2048 behind 8K and 32K (profiles/README.md, "MLA chunked
    prefill"). mla_decode_paged is never routed here.

    compute="fp8" is the consent to run an "fp8_block" pool under a bf16 q on
    the GPU, through fa_mla_prefill_fp8_kernel: the pool's e4m3 bytes enter
    the fp8 MFMA as they lie, and the LATENT columns of q are rounded to e4m3
    per (row, 128-column block) by quant.quantize_mla_fp8's rule; rotary
    columns, P and V are as in mla_decode_paged's fp8_block path. On the CPU
    it is that kernel's oracle: the fp32 reference over the dequantized rows
    and dequantize_mla_fp8(quantize_mla_fp8(q)). The rounding costs up to
    0.095 of out (abs err / (1 + abs ref)) and 0.067 of lse against unrounded
    queries (README, "MLA fp8 latent store"). Without the keyword the
    "fp8_block" pool works on the CPU and raises NotImplementedError on the
    GPU. compute="fp8" over a bf16 or fp16 pool, and any other value, raise
    ValueError.
    """
    return _mla_paged("mla_prefill_paged", True, q, pool, page_table, kv_lens,
                      vis, softmax_scale, splits, compute=compute)


def _mla_paged(who, prefill, q, pool, page_table, kv_lens, vis, softmax_scale,
               splits, tree=None, compute=None):
    """What mla_decode_paged (the decode kernel, Tq <= MLA_MAX_TQ) and
    mla_prefill_paged (prefill=True: the prefill kernel, any Tq) share.
    tree: the checked (base, mask) of mla_decode_paged, instead of vis.
    compute: mla_prefill_paged's keyword (prefill only)."""
    if compute not in (None, "fp8"):
        raise ValueError(f"{who}: compute must be None or 'fp8', got "
                         f"{compute!r}")
    if q.dim() != 4 or q.shape[-1] != MLA_D_QK:
        raise ValueError(f"{who}: q is (B, Hq, Tq, {MLA_D_QK})")
    b, hq, tq = q.shape[:3]
    if prefill and tq < 1:
        raise ValueError(f"{who}: Tq = {tq}; at least one query position")
    if not prefill and not 1 <= tq <= MLA_MAX_TQ:
        raise ValueError(f"{who}: Tq = {tq} is outside 1..{MLA_MAX_TQ}")
    if not 1 <= hq <= MLA_MAX_HEADS:
        raise ValueError(
            f"{who}: Hq = {hq} is outside the native range 1..{MLA_MAX_HEADS}")
    fp8 = pool.dtype == torch.uint8
    if (pool.dim() != 4 or pool.shape[1] != 1 or pool.shape[0] < 1
            or pool.shape[3] != (MLA_FP8_ROW if fp8 else MLA_D_QK)):
        raise ValueError(f"{who}: pool is (n_pages, 1, page, {MLA_D_QK}), or "
                         f"(n_pages, 1, page, {MLA_FP8_ROW}) uint8")
    page = pool.shape[2]
    if page not in MLA_PAGE_SIZES:
        raise ValueError(f"{who}: page must be one of {MLA_PAGE_SIZES}, got "
                         f"{page}")
    if fp8 and q.dtype != torch.bfloat16:
        raise NotImplementedError(
            f"{who}: the fp8_block pool keeps its rotary columns in bf16 and "
            f"takes a bf16 q (got {q.dtype})")
    if not fp8 and pool.dtype != q.dtype:
        raise ValueError(f"{who}: q and pool must have one dtype")
    if compute == "fp8" and not fp8:
        raise ValueError(f"{who}: compute='fp8' needs the fp8_block pool; a "
                         f"{pool.dtype} pool holds nothing in e4m3")
    if (page_table.dim() != 2 or page_table.shape[0] != b
            or page_table.shape[1] < 1 or page_table.dtype != torch.int32):
        raise ValueError(f"{who}: page_table is int32 (B, max_pages)")
    if kv_lens.dim() != 1 or kv_lens.shape[0] != b:
        raise ValueError(f"{who}: kv_lens is (B,)")
    if vis is not None and tuple(vis.shape) != (b, tq):
        raise ValueError(f"{who}: vis is (B, Tq) = ({b}, {tq}), got "
                         f"{tuple(vis.shape)}")
    if softmax_scale is None:
        softmax_scale = 1.0 / math.sqrt(MLA_D_QK)
    kv_lens = kv_lens.to(device=q.device, dtype=torch.int64).contiguous()
    if tree is not None:
        pass
    elif vis is None:
        vis = mla_chain_vis(kv_lens, tq) if tq > 1 or prefill else None
    else:
        vis = vis.to(device=q.device, dtype=torch.int64).contiguous()
    if q.device.type != "cuda":
        cap = page_table.shape[1] * page
        lens = kv_lens.clamp(0, cap)
        n_max = int(lens.max())
        ckv = torch.zeros((b, 1, max(n_max, 1), MLA_D_QK),
                          dtype=torch.float32 if fp8 else pool.dtype)
        for i, n in enumerate(lens.tolist()):
            ids = page_table[i, : -(-n // page)].long().clamp(0, pool.shape[0] - 1)
            rows = pool[ids, 0].reshape(-1, pool.shape[3])[:n]
            ckv[i, 0, :n] = dequantize_mla_fp8(rows) if fp8 else rows
        q_ref = q.float() if fp8 else q
        if compute == "fp8":  # the kernel's rounding of the latent columns
            q_ref = dequantize_mla_fp8(quantize_mla_fp8(q_ref))
        return reference.mla_reference(q_ref, ckv, lens, softmax_scale,
                                       vis=vis, tree=tree)
    ext = _load_extension()
    if ext is None:
        raise RuntimeError(
            f"{who}: the gfx950 HIP extension _tree_attn_hip is not built "
            "but a GPU tensor was passed. Build it with "
            f"__graft_entry__.build(). Import error: {_EXT_ERR}")
    if fp8 and prefill and compute != "fp8":
        raise NotImplementedError(
            f"{who}: no chunked prefill over the fp8_block pool on the GPU "
            "without compute='fp8', which rounds q's latent columns to e4m3; "
            "loop mla_decode_paged, or use a bf16 or fp16 pool")
    if q.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError(f"{who}: q and pool must both be bf16 or both fp16")
    if tree is not None:
        decode = ext.flash_attention_mla_paged_tree_fp8 if fp8 \
            else ext.flash_attention_mla_paged_tree
        return decode(q.contiguous(), pool, page_table, kv_lens, *tree,
                      float(softmax_scale), int(splits or 0))
    if fp8 and prefill:
        return ext.flash_attention_mla_prefill_paged_fp8(
            q.contiguous(), pool, page_table, kv_lens, vis,
            float(softmax_scale), int(splits or 0))
    if fp8:
        return ext.flash_attention_mla_paged_fp8(
            q.contiguous(), pool, page_table, kv_lens, vis,
            float(softmax_scale), int(splits or 0))
    if prefill:
        return ext.flash_attention_mla_prefill_paged(
            q.contiguous(), pool, page_table, kv_lens, vis,
            float(softmax_scale), int(splits or 0))
    return ext.flash_attention_mla_paged(
        q.contiguous(), pool, page_table, kv_lens, vis, float(softmax_scale),
        int(splits or 0))


# Reference-compatible alias: same name/signature shape as model.py:60.
def flash_res_lse(
    q: torch.Tensor,
    k: torch.Tensor,
    v: torch.Tensor,
    softmax_scale: float | None = None,
    is_causal: bool = False,
) -> tuple[torch.Tensor, torch.Tensor]:
    return local_attention(q, k, v, softmax_scale=softmax_scale, is_causal=is_causal)


__all__ = ["local_attention", "local_attention_mx", "flash_res_lse",
           "hip_available", "decode_loop_chunks", "mla_decode",
           "mla_decode_paged", "mla_prefill_paged", "mla_chain_vis",
           "MLA_FP8_ROW"]
