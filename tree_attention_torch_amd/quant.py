"""MX (block-scaled) fp8 quantization for the KV cache.

Reference parity note: the reference (/root/reference/model.py) has no
quantization of any kind — this module is a capability EXTENSION of the
reference's fp16 attention (model.py:51-53) for the MI355X serving
target (BASELINE.json config 5's fp8 KV path, hardened against outlier
channels/tokens that plain e4m3 saturates or NaNs on).

The gfx950 `mfma_scale_f32_32x32x64_f8f6f4` instruction dequantizes its
fp8 operands with per-32-element E8M0 scales in hardware. The scale-block
semantics were pinned on silicon (tools/check_mx_scales.py): within each
64-element contraction window the two blocks are the INTERLEAVED logical
sets {k: (k>>4)&1 == 0} = {0-15, 32-47} and {16-31, 48-63} — the
instruction's internal k-order swaps bits 4 and 5 of the logical index.

For the K cache (contraction axis = head dim, windows of 64 dims) the
quantization groups per row are therefore

    group(s64, blk) = dims  s64*64 + {0-15, 32-47}   (blk = 0)
                      s64*64 + {16-31, 48-63}        (blk = 1)

i.e. group index = (d >> 6) * 2 + ((d >> 4) & 1), giving D/32 groups per
row (4 for D=128). E8M0 scale: s = 127 + ceil(log2(absmax / 448)) clamped
to [0, 254]; stored value dequantizes as x * 2^(s-127). Zero/absent
groups use s = 127.

Why block scales at all: plain e4m3 saturates at |x| = 448 and flushes
below ~2^-9 — a K cache with outlier channels (the classic quantization
hazard in real models) clips silently. Block scales recenter each group
into e4m3's range; for unit-variance synthetic data they are a no-op by
construction (s = 127 everywhere), which is why round 1's unit-scale
path measured fine on randn inputs.
"""

from __future__ import annotations

import torch

__all__ = ["quantize_k_mx", "dequantize_k_mx", "quantize_v_mx",
           "dequantize_v_mx", "mx_group_index", "quantize_rows_fp8",
           "dequantize_rows_fp8", "quantize_mla_fp8", "dequantize_mla_fp8",
           "MLA_FP8_ROW"]

_ROW_TINY = 2.0 ** -100   # amax floor: a zero row gets a finite scale


def quantize_rows_fp8(x: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-token-scaled fp8 ("fp8_scaled"): one fp32 scale per row of the
    last dimension, all in fp32:

        scale   = max(amax(|x|), 2^-100) / 448
        payload = e4m3(clamp(x / scale, -448, 448))   round-to-nearest-even

    x (..., D) -> (payload (..., D) float8_e4m3fn, scale (...) fp32). Both
    divisions are IEEE fp32 divisions, which kv_append_quant_kernel
    (ops/hip/fa_kernels.hip) performs too: the kernel's bytes and scales
    equal these bit for bit. A row of zeros gets scale 2^-100 / 448 and a
    zero payload, so log(scale) is finite for every row."""
    xf = x.to(torch.float32)
    scale = xf.abs().amax(dim=-1).clamp_min(_ROW_TINY) / 448.0
    y = (xf / scale.unsqueeze(-1)).clamp(-448.0, 448.0)
    return y.to(torch.float8_e4m3fn), scale


def dequantize_rows_fp8(payload: torch.Tensor,
                        scale: torch.Tensor) -> torch.Tensor:
    """payload (..., D) e4m3 and scale (...) fp32 -> fp32 rows."""
    return payload.to(torch.float32) * scale.unsqueeze(-1)

MLA_FP8_ROW = 656   # bytes of one "fp8_block" latent row
_MLA_LATENT, _MLA_BLOCK = 512, 128


def quantize_mla_fp8(c: torch.Tensor) -> torch.Tensor:
    """The "fp8_block" MLA latent row: c (..., 576) -> (..., 656) uint8,

        [0, 512)    e4m3 payload of latent columns 0..511
        [512, 528)  four fp32 scales, one per block of 128 columns
        [528, 656)  rotary columns 512..575 as bf16, unquantized

    Each 128-column block is quantized on its own by quantize_rows_fp8's
    rule, so mla_append_quant_kernel (ops/hip/fa_kernels.hip) writes these
    bytes bit for bit."""
    lead = c.shape[:-1]
    payload, scale = quantize_rows_fp8(
        c[..., :_MLA_LATENT].reshape(*lead, 4, _MLA_BLOCK))
    rope = c[..., _MLA_LATENT:].to(torch.bfloat16).contiguous()
    return torch.cat([payload.view(torch.uint8).reshape(*lead, _MLA_LATENT),
                      scale.contiguous().view(torch.uint8).reshape(*lead, 16),
                      rope.view(torch.uint8).reshape(*lead, 128)], dim=-1)


def dequantize_mla_fp8(rows: torch.Tensor) -> torch.Tensor:
    """rows (..., 656) uint8 -> the (..., 576) fp32 rows they stand for."""
    lead = rows.shape[:-1]
    payload = rows[..., :_MLA_LATENT].contiguous().view(torch.float8_e4m3fn)
    scale = rows[..., _MLA_LATENT:_MLA_LATENT + 16].contiguous().view(
        torch.float32)
    latent = dequantize_rows_fp8(payload.reshape(*lead, 4, _MLA_BLOCK), scale)
    rope = rows[..., _MLA_LATENT + 16:].contiguous().view(torch.bfloat16)
    return torch.cat([latent.reshape(*lead, _MLA_LATENT), rope.float()],
                     dim=-1)


_E4M3_MAX = 448.0


def mx_group_index(d: torch.Tensor | int):
    """Logical head-dim index -> MX scale-group index (see module doc)."""
    if isinstance(d, int):
        return (d >> 6) * 2 + ((d >> 4) & 1)
    return (d >> 6) * 2 + ((d >> 4) & 1)


def quantize_k_mx(k: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Quantize K (..., T, D) to (fp8 e4m3, E8M0 group scales).

    Returns (k8, scales) with k8 float8_e4m3fn of k's shape and scales
    uint8 of shape (..., T, D//32) indexed by mx_group_index.
    """
    d = k.shape[-1]
    assert d % 64 == 0, "MX K quantization needs D a multiple of 64"
    ngrp = d // 32
    dims = torch.arange(d, device=k.device)
    gidx = mx_group_index(dims)  # (D,)
    kf = k.float()
    absmax = torch.zeros(k.shape[:-1] + (ngrp,), device=k.device)
    absmax.scatter_reduce_(-1, gidx.expand(kf.shape), kf.abs(),
                           reduce="amax", include_self=False)
    # E8M0 exponent: smallest power of two with absmax/2^e <= 448
    e = torch.ceil(torch.log2(absmax.clamp(min=1e-30) / _E4M3_MAX))
    e = torch.where(absmax > 0, e, torch.zeros_like(e))
    e = e.clamp(min=-127, max=127)
    scales = (e + 127).to(torch.uint8)
    factor = torch.pow(2.0, e)
    k8 = (kf / factor.gather(-1, gidx.expand(kf.shape))).to(
        torch.float8_e4m3fn)
    # flush e4m3 SUBNORMALS to zero: the hardware's scaled-MFMA path does
    # not honor fp8 subnormal inputs (measured: down-scaled groups showed
    # lse errors exactly at subnormal-contribution magnitude, up-scaled
    # groups were exact), so the format defines them away — they are
    # <= 2^-9 of their block max anyway.
    k8f = k8.float()
    k8 = torch.where(k8f.abs() < 2.0 ** -6, torch.zeros_like(k8f),
                     k8f).to(torch.float8_e4m3fn)
    return k8, scales


def dequantize_k_mx(k8: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """Exact dequantization (the oracle's view of the quantized cache)."""
    d = k8.shape[-1]
    dims = torch.arange(d, device=k8.device)
    gidx = mx_group_index(dims)
    factor = torch.pow(2.0, scales.float() - 127)
    return k8.float() * factor.gather(-1, gidx.expand(k8.shape))


def quantize_v_mx(v: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Quantize V (..., T, D): PV contracts over KEYS, so the scale groups
    run along the TOKEN axis — per dim, per 64-token window, the two
    interleaved sets {t: (t>>4)&1 == blk} (same silicon-pinned block
    structure as K's dims). Returns (v8, scales) with scales uint8 of
    shape (..., T//32, D) indexed by [token-group][dim], token-group =
    (t>>6)*2 + ((t>>4)&1). T must be a multiple of 64."""
    t = v.shape[-2]
    assert t % 64 == 0, "MX V quantization needs T a multiple of 64"
    v8t, st = quantize_k_mx(v.transpose(-1, -2).contiguous())
    return (v8t.transpose(-1, -2).contiguous(),
            st.transpose(-1, -2).contiguous())


def dequantize_v_mx(v8: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    return dequantize_k_mx(
        v8.transpose(-1, -2).contiguous(),
        scales.transpose(-1, -2).contiguous()).transpose(-1, -2).contiguous()
