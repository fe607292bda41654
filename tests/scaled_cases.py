"""The "fp8_scaled" tests' inputs: K row j is randn * 2^((5 j) % 13 - 6), V row
j randn * 2^((7 j) % 13 - 6), one row per sequence near +-3000 in both."""

import torch

from tree_attention_torch_amd.quant import dequantize_rows_fp8
from tree_attention_torch_amd import session as S

B, HKV, D = 4, 2, 128
LENS = (0, 1, 129, 700)
OUTLIER_AT = 3          # local position of the outlier row
# Keys q scores ~4 on. 129: V scales 2^-5, 2^5; other keys of K scale >= 2
# nulled. 700 (more of those than q has dimensions): the largest K rows.
TARGETS = {129: [2, 15, 28, 41, 54, 9, 22, 35, 48, 61],
           700: [5, 135, 265, 525, 655, 10, 140, 270, 530, 660]}


def make_kv():
    g, seqs = torch.Generator().manual_seed(0), []
    for n in LENS:
        j = torch.arange(n).view(1, n, 1)
        k = torch.randn(HKV, n, D, generator=g) * 2.0 ** ((5 * j) % 13 - 6)
        v = torch.randn(HKV, n, D, generator=g) * 2.0 ** ((7 * j) % 13 - 6)
        for t in (k, v) if n > OUTLIER_AT else ():
            t[:, OUTLIER_AT] = torch.randn(HKV, D, generator=g).sign() * (
                3000 + 100 * torch.rand(HKV, D, generator=g))
        seqs.append((k.bfloat16(), v.bfloat16()))
    return seqs


def make_q(seqs, g_heads: int) -> torch.Tensor:
    """(B, Hkv * G, 1, D) bf16 that the kernel's per-row e4m3 quantization
    reproduces exactly (e4m3 values, the largest 448, times a power of two):
    kernel and reference read one query. Before that rounding, which moves
    the outlier's score by tens of units, a head's q is the minimum-norm
    vector scoring ~4 on its TARGETS and -600 on the outlier."""
    g = torch.Generator().manual_seed(1)
    q = torch.randn(B, HKV * g_heads, 1, D, generator=g).double()
    for b, (k, _) in enumerate(seqs):
        n = k.shape[1]
        for h in range(HKV * g_heads if n in TARGETS else 0):
            kk, j = k[h // g_heads].double(), torch.arange(n)
            null = ((5 * j) % 13 - 6 >= 1) & (n == 129)
            null[TARGETS[n] + [OUTLIER_AT]] = False
            a = torch.cat([kk[TARGETS[n]], kk[null], kk[OUTLIER_AT][None]])
            rhs = torch.zeros(a.shape[0], dtype=torch.float64)
            rhs[:10] = (4 + 0.5 * torch.randn(10, generator=g)) * D ** 0.5
            rhs[-1] = -600.0 * D ** 0.5
            q[b, h, 0] = torch.linalg.pinv(a) @ rhs
    amax = q.abs().amax(-1, keepdim=True)
    step = 2.0 ** torch.round(torch.log2(amax / 448))
    grid = (q * (448 * step / amax) / step).float().to(torch.float8_e4m3fn)
    return (grid.double() * step).bfloat16()


def attention_f64(q: torch.Tensor, rows):
    """q (B, Hq, 1, D), rows[b] = K, V (Hkv, n, D) -> out, probs[b] (Hq, n)"""
    out = torch.zeros(q.shape, dtype=torch.float64)
    probs = []
    for b, (k, v) in enumerate(rows):
        g_heads = q.shape[1] // k.shape[0]
        kk = k.double().repeat_interleave(g_heads, 0)
        s = torch.einsum("hd,hnd->hn", q[b, :, 0].double(), kk) * D ** -0.5
        probs.append(torch.softmax(s, dim=-1))   # (an empty row: out = 0)
        out[b, :, 0] = torch.einsum(
            "hn,hnd->hd", probs[-1], v.double().repeat_interleave(g_heads, 0))
    return out, probs


def check_spread(probs) -> None:
    # keys over 1 %: 129: >= 8, V scales span 2^10; 700: in and past [128, 512)
    for p in probs:
        j = torch.arange(p.shape[1])
        for h in range(p.shape[0]):
            big = (p[h] > 0.01) & (j != OUTLIER_AT)
            if p.shape[1] == 129:
                vexp = ((7 * j) % 13 - 6)[big]
                assert big.sum() >= 8 and vexp.max() - vexp.min() >= 10, h
            if p.shape[1] == 700:
                assert big[128:512].any() and big[512:].any(), h


def session(kind, kv_dtype="fp8_scaled", device="cpu"):
    kw = {"device": device, "kv_dtype": kv_dtype}
    return (S.RaggedDecodeSession(B, HKV, D, 1024, **kw) if kind == "slab" else
            S.PagedDecodeSession(B, HKV, D, 1024, 4096, page=kind, **kw))


def fill(sess, seqs):
    # all but each sequence's last token by prefill, the last by append
    k_new = torch.zeros(B, HKV, 1, D, dtype=torch.bfloat16)
    v_new = torch.zeros_like(k_new)
    for b, (k, v) in enumerate(seqs):
        n = k.shape[1]
        if n > 1:
            sess.prefill(b, k[:, : n - 1], v[:, : n - 1])
        if n:
            k_new[b, :, 0], v_new[b, :, 0] = k[:, n - 1], v[:, n - 1]
    sess.append(k_new.to(sess.device), v_new.to(sess.device),
                active=[n > 0 for n in LENS])


def stored(sess, b, n):
    """(K bytes, K scales, V bytes, V scales) of row b's first n positions."""
    if hasattr(sess, "k_pool"):
        idx = torch.tensor(sess._pages[b][: -(-n // sess.page)],
                           dtype=torch.long, device=sess.device)
        ts = (sess.k_pool, sess.k_scale, sess.v_pool, sess.v_scale)
        ts = [t.index_select(0, idx).transpose(0, 1).flatten(1, 2) for t in ts]
    else:
        ts = [t[b] for t in (sess.k, sess.k_scale, sess.v, sess.v_scale)]
    return [t[:, :n].cpu() for t in ts]


def stored_rows(sess):
    got = [stored(sess, b, n) for b, n in enumerate(sess.local_lens)]
    return [(dequantize_rows_fp8(k8, ks), dequantize_rows_fp8(v8, vs))
            for k8, ks, v8, vs in got]
