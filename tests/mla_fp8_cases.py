"""fp8_block latent pools and a session walk for the MLA fp8 tests (GPU and
CPU): the reference is ref64 over the DEQUANTIZED rows, so the kernel is
tested and the quantizer is not."""

import torch

import tree_attention_torch_amd as ta
from mla_paged_cases import check, paged, ref64
from tree_attention_torch_amd.quant import dequantize_mla_fp8, quantize_mla_fp8


def spread(rows, first_key=0):
    """Latent block j of key k times 2^((k + 3j) % 5 - 3): the four blocks of
    a key and the same block of neighbouring keys all differ, so a scale from
    the wrong block or the wrong key is off by at least 2x. The largest
    factor is 2: P is rounded to bf16 (2^-9 relative) in this kernel as in
    the bf16 one, which puts up to 2^-9 * max|v| on an output, and the 0.025
    of BARS["half"] allows that for |v| < 12.8, i.e. randn rows (|x| < 5)
    times 2. Under the 2^4 of a wider spread the same rounding reaches
    0.035 on one output in 65536."""
    key = torch.arange(first_key, first_key + rows.shape[-2])[:, None]
    e = (key + 3 * torch.arange(4)[None, :]) % 5 - 3
    f = torch.cat([(2.0 ** e).repeat_interleave(128, 1),
                   torch.ones(len(key), 64)], 1)
    return (rows.float() * f).to(rows.dtype)


def deq(rows):
    return dequantize_mla_fp8(quantize_mla_fp8(rows))


def paged_fp8(lens, page, seed=0, max_pages=None):
    """paged() with spread rows in a uint8 pool, 0xFF (NaN as e4m3, fp32 and
    bf16) wherever nothing may be read; returns the dequantized rows."""
    rows, pool, table = paged(lens, page, seed=seed, max_pages=max_pages)
    rows = [spread(r) for r in rows]
    pool8 = torch.full((pool.shape[0], 1, page, 656), 0xFF, dtype=torch.uint8)
    for b, r in enumerate(rows):
        for j in range(-(-len(r) // page)):
            part = r[j * page : (j + 1) * page]
            pid = int(table[b, j].clamp(0, pool.shape[0] - 1))
            pool8[pid, 0, : len(part)] = quantize_mla_fp8(part)
    return [deq(r) for r in rows], pool8, table


def session_walk(device):
    """mla_paged_cases.session_walk under dtype="fp8_block": every step
    against ref64 over a host mirror of dequantized rows."""
    g = torch.Generator().manual_seed(5)
    new = lambda *s: torch.randn(*s, generator=g).bfloat16()
    sess = ta.PagedMlaSession(3, 600, page=128, n_pages=8, dtype="fp8_block",
                              device=device)
    assert sess.pool.dtype == torch.uint8 and sess.pool.shape[-1] == 656
    rows = [spread(new(n, 576)) for n in (130, 5, 250)]
    for b, r in enumerate(rows):
        sess.prefill(b, r.to(device))
    mirror = [deq(r) for r in rows]

    def attend(tq, vis=None):
        q = new(3, 16, tq, 576)
        fn = sess.attend if tq == 1 else sess.attend_many
        check(fn(q.to(device)), None, ref64(q, mirror, vis)[0], None)

    attend(1)
    for active in (None, [True, False, True]):
        c = spread(new(3, 1, 1, 576), 3)
        sess.append(c.to(device), active)
        for b in range(3):
            if active is None or active[b]:
                mirror[b] = torch.cat([mirror[b], deq(c[b, 0])])
        attend(1)
    c, counts = spread(new(3, 1, 3, 576), 7), [3, 0, 2]
    before = [len(r) for r in mirror]
    sess.append_many(c.to(device), counts)
    mirror = [torch.cat([r, deq(c[b, 0, :n])])
              for b, (r, n) in enumerate(zip(mirror, counts))]
    attend(3, [[t0 + (min(i, n - 1) + 1 if n else 0) for i in range(3)]
               for t0, n in zip(before, counts)])
    sess.truncate(0, before[0] + 1)     # one draft of row 0 accepted
    mirror[0] = mirror[0][: before[0] + 1]
    attend(1)
    free = sess.free_pages
    sess.reset(2)
    assert sess.free_pages > free
    r2 = spread(new(140, 576))
    sess.prefill(2, r2.to(device))
    mirror[2] = deq(r2)
    assert sess.totals == [len(r) for r in mirror]
    attend(1)
