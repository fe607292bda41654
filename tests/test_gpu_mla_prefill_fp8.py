"""fa_mla_prefill_fp8_kernel (ta.mla_prefill_paged and PagedMlaSession.
attend_prefill under compute="fp8") against ref64 over the dequantized rows
and the e4m3-rounded queries: both roundings are the declared format, so the
kernel is tested and the quantizers are not."""

import pytest
import torch

import tree_attention_torch_amd as ta
from mla_fp8_cases import deq, paged_fp8, spread
from mla_paged_cases import chain, check, ref64
from tree_attention_torch_amd.quant import dequantize_mla_fp8, quantize_mla_fp8

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def queries(*shape):
    # spread: a query scale from the wrong block is off by at least 2x
    return spread(torch.randn(*shape)).to(BF16)


def run(q, pool, table, lens, fn=None, **kw):
    if kw.get("vis") is not None:
        kw["vis"] = torch.tensor(kw["vis"]).cuda()
    if fn is None:
        fn, kw["compute"] = ta.mla_prefill_paged, "fp8"
    return fn(q.cuda(), pool.cuda(), table.cuda(), torch.tensor(lens).cuda(),
              **kw)


@pytest.mark.parametrize("hq,t,lens,page,kw", [
    (16, 9, [130, 300, 65], 128, {}),    # 144 rows: one block seam
    (40, 5, [130, 300, 65], 128, {"softmax_scale": 0.1352}),
    (128, 2, [130, 65], 128, {}),
    (16, 1, [130, 300, 65], 128, {}),    # fewer rows than a wave's 32
    (8, 70, [200], 128, {}),             # the diagonal crosses a tile
    (16, 65, [65], 128, {}),             # query 0 sees one key
    (40, 5, [130, 700, 65], 512, {}),
    # 128-key chunks: the early queries see no key of the later chunks
    (16, 40, [300, 260], 128, {"splits": 3, "max_pages": 3}),
])
def test_seams(hq, t, lens, page, kw):
    kw = dict(kw)
    rows, pool, table = paged_fp8(lens, page, seed=1,
                                  max_pages=kw.pop("max_pages", None))
    q = queries(len(lens), hq, t, 576)
    out, lse = run(q, pool, table, lens, **kw)
    check(out, lse,
          *ref64(deq(q), rows, chain(lens, t), kw.get("softmax_scale")))


def test_explicit_vis():
    lens, hq = [130, 300, 65], 16
    rows, pool, table = paged_fp8(lens, 128, seed=1)
    vis = [[7, 0, n + 9, 64, 65, 128, 129, n, 1] for n in lens]
    q = queries(3, hq, 9, 576)
    out, lse = run(q, pool, table, lens, vis=vis)
    want = [[min(v, n) for v in r] for r, n in zip(vis, lens)]
    assert (out[:, :, 1] == 0).all() and (lse[:, :, 1] == -float("inf")).all()
    check(out, lse, *ref64(deq(q), rows, want))


@pytest.mark.parametrize("must_see", [False, True])
def test_needles(must_see):
    # test_gpu_mla_prefill.test_needles over the fp8_block rows: the query of
    # a needle position is the (dequantized) row at, or one short of, its limit
    hq, t, at = 16, 24, [0, 7, 8, 23]
    vis = [100] * t
    for pos, v in zip(at, [64, 65, 128, 129]):
        vis[pos] = v
    rows, pool, table = paged_fp8([200], 128, seed=2)
    j = torch.tensor(vis) - int(must_see)
    q = rows[0][j][None, None].expand(1, hq, t, 576).to(BF16).contiguous()
    out, lse = run(q, pool, table, [200], vis=[vis])
    check(out, lse, *ref64(deq(q), rows, [vis]))
    if must_see:   # the needle scores tens, the rest ~N(0, 1)
        check(out[:, :, at], None,
              rows[0][j[at], :512].double().expand(1, hq, 4, 512), None)


@pytest.mark.parametrize("t", [4, 16])
def test_agrees_with_decode(t):
    # The fp8_block decode path rounds nothing of q: give it the rounded
    # queries, cast to bf16. With a block scale amax / 448 that cast rounds
    # every column by up to 2^-9 again, which alone moved one lse of 1920 by
    # 0.0082 (0.0057 allowed) at t = 16 while the kernel met ref64. So the
    # queries' block scales are snapped to powers of two first: e4m3 times
    # 2^k is a bf16 value and its block maximum is 448 * 2^k, so the cast is
    # exact, the kernel's rounding is the identity and both kernels see the
    # same numbers.
    lens = [130, 300, 65]
    rows, pool, table = paged_fp8(lens, 128, seed=3)
    q8 = quantize_mla_fp8(queries(3, 40, t, 576))
    sc = q8[..., 512:528].contiguous().view(torch.float32)
    q8[..., 512:528] = (2.0 ** sc.log2().round()).view(torch.uint8)
    q = dequantize_mla_fp8(q8).to(BF16)
    assert torch.equal(q.float(), deq(q))
    out, lse = run(q, pool, table, lens)
    do, dl = run(q, pool, table, lens, fn=ta.mla_decode_paged)
    check(out, lse, do.double().cpu(), dl.double().cpu())


def test_session():
    g = torch.Generator().manual_seed(5)
    new = lambda *s: torch.randn(*s, generator=g).to(BF16)
    sess = ta.PagedMlaSession(2, 600, page=128, dtype="fp8_block")
    rows = spread(new(200, 576))
    sess.prefill(1, rows[:130].cuda())
    sess.prefill(1, rows[130:].cuda())
    q1 = new(2, 16, 1, 576)
    before = sess.attend(q1.cuda())
    state = (list(sess.totals), sess.free_pages, sess.local_len_dev.clone(),
             sess.pool.clone())
    q = spread(new(16, 70, 576))
    out = sess.attend_prefill(1, q.cuda(), compute="fp8")
    assert out.shape == (1, 16, 70, 512)
    check(out, None,
          ref64(deq(q)[None], [deq(rows)], chain([200], 70))[0], None)
    assert state[:2] == (list(sess.totals), sess.free_pages)
    assert torch.equal(state[2], sess.local_len_dev)
    assert torch.equal(state[3], sess.pool)
    assert torch.equal(before, sess.attend(q1.cuda()))
    bf16 = ta.PagedMlaSession(1, 300, page=128)
    bf16.prefill(0, rows[:40].cuda())
    with pytest.raises(ValueError):
        bf16.attend_prefill(0, q[:, :20].cuda(), compute="fp8")
