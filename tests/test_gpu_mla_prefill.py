"""fa_mla_prefill_kernel (ta.mla_prefill_paged, PagedMlaSession.attend_prefill)
against an fp64 masked softmax gathered through the page table on the host."""

import pytest
import torch

import tree_attention_torch_amd as ta
from mla_paged_cases import chain, check, paged, ref64

pytestmark = pytest.mark.gpu

BF16, FP16 = torch.bfloat16, torch.float16


def run(q, pool, table, lens, fn=None, **kw):
    if kw.get("vis") is not None:
        kw["vis"] = torch.tensor(kw["vis"]).cuda()
    return (fn or ta.mla_prefill_paged)(q.cuda(), pool.cuda(), table.cuda(),
                                        torch.tensor(lens).cuda(), **kw)


@pytest.mark.parametrize("hq,t,lens,dtype,page,kw", [
    (16, 9, [130, 300, 65], BF16, 128, {}),    # 144 rows: one block seam
    (16, 9, [130, 300, 65], FP16, 128, {}),
    (40, 5, [130, 300, 65], BF16, 128, {"softmax_scale": 0.1352}),
    (128, 2, [130, 65], BF16, 128, {}),
    (16, 1, [130, 300, 65], BF16, 128, {}),    # fewer rows than a wave's 32
    (8, 70, [200], BF16, 128, {}),             # the diagonal crosses a tile
    (16, 65, [65], BF16, 128, {}),             # query 0 sees one key
    (40, 5, [130, 700, 65], BF16, 512, {}),
    # 128-key chunks: the early queries see no key of the later chunks
    (16, 40, [130, 140], BF16, 128, {"splits": 2, "max_pages": 2}),
    (16, 40, [300, 260], BF16, 128, {"splits": 3, "max_pages": 3}),
])
def test_seams(hq, t, lens, dtype, page, kw):
    kw = dict(kw)
    rows, pool, table = paged(lens, page, dtype, seed=1,
                              max_pages=kw.pop("max_pages", None))
    q = torch.randn(len(lens), hq, t, 576).to(dtype)
    out, lse = run(q, pool, table, lens, **kw)
    check(out, lse, *ref64(q, rows, chain(lens, t), kw.get("softmax_scale")))


def test_explicit_vis():
    # what a rank holding a slice sees: non-monotone, a blind query, one past
    # the length, tile and page seams
    lens, hq = [130, 300, 65], 16
    rows, pool, table = paged(lens, 128, seed=1)
    vis = [[7, 0, n + 9, 64, 65, 128, 129, n, 1] for n in lens]
    q = torch.randn(3, hq, 9, 576).to(BF16)
    out, lse = run(q, pool, table, lens, vis=vis)
    want = [[min(v, n) for v in r] for r, n in zip(vis, lens)]
    assert (out[:, :, 1] == 0).all() and (lse[:, :, 1] == -float("inf")).all()
    check(out, lse, *ref64(q, rows, want))


@pytest.mark.parametrize("must_see", [False, True])
def test_needles(must_see):
    # test_gpu_mla_paged.test_needles with the four needles at positions 0, 7,
    # 8 and 23 of 24 (Hq 16: rows 0, 112, 128 and 368, in different waves'
    # and blocks' ranges); the padding positions see 100 keys
    hq, t, at = 16, 24, [0, 7, 8, 23]
    vis = [100] * t
    for pos, v in zip(at, [64, 65, 128, 129]):
        vis[pos] = v
    rows, pool, table = paged([200], 128, seed=2)
    j = torch.tensor(vis) - int(must_see)
    q = rows[0][j][None, None].expand(1, hq, t, 576).contiguous()
    out, lse = run(q, pool, table, [200], vis=[vis])
    check(out, lse, *ref64(q, rows, [vis]))
    if must_see:   # the needle scores ~24, the rest ~N(0, 1)
        check(out[:, :, at], None,
              rows[0][j[at], :512].double().expand(1, hq, 4, 512), None)


@pytest.mark.parametrize("t", [4, 16])
def test_agrees_with_decode(t):
    lens = [130, 300, 65]
    rows, pool, table = paged(lens, 128, seed=3)
    q = torch.randn(3, 40, t, 576).to(BF16)
    out, lse = run(q, pool, table, lens)
    do, dl = run(q, pool, table, lens, fn=ta.mla_decode_paged)
    check(out, lse, do.double().cpu(), dl.double().cpu())


def test_session():
    g = torch.Generator().manual_seed(5)
    new = lambda *s: torch.randn(*s, generator=g).to(BF16)
    sess = ta.PagedMlaSession(2, 600, page=128)
    mirror = new(200, 576)
    sess.prefill(1, mirror[:130].cuda())
    sess.prefill(1, mirror[130:].cuda())
    q1 = new(2, 16, 1, 576)
    before = sess.attend(q1.cuda())
    state = (list(sess.totals), sess.free_pages, sess.local_len_dev.clone())
    q = new(16, 70, 576)
    out = sess.attend_prefill(1, q.cuda())
    assert out.shape == (1, 16, 70, 512)
    check(out, None, ref64(q[None], [mirror], chain([200], 70))[0], None)
    assert state[:2] == (list(sess.totals), sess.free_pages)
    assert torch.equal(state[2], sess.local_len_dev)
    assert torch.equal(before, sess.attend(q1.cuda()))


def test_fp8_block_refused():
    sess = ta.PagedMlaSession(1, 300, page=128, dtype="fp8_block")
    sess.prefill(0, torch.randn(40, 576).to(BF16).cuda())
    q = torch.randn(1, 16, 20, 576).to(BF16).cuda()
    with pytest.raises(NotImplementedError):
        sess.attend_prefill(0, q)
    with pytest.raises(NotImplementedError):
        ta.mla_prefill_paged(q, sess.pool, sess.page_table, sess.local_len_dev)
