"""fa_mla_decode_kernel over the fp8_block pool and mla_append_quant_kernel
against an fp64 masked softmax over the dequantized rows."""

import pytest
import torch

import tree_attention_torch_amd as ta
from mla_fp8_cases import paged_fp8, session_walk, spread
from mla_paged_cases import chain, check, ref64
from tree_attention_torch_amd.quant import quantize_mla_fp8
from tree_attention_torch_amd.session import _n_local, _place

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
LENS = [0, 1, 64, 65, 128, 129, 257, 1000]


def run(q, pool, table, lens, **kw):
    if kw.get("vis") is not None:
        kw["vis"] = torch.tensor(kw["vis"]).cuda()
    return ta.mla_decode_paged(q.cuda(), pool.cuda(), table.cuda(),
                               torch.tensor(lens).cuda(), **kw)


@pytest.mark.parametrize("hq,page", [(16, 128), (40, 128), (128, 128), (40, 512)])
def test_seams(hq, page):
    rows, pool, table = paged_fp8(LENS, page)
    q = torch.randn(len(LENS), hq, 1, 576).to(BF16)
    out, lse = run(q, pool, table, LENS)
    assert (out[0] == 0).all() and (lse[0] == -float("inf")).all()
    check(out, lse, *ref64(q, rows))


@pytest.mark.parametrize("explicit", [False, True])
@pytest.mark.parametrize("hq,tq,lens,kw", [
    (16, 2, [130, 300, 65], {}),
    (40, 5, [130, 300, 65], {}),
    (128, 3, [130, 65], {}),
    # two 128-key chunks: queries 0 and 1 see no key of the second
    (16, 4, [130, 130], {"splits": 2, "max_pages": 2}),
])
def test_multi_token(hq, tq, lens, kw, explicit):
    kw = dict(kw)
    rows, pool, table = paged_fp8(lens, 128, seed=1,
                                  max_pages=kw.pop("max_pages", None))
    q = torch.randn(len(lens), hq, tq, 576).to(BF16)
    vis = [([7, 0, n + 9, 64, 128][:tq]) for n in lens] if explicit else None
    out, lse = run(q, pool, table, lens, vis=vis, **kw)
    want = [[min(v, n) for v in r] for r, n in zip(vis, lens)] if explicit \
        else chain(lens, tq)
    check(out, lse, *ref64(q, rows, want))


def test_session():
    session_walk("cuda")


def test_graphed_step():
    g = torch.Generator().manual_seed(3)
    new = lambda *s: spread(torch.randn(*s, generator=g).to(BF16)).cuda()
    eager, graphed = (ta.PagedMlaSession(2, 500, page=128, dtype="fp8_block")
                      for _ in range(2))
    for b, n in enumerate((126, 10)):
        r = new(n, 576)
        eager.prefill(b, r)
        graphed.prefill(b, r)
    q_static, c_static = new(2, 16, 1, 576), new(2, 1, 1, 576)
    replay = graphed.graphed_step(q_static, c_static)
    for active in (None, [True, False], None):   # the third lands on a new page
        q, c = new(2, 16, 1, 576), new(2, 1, 1, 576)
        q_static.copy_(q)
        c_static.copy_(c)
        eager.append(c, active)
        assert torch.equal(replay(active), eager.attend(q))
    assert graphed.totals == eager.totals == [129, 12]
    assert torch.equal(graphed.local_len_dev, eager.local_len_dev)
    assert torch.equal(graphed.pool, eager.pool)


def test_pool_append_sharded():
    ext = ta.ops.flash._load_extension()
    block, rank, world, page, T = 64, 1, 2, 128, 4
    totals, counts = [62, 100, 190], [4, 0, 3]   # rank 1 owns 64, 65 and 192
    pool = torch.full((4, 1, page, 656), 0xFF, dtype=torch.uint8)
    table = torch.tensor([[2], [0], [3]], dtype=torch.int32)
    c_new = spread(torch.randn(3, 1, T, 576).to(BF16))
    c_new[0, 0, 2, :128] = 0      # a zero block: the floor scale
    total = torch.tensor(totals).cuda()
    local = torch.tensor([_n_local(t, block, rank, world) for t in totals]).cuda()
    vis = torch.zeros(3, T, dtype=torch.long).cuda()
    pool_d = pool.cuda()
    ext.mla_pool_append_quant(pool_d, table.cuda(), c_new.cuda(), total, local,
                              torch.tensor(counts, dtype=torch.int32).cuda(),
                              vis, block, rank, world)
    want_vis = []
    for b, (t0, c) in enumerate(zip(totals, counts)):
        for i in range(c):
            owner, pos = _place(t0 + i, block, world)
            if owner == rank:
                pool[table[b, pos // page], 0, pos % page] = \
                    quantize_mla_fp8(c_new[b, 0, i])
        want_vis.append([_n_local(t0 + (min(i, c - 1) + 1 if c else 0), block,
                                  rank, world) for i in range(T)])
    assert total.tolist() == [t + c for t, c in zip(totals, counts)]
    assert local.tolist() == [_n_local(t + c, block, rank, world)
                              for t, c in zip(totals, counts)]
    assert vis.tolist() == want_vis
    assert torch.equal(pool_d.cpu(), pool)
