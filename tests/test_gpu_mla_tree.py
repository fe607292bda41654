"""fa_mla_decode_kernel under an ancestor mask, the tree append and commit
kernels of the MLA pool, and the session's tree step, against fp64 and the
host formulas."""

import pytest
import torch

import tree_attention_torch_amd as ta
from mla_fp8_cases import paged_fp8
from mla_paged_cases import check, paged
from mla_tree_cases import ref64_tree, tree_walk
from tree_attention_torch_amd.quant import quantize_mla_fp8
from tree_attention_torch_amd.session import _n_local, _place, _tree_masks

pytestmark = pytest.mark.gpu

BF16, FP16 = torch.bfloat16, torch.float16
BASES = [0, 63, 64, 65, 127, 128, 129]   # pool start, tile seam, page seam
# explicit, non-monotone: blind (on base 0: sees nothing), slot 15 alone, bits
# above 15 (ignored), siblings 1 and 2 under node 0, then anything
MASKS = [0, 1 << 15, 0x7FFF0000 | 0b0110, 0b0011, 0b0101, 0xFFFF, 0x8002,
         0b1, 0x0F0F, 0x4000, 0x00FF, 0xAAAA, 0x5555, 0x0180, 0xC001, 0x0008]


def run(q, pool, table, lens, bases, masks, **kw):
    tree = (torch.tensor(bases).cuda(),
            torch.tensor(masks, dtype=torch.int32).cuda())
    return ta.mla_decode_paged(q.cuda(), pool.cuda(), table.cuda(),
                               torch.tensor(lens).cuda(), tree=tree, **kw)


@pytest.mark.parametrize("hq,tq,bases,extra,kind,page,kw", [
    (5, 3, BASES, 16, BF16, 128, {}),          # 15 rows: HB 16, four key waves
    (4, 7, BASES, 16, FP16, 128, {}),          # 28 rows: HB 32, two key waves
    (16, 3, BASES, 16, BF16, 128, {}),
    (40, 7, BASES, 16, FP16, 128, {}),
    (128, 16, [0, 65, 129], 16, BF16, 128, {}),
    (5, 3, BASES, 16, "fp8", 128, {}),
    (4, 7, BASES, 16, "fp8", 128, {}),
    (16, 16, BASES, 16, "fp8", 128, {}),
    (40, 3, [63, 128, 500], 16, BF16, 512, {}),
    # two 128-key chunks. Base 120: slots 8..15 lie in chunk 1, rel = -8.
    # Base 105: rows 121..139 are slots >= 16, dead in both chunks (rel = -23)
    (16, 7, [120, 105], [16, 35], BF16, 128, {"splits": 2, "max_pages": 2}),
    (16, 7, [120, 105], [16, 35], "fp8", 128, {"splits": 2, "max_pages": 2}),
])
def test_tree_mask(hq, tq, bases, extra, kind, page, kw):
    kw = dict(kw)
    extra = extra if isinstance(extra, list) else [extra] * len(bases)
    lens = [b + e for b, e in zip(bases, extra)]
    make = paged_fp8 if kind == "fp8" else \
        (lambda *a, **k: paged(a[0], a[1], kind, **k))
    rows, pool, table = make(lens, page, seed=4,
                             max_pages=kw.pop("max_pages", None))
    q = torch.randn(len(lens), hq, tq, 576).to(BF16 if kind == "fp8" else kind)
    masks = [MASKS[:tq]] * len(lens)
    out, lse = run(q, pool, table, lens, bases, masks, **kw)
    if bases[0] == 0:   # the blind row: exact
        assert (out[0, :, 0] == 0).all() and (lse[0, :, 0] == -float("inf")).all()
    check(out, lse, *ref64_tree(q, rows, bases, masks))


@pytest.mark.parametrize("hq", [5, 64])
@pytest.mark.parametrize("must_see", [False, True])
def test_needles(hq, must_see):
    # q[h, t] is the draft at slot s[t]: it scores ~24, the rest ~N(0, 1). The
    # mask admits that slot alone, or omits it alone: a mask applied one slot
    # off changes the output by ~|row|. Slots 7 / 8 straddle the page seam.
    base, s = 120, torch.tensor([0, 7, 8, 15])
    rows, pool, table = paged([136], 128, seed=2)
    q = rows[0][base + s][None, None].expand(1, hq, 4, 576).contiguous()
    masks = [[(1 << int(i)) if must_see else 0xFFFF ^ (1 << int(i)) for i in s]]
    out, lse = run(q, pool, table, [136], [base], masks)
    ro, rl = ref64_tree(q, rows, [base], masks)
    want = rows[0][base + s, :512].double().expand(1, hq, 4, 512)
    assert ((ro - want).abs().max() < 1e-4) == must_see   # the case bites
    check(out, lse, ro, rl)


def test_chain_as_tree():
    lens, tq = [130, 300, 65], 5
    rows, pool, table = paged(lens, 128, seed=1)
    q = torch.randn(3, 40, tq, 576).to(BF16)
    chain = [[(2 << i) - 1 for i in range(tq)]] * 3   # parents[j] = j - 1
    out, lse = run(q, pool, table, lens, [n - tq for n in lens], chain)
    co, cl = ta.mla_decode_paged(q.cuda(), pool.cuda(), table.cuda(),
                                 torch.tensor(lens).cuda())
    check(out, lse, co.double().cpu(), cl.double().cpu())


@pytest.mark.parametrize("quant", [False, True])
def test_pool_append_commit_sharded(quant):
    ext = ta.ops.flash._load_extension()
    block, rank, world, page, T = 64, 1, 2, 128, 6
    totals, counts = [62, 100, 190, 126], [6, 0, 4, 5]  # rank 1: 64.., 192.., -
    parents = [[-1, 0, 0, 1, 3, 2], [-1] * 6, [-1, -1, 1, 9, 0, 0],  # 9: clamped
               [-1, 0, 1, 1, 2, 0]]
    pool = torch.full((4, 1, page, 656 if quant else 1152), 0xFF,
                      dtype=torch.uint8)
    pool = pool if quant else pool.view(BF16)
    table = torch.tensor([[2], [0], [3], [1]], dtype=torch.int32)
    c_new = torch.randn(4, 1, T, 576).to(BF16)
    stored = quantize_mla_fp8(c_new) if quant else c_new
    dev = lambda x, dt=torch.int32: torch.tensor(x, dtype=dt).cuda()
    total = dev(totals, torch.long)
    local = dev([_n_local(t, block, rank, world) for t in totals], torch.long)
    base, mask = dev([0] * 4, torch.long), dev([[0] * T] * 4)
    pool_d, table_d, c_d, counts_d = pool.cuda(), table.cuda(), c_new.cuda(), dev(counts)
    (ext.mla_pool_append_tree_quant if quant else ext.mla_pool_append_tree)(
        pool_d, table_d, c_d, total, local, counts_d, dev(parents), base, mask,
        block, rank, world)

    def place(b, t, src):
        owner, pos = _place(t, block, world)
        if owner == rank:
            pool[table[b, pos // page], 0, pos % page] = stored[b, 0, src]

    for b, (t0, c) in enumerate(zip(totals, counts)):
        for i in range(c):
            place(b, t0 + i, i)
    want = [_tree_masks(t0, c, p, T, block, rank, world)
            for t0, c, p in zip(totals, counts, parents)]
    ends = [t + c for t, c in zip(totals, counts)]
    assert base.tolist() == [w[0] for w in want]
    assert mask.tolist() == [w[1] for w in want]
    assert total.tolist() == ends
    assert local.tolist() == [_n_local(t, block, rank, world) for t in ends]
    assert torch.equal(pool_d.cpu().view(torch.uint8), pool.view(torch.uint8))
    # keep paths that skip nodes; row 2 keeps nothing, row 1 had nothing
    paths, keep = [[0, 2, 5, 0, 0, 0], [0] * 6, [0] * 6, [1, 3, 4, 0, 0, 0]], \
        [3, 0, 0, 3]
    (ext.mla_pool_commit_path_quant if quant else ext.mla_pool_commit_path)(
        pool_d, table_d, c_d, total, local, counts_d, dev(paths), dev(keep),
        block, rank, world)
    for b, (t0, n) in enumerate(zip(totals, keep)):
        for i in range(n):
            place(b, t0 + i, paths[b][i])
    ends = [t + n for t, n in zip(totals, keep)]
    assert total.tolist() == ends
    assert local.tolist() == [_n_local(t, block, rank, world) for t in ends]
    assert torch.equal(pool_d.cpu().view(torch.uint8), pool.view(torch.uint8))


@pytest.mark.parametrize("dtype", ["bf16", "fp8_block"])
def test_session(dtype):
    tree_walk("cuda", dtype)


@pytest.mark.parametrize("dtype", ["bf16", "fp8_block"])
def test_graphed_step_tree(dtype):
    g = torch.Generator().manual_seed(3)
    new = lambda *s: torch.randn(*s, generator=g).to(BF16).cuda()
    eager, graphed = (ta.PagedMlaSession(2, 500, page=128, dtype=dtype)
                      for _ in range(2))
    for b, n in enumerate((125, 10)):
        r = new(n, 576)
        eager.prefill(b, r)
        graphed.prefill(b, r)
    q_static, c_static = new(2, 16, 4, 576), new(2, 1, 4, 576)
    p_static = torch.zeros(2, 4, dtype=torch.int32).cuda()
    replay = graphed.graphed_step_tree(q_static, c_static, p_static)
    steps = [([4, 2], [[-1, 0, 0, 2], [-1, -1, 0, 0]], [[0, 2, 3], [1]]),
             ([3, 4], [[-1, -1, 1, 0], [-1, 0, 1, 2]], [[1, 2], [0, 1, 2, 3]])]
    for counts, parents, paths in steps:   # the first crosses onto a new page
        q, c = new(2, 16, 4, 576), new(2, 1, 4, 576)
        q_static.copy_(q)
        c_static.copy_(c)
        p_static.copy_(torch.tensor(parents, dtype=torch.int32))
        eager.append_tree(c, parents, counts)
        assert torch.equal(replay(counts), eager.attend_tree(q))
        for sess in (eager, graphed):
            sess.commit(paths, [len(p) for p in paths])
        assert torch.equal(graphed.local_len_dev, eager.local_len_dev)
        assert torch.equal(graphed.pool, eager.pool)
    assert graphed.totals == eager.totals == [130, 15]
