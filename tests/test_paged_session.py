"""PagedDecodeSession on the CPU: the same stream as a RaggedDecodeSession
gives the same bits; a pool smaller than B x max_tokens serves a skewed
batch; pages return on reset and are reused; exhaustion and capacity raise
before anything moves."""

import os

import pytest
import torch
import torch.multiprocessing as mp

import paged_cases as pc
import ragged_cases as rc
from tree_attention_torch_amd.session import (PagedDecodeSession,
                                              RaggedDecodeSession)

LENGTHS = (1023, 0, 64, 513)


def _sessions(page, pool_tokens, block=256, max_tokens=rc.CAP - 256, **kw):
    common = dict(device="cpu", kv_dtype="fp32", block=block)
    paged = PagedDecodeSession(rc.B, rc.HKV, rc.D, max_tokens=max_tokens,
                               pool_tokens=pool_tokens, page=page, **common,
                               **kw)
    ragged = RaggedDecodeSession(rc.B, rc.HKV, rc.D, max_tokens=max_tokens,
                                 **common, **kw)
    return paged, ragged


def _feed(sessions, rg, lengths, tail=3):
    """Sequence b's first lengths[b] tokens: all but the last `tail` through
    prefill, the rest through masked appends (tests/test_gpu_ragged.py)."""
    ks, vs = rc.stream(rg)
    for sess in sessions:
        for b, n in enumerate(lengths):
            if n > tail:
                sess.prefill(b, ks[b, :, :n - tail], vs[b, :, :n - tail])
        while sess.totals != list(lengths):
            mask = [sess.totals[b] < lengths[b] for b in range(rc.B)]
            at = torch.tensor(sess.totals).clamp(max=rg.cap - 1)
            bi = torch.arange(rc.B)
            sess.append(ks[bi, :, at][:, :, None], vs[bi, :, at][:, :, None],
                        mask)
        assert sess.total_dev.tolist() == sess.totals == list(lengths)
        assert sess.local_len_dev.tolist() == sess.local_lens


def _pages(lengths, page):
    return [pc.pages_of(n, page) for n in lengths]


@pytest.mark.parametrize("page", pc.PAGES)
def test_paged_equals_ragged_and_pool_is_small(page):
    """8 (page 256) or 14 (page 128) pages serve (1023, 0, 64, 513): at
    most half of the slab's 4 x 1024 rows, and not one page to spare."""
    rg = pc.build(LENGTHS, "bf16", page)
    need = _pages(LENGTHS, page)
    paged, ragged = _sessions(page, pool_tokens=sum(need) * page)
    assert paged.page == page and paged.n_pages == sum(need)
    assert paged.n_pages * page <= rc.B * ragged.capacity // 2
    assert paged.capacity == ragged.capacity == rc.CAP
    assert paged.free_pages == paged.n_pages
    _feed((paged, ragged), rg, LENGTHS)
    assert paged.free_pages == 0
    assert [len(p) for p in paged._pages] == need
    assert paged.page_table.dtype == torch.int32
    for b, ids in enumerate(paged._pages):
        assert paged.page_table[b, :len(ids)].tolist() == ids
    q = rg.q.float()
    out = paged.attend(q)
    assert torch.equal(out, ragged.attend(q))
    rc.compare(rg, out, None, "PagedDecodeSession.attend (CPU)")
    assert not out[1].any()


def test_paged_reset_reuses_pages():
    page = 128
    rg = pc.build(LENGTHS, "bf16", page)
    need = _pages(LENGTHS, page)
    paged, _ = _sessions(page, pool_tokens=(sum(need) + 2) * page)
    _feed((paged,), rg, LENGTHS)
    assert paged.free_pages == 2
    old = list(paged._pages[0])
    assert len(old) == need[0] == 8
    paged.reset(0)
    assert paged.free_pages == 2 + need[0]
    assert paged.totals[0] == 0 and paged.local_lens[0] == 0
    assert paged.total_dev.tolist() == paged.totals
    # what row 0 left behind must not leak into the next tenant
    paged.k_pool[old] = 2.0 * rg.q[0, 0, 0].float()
    paged.v_pool[old] = float("nan")
    # the new sequence: row 3's 513 tokens, now in slot 0 as well
    lengths = (LENGTHS[3], 0, 64, 513)
    ks, vs = rc.stream(rg)
    paged.prefill(0, ks[3, :, :510], vs[3, :, :510])
    for t in range(510, 513):
        paged.append(ks[3:4, :, t:t + 1].expand(rc.B, -1, -1, -1),
                     vs[3:4, :, t:t + 1].expand(rc.B, -1, -1, -1),
                     [True, False, False, False])
    assert paged.totals == list(lengths)
    assert paged._pages[0] == old[:5]        # handed out again, in order
    assert paged.free_pages == 2 + need[0] - 5
    q = rg.q.float().clone()
    q[0] = q[3]
    out = paged.attend(q)
    assert torch.isfinite(out).all()
    assert torch.equal(out[0], out[3])
    want = torch.cat([rg.ref_out[3:4], rg.ref_out[1:]])
    torch.testing.assert_close(out, want, rtol=1e-5, atol=1e-5)


def _state(sess):
    return (list(sess.totals), list(sess.local_lens), sess.total_dev.tolist(),
            sess.local_len_dev.tolist(), sess.free_pages,
            [list(p) for p in sess._pages], sess.k_pool.clone(),
            sess.page_table.clone())


def _unchanged(sess, before):
    after = _state(sess)
    assert after[:6] == before[:6]
    assert torch.equal(after[6], before[6]) and torch.equal(after[7],
                                                            before[7])


def test_paged_pool_exhaustion_names_the_row():
    torch.manual_seed(2)
    sess = PagedDecodeSession(3, 2, 16, max_tokens=1024, pool_tokens=384,
                              page=128, device="cpu", kv_dtype="fp32",
                              block=64)
    assert sess.n_pages == 3 and sess.free_pages == 3
    k1 = torch.randn(3, 2, 1, 16)
    seq = torch.randn(2, 128, 16)
    sess.prefill(0, seq, seq)            # row 0: one full page
    sess.append(k1, k1, [False, True, True])
    assert sess.free_pages == 0
    before = _state(sess)
    # row 0 needs its second page, rows 1 and 2 have room on theirs
    with pytest.raises(RuntimeError, match=r"pool exhausted: row 0 "):
        sess.append(2 * k1, 2 * k1)
    _unchanged(sess, before)
    with pytest.raises(RuntimeError, match=r"pool exhausted: row 2 "):
        sess.prefill(2, seq, seq)        # 1 + 128 tokens: a second page
    _unchanged(sess, before)
    sess.append(k1, k1, [False, True, True])      # the others go on
    assert sess.totals == [128, 2, 2]
    sess.reset(1)
    assert sess.free_pages == 1
    sess.append(k1, k1, [True, False, False])     # row 0 takes row 1's page
    assert sess.totals == [129, 0, 2] and sess.free_pages == 0
    assert sess.total_dev.tolist() == sess.totals


def test_paged_capacity_names_the_row():
    torch.manual_seed(1)
    sess = PagedDecodeSession(2, 2, 16, max_tokens=64, pool_tokens=1024,
                              page=128, device="cpu", kv_dtype="fp32",
                              block=64)
    assert sess.capacity == 128          # 2 blocks of 64 = one page
    k1 = torch.randn(2, 2, 1, 16)
    seq = torch.randn(2, 128, 16)
    sess.prefill(1, seq, seq)
    sess.append(k1, k1, [True, False])
    before = _state(sess)
    with pytest.raises(RuntimeError, match=r"capacity exceeded: row 1 "):
        sess.append(2 * k1, 2 * k1)      # row 0 has room, row 1 has none
    _unchanged(sess, before)
    with pytest.raises(RuntimeError, match=r"row 1 "):
        sess.prefill(1, k1[0], k1[0])
    _unchanged(sess, before)
    sess.append(k1, k1, [True, False])
    assert sess.totals == [2, 128]
    with pytest.raises(ValueError, match="active"):
        sess.append(k1, k1, [True])


def test_paged_session_rejects_bad_arguments():
    for page in (0, 64, 100, 192, 2048):
        with pytest.raises(ValueError, match="page"):
            PagedDecodeSession(2, 2, 128, max_tokens=128, pool_tokens=4096,
                               page=page, device="cpu", kv_dtype="fp32")
    for name in ("mx", "fp8_mx"):
        with pytest.raises(ValueError, match="MX"):
            PagedDecodeSession(2, 2, 128, max_tokens=128, pool_tokens=4096,
                               device="cpu", kv_dtype=name, block=64)
    sess = PagedDecodeSession(2, 2, 128, max_tokens=128, pool_tokens=4096,
                              device="cpu", kv_dtype="fp32")
    assert sess.page == 256
    with pytest.raises(ValueError, match="GPU"):
        sess.graphed_step(torch.zeros(2, 2, 1, 128), torch.zeros(2, 2, 1, 128),
                          torch.zeros(2, 2, 1, 128))
    import tree_attention_torch_amd as ta

    assert ta.PagedDecodeSession is PagedDecodeSession


def _worker(rank, world, port):
    import sys

    import torch.distributed as dist

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        page = 128
        rg = pc.build(LENGTHS, "bf16", page)
        # block 64 over two ranks: each shard holds about half of every row,
        # and a block is half a page
        paged, ragged = _sessions(page, pool_tokens=1024, block=64,
                                  max_tokens=rc.CAP)
        _feed((paged, ragged), rg, LENGTHS)
        assert paged.local_lens == ragged.local_lens
        assert max(paged.local_lens) < 600
        assert paged.n_pages == 8 and paged.free_pages == \
            8 - sum(_pages(paged.local_lens, page))
        q = rg.q.float()
        for combine in ("allgather", "allreduce"):
            out = paged.attend(q, combine=combine)
            assert torch.equal(out, ragged.attend(q, combine=combine))
            rc.compare(rg, out, None, f"rank {rank} {combine}")
    finally:
        dist.destroy_process_group()


def test_paged_equals_ragged_ws2():
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 2, 29771))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
