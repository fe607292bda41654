"""fork() on the CPU (fp32 storage): a forked PagedDecodeSession gives the
bits of one whose rows were prefilled independently and of the slab session
driven through fork(); pages are counted, shared, copied on the first write
and returned by the last holder; exhaustion and bad arguments raise before
anything moves. The scenario is tests/fork_cases.py."""

import os

import pytest
import torch
import torch.multiprocessing as mp

import fork_cases as fc
import paged_cases as pc
import ragged_cases as rc
from tree_attention_torch_amd.session import (PagedDecodeSession,
                                              RaggedDecodeSession, _n_local)


def _paged(page, n_pages=None, **kw):
    kw = dict(dict(device="cpu", kv_dtype="fp32", block=256,
                   max_tokens=rc.CAP - 256), **kw)
    n_pages = n_pages or fc.pool_pages(page)
    sess = PagedDecodeSession(rc.B, rc.HKV, rc.D, pool_tokens=n_pages * page,
                              page=page, **kw)
    assert sess.n_pages == n_pages
    return sess


def _slab(**kw):
    kw = dict(dict(device="cpu", kv_dtype="fp32", block=256,
                   max_tokens=rc.CAP - 256), **kw)
    return RaggedDecodeSession(rc.B, rc.HKV, rc.D, **kw)


def _trio(page):
    """(forked paged, independently prefilled paged, forked slab), loaded."""
    sessions = (_paged(page), _paged(page), _slab())
    for sess, forked in zip(sessions, (True, False, True)):
        ks, vs = fc.load(sess, page, "bf16", forked)
    return sessions, ks, vs


def _run(sessions, ks, vs, page, steps, q, first=0):
    """Continuation steps [first, steps) on every session; the first
    session's outputs equal the others' after every step."""
    out = None
    for i in range(first, steps):
        k_new, v_new = fc.step_tokens(ks, vs, page, i)
        outs = []
        for sess in sessions:
            sess.append(k_new, v_new)
            outs.append(sess.attend(q))
        for other in outs[1:]:
            assert torch.equal(outs[0], other), f"step {i}"
        out = outs[0]
    return out


@pytest.mark.parametrize("page", fc.PAGES)
def test_forked_equals_independent_and_slab(page):
    sessions, ks, vs = _trio(page)
    q = fc.at(page, "bf16", fc.STEPS).q.float()
    outs = [s.attend(q) for s in sessions]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    first = fc.at(page, "bf16", 1)
    _run(sessions, ks, vs, page, 1, q)
    rc.compare(first, sessions[0].attend(first.q.float()), None,
               f"forked, page {page}, step 1")
    out = _run(sessions, ks, vs, page, fc.STEPS, q, first=1)
    rc.compare(fc.at(page, "bf16", fc.STEPS), out, None,
               f"forked, page {page}, step {fc.STEPS}")
    forked, indep, _ = sessions
    assert forked.totals == indep.totals == list(fc.lengths_at(page, fc.STEPS))
    assert forked.free_pages > indep.free_pages == fc.SPARE
    fc.table_matches(forked)


@pytest.mark.parametrize("page", fc.PAGES)
def test_page_accounting(page):
    exp = fc.EXPECT[page]
    sess = _paged(page)
    ks, vs = (t for t in fc.fed(page, "bf16"))
    sess.prefill(0, ks[0, :, :fc.PREFIX], vs[0, :, :fc.PREFIX])
    free = sess.free_pages
    assert free == sess.n_pages - pc.pages_of(fc.PREFIX, page)
    assert sess.shared_pages == 0
    pool = sess.k_pool.clone().view(torch.uint8)    # unwritten rows too
    for b in range(1, rc.B):
        sess.fork(0, b, fc.starts(page)[b])
        assert sess.free_pages == free, "fork takes no page"
        fc.table_matches(sess)
    assert torch.equal(sess.k_pool.view(torch.uint8), pool), \
        "fork moves no KV byte"
    assert sess.shared_pages == exp["shared_forked"]
    for b in range(1, rc.B):
        assert sess._pages[b] == sess._pages[0][:len(sess._pages[b])]
    # the rows take their first token one after the other
    k_new, v_new = fc.step_tokens(ks, vs, page, 0)
    copies = dict(exp["copies"])
    for b in range(rc.B):
        held, before = len(sess._pages[b]), list(sess._pages[b])
        at = sess.local_lens[b]
        sess.append(k_new, v_new, [r == b for r in range(rc.B)])
        took = exp["taken"][b]
        assert free - sess.free_pages == took, f"row {b}"
        free = sess.free_pages
        fc.table_matches(sess)
        if b in copies:         # the tail page was replaced by a copy
            assert at % page == copies[b]
            assert len(sess._pages[b]) == held
            assert sess._pages[b][:-1] == before[:-1]
            new, old = sess._pages[b][-1], before[-1]
            assert new != old and sess._refs[new] == 1
            assert torch.equal(sess.k_pool[new, :, :at % page],
                               sess.k_pool[old, :, :at % page])
            assert torch.equal(sess.v_pool[new, :, :at % page],
                               sess.v_pool[old, :, :at % page])
        elif took:              # a fresh page on a page boundary
            assert at % page == 0 and len(sess._pages[b]) == held + 1
        else:                   # the row's own tail page, written in place
            assert sess._pages[b] == before
    assert sess.shared_pages == exp["shared_after"]
    assert sorted(sess._free + [p for p, r in enumerate(sess._refs) if r]) \
        == list(range(sess.n_pages))
    held = [p for row in sess._pages for p in row]
    assert [held.count(p) for p in range(sess.n_pages)] == sess._refs


@pytest.mark.parametrize("page", fc.PAGES)
def test_lifetime(page):
    (forked, indep, _), ks, vs = _trio(page)
    q = fc.at(page, "bf16", fc.STEPS).q.float()
    before = _run((forked, indep), ks, vs, page, fc.STEPS, q)
    free = forked.free_pages
    own = [p for p in forked._pages[0] if forked._refs[p] == 1]
    shared = [p for p in forked._pages[0] if forked._refs[p] > 1]
    assert own and shared
    forked.reset(0)
    assert forked.free_pages == free + len(own)
    assert sorted(forked._free[-len(own):]) == sorted(own)
    assert all(forked._refs[p] >= 1 for p in shared)
    # what row 0 left behind is poisoned and handed to a new tenant
    fc.poison(forked, q, own)
    n_new = len(own) * page - 5
    forked.prefill(0, ks[3, :, 600:600 + n_new], vs[3, :, 600:600 + n_new])
    assert sorted(forked._pages[0]) == sorted(own)
    gone = fc.after_reset(page, "bf16")
    after = forked.attend(q)
    assert torch.equal(after[1:], before[1:]), "the forks lost shared pages"
    forked.reset(0)
    fc.poison(forked, q)
    rc.compare(gone, forked.attend(gone.q.float()), None,
               f"row 0 gone, page {page}")
    # the last holder returns a shared page
    p0 = shared[0]
    holders = [b for b in range(1, rc.B) if p0 in forked._pages[b]]
    assert len(holders) >= 2
    for b in holders[:-1]:
        forked.reset(b)
        assert p0 not in forked._free and forked._refs[p0] >= 1
    forked.reset(holders[-1])
    assert p0 in forked._free and forked._refs[p0] == 0
    for b in range(rc.B):
        forked.reset(b)
    assert forked.free_pages == forked.n_pages and forked.shared_pages == 0
    assert sorted(forked._free) == list(range(forked.n_pages))
    assert not any(forked._refs)


def test_truncate_into_shared_page_copies_again():
    page = 128
    (forked, indep, _), ks, vs = _trio(page)
    q = fc.at(page, "bf16", fc.STEPS).q.float()
    _run((forked, indep), ks, vs, page, fc.STEPS, q)
    p0 = forked._pages[0][0]
    assert forked._refs[p0] == rc.B
    before = forked.attend(q)
    for sess in (forked, indep):
        sess.truncate(1, 100)       # below the fork point 129, inside page 0
    assert forked._pages[1] == [p0] and forked._refs[p0] == rc.B
    free = forked.free_pages
    k_new, v_new = fc.step_tokens(ks, vs, page, 7)
    for sess in (forked, indep):
        sess.append(k_new, v_new, [False, True, False, False])
    assert forked.free_pages == free - 1 and forked._refs[p0] == rc.B - 1
    new = forked._pages[1][0]
    assert new != p0 and forked._refs[new] == 1
    assert torch.equal(forked.k_pool[new, :, :100], forked.k_pool[p0, :, :100])
    fc.table_matches(forked)
    after = forked.attend(q)
    assert torch.equal(after, indep.attend(q))
    keep = [0, 2, 3]
    assert torch.equal(after[keep], before[keep]), "a sibling changed"
    assert not torch.equal(after[1], before[1])


@pytest.mark.parametrize("page", fc.PAGES)
def test_drafts_on_forked_rows(page):
    """append_many + truncate and append_tree + commit right after the fork:
    the copy-on-write happens inside the multi-token appends."""
    (forked, indep, slab), ks, vs = _trio(page)
    sessions = (forked, indep, slab)
    t = 4
    st = torch.tensor(fc.starts(page))
    bi = torch.arange(rc.B)
    idx = st[:, None] + torch.arange(t)[None, :]                 # (B, T)
    kd = ks[bi[:, None], :, idx].permute(0, 2, 1, 3).contiguous()
    vd = vs[bi[:, None], :, idx].permute(0, 2, 1, 3).contiguous()
    g = torch.Generator().manual_seed(11)
    q = torch.randn(rc.B, rc.HQ, t, rc.D, generator=g)
    q1 = fc.at(page, "bf16", 1).q.float()
    counts = [4, 3, 0, 2]
    outs = []
    for sess in sessions:
        sess.append_many(kd, vd, counts)
        outs.append(sess.attend_many(q))
        for b in range(rc.B):
            sess.truncate(b, fc.starts(page)[b] + min(counts[b], 1))
        outs.append(sess.attend(q1))
    for i in (0, 1):
        assert torch.equal(outs[i], outs[i + 2]), ("append_many", i)
        assert torch.equal(outs[i], outs[i + 4]), ("append_many, slab", i)
    fc.table_matches(forked)
    # a tree on top: node 1 and 2 hang off node 0, node 3 off node 1
    parents = [[-1, 0, 0, 1]] * rc.B
    idx = idx + 1
    kd = ks[bi[:, None], :, idx].permute(0, 2, 1, 3).contiguous()
    vd = vs[bi[:, None], :, idx].permute(0, 2, 1, 3).contiguous()
    counts = [4, 4, 3, 0]
    paths, lens = [[0, 1, 3], [0, 2], [0], []], [3, 2, 1, 0]
    outs = []
    for sess in sessions:
        sess.append_tree(kd, vd, parents, counts)
        outs.append(sess.attend_tree(q))
        sess.commit(paths, lens)
        outs.append(sess.attend(q1))
    for i in (0, 1):
        assert torch.equal(outs[i], outs[i + 2]), ("append_tree", i)
        assert torch.equal(outs[i], outs[i + 4]), ("append_tree, slab", i)
    assert forked.totals == indep.totals
    fc.table_matches(forked)
    held = [p for row in forked._pages for p in row]
    assert [held.count(p) for p in range(forked.n_pages)] == forked._refs


def _state(sess):
    return (list(sess.totals), list(sess.local_lens), sess.total_dev.tolist(),
            sess.local_len_dev.tolist(), sess.free_pages,
            [list(p) for p in sess._pages], list(sess._free),
            list(sess._refs), sess.k_pool.clone().view(torch.uint8),
            sess.v_pool.clone().view(torch.uint8),
            sess.page_table.clone())
    # (the pools as bytes: rows nobody wrote may hold NaN bit patterns)


def _unchanged(sess, before):
    after = _state(sess)
    assert after[:8] == before[:8]
    for a, b in zip(after[8:], before[8:]):
        assert torch.equal(a, b)


def test_exhaustion_counts_the_copy():
    torch.manual_seed(4)
    sess = PagedDecodeSession(3, 2, 16, max_tokens=1024, pool_tokens=256,
                              page=128, device="cpu", kv_dtype="fp32",
                              block=64)
    assert sess.n_pages == 2
    seq = torch.randn(2, 130, 16)
    k1 = torch.randn(3, 2, 1, 16)
    sess.prefill(0, seq, seq)
    sess.fork(0, 1, 129)
    sess.fork(0, 2, 128)
    assert sess.free_pages == 0 and sess.shared_pages == 2
    before = _state(sess)
    # row 1 would write row 1 of a page row 0 holds: it needs a copy
    with pytest.raises(RuntimeError, match=r"pool exhausted: row 1 "):
        sess.append(k1, k1, [False, True, False])
    _unchanged(sess, before)
    # row 0's tail is that same page: whoever writes first needs the copy
    with pytest.raises(RuntimeError, match=r"pool exhausted: row 0 "):
        sess.append(k1, k1, [True, True, False])
    _unchanged(sess, before)
    # row 2 sits on a page boundary: a fresh page, not a copy
    with pytest.raises(RuntimeError, match=r"pool exhausted: row 2 "):
        sess.append(k1, k1, [False, False, True])
    _unchanged(sess, before)
    with pytest.raises(RuntimeError, match=r"pool exhausted: row 1 "):
        sess.append_many(k1.expand(-1, -1, 2, -1), k1.expand(-1, -1, 2, -1),
                         [0, 2, 0])
    _unchanged(sess, before)
    sess.reset(0)                   # row 1 is now the tail page's one holder
    assert sess.free_pages == 0 and sess.shared_pages == 1
    sess.append(k1, k1, [False, True, False])
    assert sess.totals == [0, 130, 128] and sess.free_pages == 0
    assert torch.equal(sess.k_pool[sess._pages[1][1], :, 1], k1[1, :, 0])


def test_fork_rejects_bad_arguments():
    for sess in (_paged(128), _slab()):
        ks, vs = fc.fed(128, "bf16")
        sess.prefill(0, ks[0, :, :10], vs[0, :, :10])
        for src, dst, tokens in ((0, 0, None), (1, 1, 0), (0, 1, 11),
                                 (0, 1, -1), (1, 0, 1), (0, rc.B, None),
                                 (-1, 1, None), (rc.B, 0, None), (0, -1, 3)):
            with pytest.raises(ValueError, match="fork"):
                sess.fork(src, dst, tokens)
        assert sess.totals == [10, 0, 0, 0]
        sess.fork(0, 1)             # None: all of them
        sess.fork(0, 2, 0)
        assert sess.totals == [10, 10, 0, 0]
        assert sess.total_dev.tolist() == sess.totals
    assert not hasattr(_slab(), "shared_pages")
    sess = _paged(128)
    with pytest.raises(AttributeError):
        sess.shared_pages = 1


def test_fork_drops_what_dst_held_and_the_pending_tree():
    page = 128
    sess = _paged(page)
    ks, vs = fc.fed(page, "bf16")
    sess.prefill(0, ks[0, :, :200], vs[0, :, :200])
    sess.prefill(1, ks[1, :, :300], vs[1, :, :300])
    assert sess.free_pages == sess.n_pages - 5
    kd = ks[:, :, 300:302].contiguous()
    sess.append_tree(kd, kd, [[-1, 0]] * rc.B, [2, 0, 0, 0])
    sess.fork(0, 1, 150)
    assert sess.free_pages == sess.n_pages - 2 and sess.shared_pages == 2
    with pytest.raises(RuntimeError, match="no append_tree"):
        sess.commit([[0], [], [], []], [1, 0, 0, 0])
    with pytest.raises(RuntimeError, match="no append_tree"):
        sess.attend_tree(torch.zeros(rc.B, rc.HQ, 2, rc.D))
    assert sess.totals == [202, 150, 0, 0]


def _worker(rank, world, port):
    import sys

    import torch.distributed as dist

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        page, block = 128, 64
        kw = dict(block=block, max_tokens=rc.CAP)
        forked, slab = _paged(page, n_pages=16, **kw), _slab(**kw)
        for sess in (forked, slab):
            ks, vs = fc.load(sess, page, "bf16", True)

        def counts_ok():
            want = [_n_local(t, block, rank, world) for t in forked.totals]
            assert forked.local_lens == slab.local_lens == want
            fc.table_matches(forked)     # ceil(_n_local / page) pages a row

        counts_ok()
        used = pc.pages_of(_n_local(fc.PREFIX, block, rank, world), page)
        assert forked.free_pages == 16 - used, "the forks took no page"
        q = fc.at(page, "bf16", fc.STEPS).q.float()
        # collectives are slow on gloo: attend across the first (copying)
        # step only, then at the end
        _run((forked, slab), ks, vs, page, 1, q)
        for i in range(1, fc.STEPS):
            k_new, v_new = fc.step_tokens(ks, vs, page, i)
            for sess in (forked, slab):
                sess.append(k_new, v_new)
        counts_ok()
        held = [p for row in forked._pages for p in row]
        assert [held.count(p) for p in range(16)] == forked._refs
        assert forked.free_pages == 16 - len(set(held))
        rg = fc.at(page, "bf16", fc.STEPS)
        for combine in ("allgather", "allreduce"):
            out = forked.attend(q, combine=combine)
            assert torch.equal(out, slab.attend(q, combine=combine))
            rc.compare(rg, out, None, f"rank {rank} {combine}")
    finally:
        dist.destroy_process_group()


def test_forked_ws2():
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 2, 29781))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
