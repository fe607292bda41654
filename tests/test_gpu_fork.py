"""Prefix sharing on the GPU: kv_pool_copy_rows against the byte model of
tests/fork_cases.py, its binding's refusals, and the fork scenario on a
PagedDecodeSession, eager and through the three captured steps (what the
scenario can see is proven on the CPU in tests/test_fork_sensitivity.py)."""

import pytest
import torch

import fork_cases as fc
import paged_cases as pc
import ragged_cases as rc

pytestmark = pytest.mark.gpu

NGPU = torch.cuda.device_count() if torch.cuda.is_available() else 0
_PORT = 29690
U8 = torch.uint8
_TD = {"bf16": torch.bfloat16, "fp16": torch.float16,
       "fp8": torch.float8_e4m3fn}


@pytest.fixture(scope="module")
def ext():
    from tree_attention_torch_amd.ops import flash

    assert flash.hip_available(), "HIP extension must be built in-tree"
    return flash._load_extension()


# --------------------------------------------------------------------------
# kv_pool_copy_rows
# --------------------------------------------------------------------------
N_PAGES = 24       # 4 sources, up to 17 destinations, 3 pages nobody names


def _pools(dtype, page, hkv, d=rc.D, n_pages=N_PAGES):
    """Random BYTES, so every bit pattern of the dtype travels."""
    td = _TD[dtype]
    g = torch.Generator().manual_seed(page + hkv)
    raw = torch.randint(0, 256, (2, n_pages, hkv, page, d * td.itemsize),
                        dtype=U8, generator=g)
    return raw[0].view(td), raw[1].view(td)


def _rows_of(page):
    return (0, 1, 63, 127, 128, page - 1, page)


def _triples(n, page, shift=0):
    rows = _rows_of(page)
    return [(i % 4, 4 + i, rows[(i + shift) % len(rows)]) for i in range(n)]


def _check_copy(ext, k, v, triples, what):
    """The device copy of `triples` over pools k / v (CPU) against
    fork_cases.copy_rows: the whole pool, as bytes."""
    kd, vd = k.cuda(), v.cuda()
    ext.kv_pool_copy_rows(kd, vd, [t[0] for t in triples],
                          [t[1] for t in triples], [t[2] for t in triples])
    want_k, want_v = k.clone(), v.clone()
    fc.copy_rows(want_k, want_v, triples)
    assert torch.equal(kd.cpu().view(U8), want_k.view(U8)), f"K, {what}"
    assert torch.equal(vd.cpu().view(U8), want_v.view(U8)), f"V, {what}"


@pytest.mark.parametrize("hkv", [1, 2])
@pytest.mark.parametrize("page", [128, 1024])
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp8"])
def test_kv_pool_copy_rows(ext, dtype, page, hkv):
    k, v = _pools(dtype, page, hkv)
    for rows in _rows_of(page):                          # n = 1
        _check_copy(ext, k, v, [(2, 9, rows)], f"n = 1, rows = {rows}")
    for shift in (0, 3):                                 # n = 16
        _check_copy(ext, k, v, _triples(16, page, shift),
                    f"n = 16, shift {shift}")
    _check_copy(ext, k, v, _triples(17, page, 5), "n = 17: two launches")
    # a later launch may read what an earlier one wrote
    chain = _triples(16, page, 2) + [(4, 21, page), (19, 22, 127)]
    _check_copy(ext, k, v, chain, "n = 18, chained")


@pytest.mark.parametrize("dtype,d", [("bf16", 6), ("fp8", 12), ("fp16", 2)])
def test_kv_pool_copy_rows_4_byte_units(ext, dtype, d):
    """Rows of 12 or 4 bytes: no 16-byte unit fits."""
    k, v = _pools(dtype, 128, 2, d=d)
    _check_copy(ext, k, v, _triples(16, 128, 1), f"D = {d}")
    _check_copy(ext, k, v, [(0, 5, 128)], f"D = {d}, whole page")


def test_kv_pool_copy_rows_checks(ext):
    """Every refusal raises before anything is launched: the pools keep
    their bytes."""
    k0, v0 = _pools("bf16", 128, 2, n_pages=20)
    k, v = k0.cuda(), v0.cuda()

    def copy(src, dst, rows, k=k, v=v):
        ext.kv_pool_copy_rows(k, v, src, dst, rows)

    copy([], [], [])                        # nothing to do, nothing launched
    bad = [
        ([0], [1, 2], [1, 1]), ([0, 0], [1, 2], [1]),   # unequal lengths
        ([-1], [1], [1]), ([20], [1], [1]),             # src out of range
        ([0], [-1], [1]), ([0], [20], [1]),             # dst out of range
        ([3], [3], [1]),                                # src == dst
        ([0, 1], [2, 2], [1, 1]),                       # a dst twice
        ([0, 2], [2, 3], [1, 1]),                       # a dst that is a src
        ([0], [1], [-1]), ([0], [1], [129]),            # rows out of range
        # the 17th triple is bad: the first 16 must not go out either
        ([0] * 17, list(range(1, 17)) + [20], [1] * 17),
        ([0] * 17, list(range(1, 17)) + [0], [1] * 17),
    ]
    for src, dst, rows in bad:
        with pytest.raises(RuntimeError, match="kv_pool_copy_rows"):
            copy(src, dst, rows)
    kw = dict(dtype=torch.bfloat16, device="cuda")
    pools = [
        (k, v[:19]),                                    # shapes differ
        (k, v.half()),                                  # dtypes differ
        (k, v0),                                        # a CPU pool
        (k[:, :, :, ::2], v[:, :, :, ::2]),             # not contiguous
        (k[0], v[0]),                                   # not 4-d
        (torch.zeros(4, 2, 64, 128, **kw),) * 2,        # page 64
        (torch.zeros(4, 2, 128, 1, **kw),) * 2,         # 2-byte rows
    ]
    for kp, vp in pools:
        with pytest.raises(RuntimeError, match="kv_pool_copy_rows"):
            copy([0], [1], [1], k=kp, v=vp)
    torch.cuda.synchronize()
    assert torch.equal(k.cpu().view(U8), k0.view(U8))
    assert torch.equal(v.cpu().view(U8), v0.view(U8))
    copy([0], [1], [128])
    assert _bytes_equal(k[1], k[0]) and _bytes_equal(v[1], v[0])


# --------------------------------------------------------------------------
# the scenario on a PagedDecodeSession
# --------------------------------------------------------------------------
def _session(dtype, page, device="cuda", **kw):
    from tree_attention_torch_amd.session import PagedDecodeSession

    kw = dict(dict(max_tokens=rc.CAP - 256, block=256), **kw)
    sess = PagedDecodeSession(rc.B, rc.HKV, rc.D,
                              pool_tokens=fc.pool_pages(page) * page,
                              page=page, device=device, kv_dtype=dtype, **kw)
    assert sess.n_pages == fc.pool_pages(page)
    return sess


def _bytes_equal(a, b):
    return torch.equal(a.view(U8), b.view(U8))


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("page", fc.PAGES)
def test_forked_session_gpu(ext, page, dtype):
    """Forked against independently prefilled: the same kernel over the
    same bytes on other physical pages, so the outputs are bit-equal after
    every step; and against the fp32 oracle after the copying step, at the
    end, and once row 0 has left."""
    exp = fc.EXPECT[page]
    forked, indep = _session(dtype, page), _session(dtype, page)
    ks, vs = fc.load(forked, page, dtype, True, "cuda")
    fc.load(indep, page, dtype, False, "cuda")
    last = fc.at(page, dtype, fc.STEPS)
    q = last.q.cuda()
    assert forked.shared_pages == exp["shared_forked"]
    assert forked.free_pages == forked.n_pages - pc.pages_of(fc.PREFIX, page)
    for sess in (forked, indep):    # a page handed out from here on is poison
        fc.poison(sess, q)
    assert torch.equal(forked.attend(q), indep.attend(q))
    for i in range(fc.STEPS):
        k_new, v_new = fc.step_tokens(ks, vs, page, i)
        free = forked.free_pages
        for sess in (forked, indep):
            sess.append(k_new, v_new)
        out = forked.attend(q)
        assert torch.equal(out, indep.attend(q)), f"step {i}"
        if i == 0:
            assert free - forked.free_pages == sum(exp["taken"])
            assert forked.shared_pages == exp["shared_after"]
            first = fc.at(page, dtype, 1)
            rc.compare(first, forked.attend(first.q.cuda()), None,
                       f"forked, page {page}, step 1")
    rc.compare(last, out, None, f"forked, page {page}, step {fc.STEPS}")
    fc.table_matches(forked)
    assert forked.local_len_dev.tolist() == list(fc.lengths_at(page, fc.STEPS))
    for b in range(rc.B):       # the stored bytes are the stream's
        n = forked.local_lens[b]
        stored = forked._rows(b, n)[0][0].cpu()
        assert _bytes_equal(stored, last.k[b, :, :n]), f"row {b}"
    assert forked.free_pages > indep.free_pages == fc.SPARE
    forked.reset(0)
    fc.poison(forked, q)
    gone = fc.after_reset(page, dtype)
    rc.compare(gone, forked.attend(gone.q.cuda()), None,
               f"row 0 gone, page {page}")
    for b in range(rc.B):
        forked.reset(b)
    assert forked.free_pages == forked.n_pages and forked.shared_pages == 0


def _statics(t, dtype=torch.bfloat16):
    q = torch.zeros(rc.B, rc.HQ, t, rc.D, dtype=dtype, device="cuda")
    k = torch.zeros(rc.B, rc.HKV, t, rc.D, dtype=dtype, device="cuda")
    return q, k, torch.zeros_like(k)


@pytest.mark.parametrize("dtype,page", [("bf16", 128), ("fp8", 256)])
def test_graphed_step_survives_fork(ext, dtype, page):
    """graphed_step captured while rows 1..3 are empty; then the forks; then
    replays across the copying step and, at page 128, a page boundary: the
    copies go out eagerly ahead of each replay and the static table carries
    the new pages in. Bit-equal to an eager forked twin, pools included."""
    sess, twin = _session(dtype, page), _session(dtype, page)
    ks, vs = (t.cuda() for t in fc.fed(page, dtype))
    for s in (sess, twin):
        s.k_pool.zero_()    # the pools are compared whole at the end, the
        s.v_pool.zero_()    # rows nobody ever wrote included
        s.prefill(0, ks[0, :, :fc.PREFIX], vs[0, :, :fc.PREFIX])
    q_static, k_static, v_static = _statics(1)
    replay = sess.graphed_step(q_static, k_static, v_static)
    assert sess.totals == [fc.PREFIX, 0, 0, 0]
    last = fc.at(page, dtype, fc.STEPS)
    for s in (sess, twin):
        for b in range(1, rc.B):
            s.fork(0, b, fc.starts(page)[b])
        fc.poison(s, last.q)
    assert sess.local_len_dev.tolist() == list(fc.starts(page))
    q_static.copy_(last.q)
    for i in range(fc.STEPS):
        k_new, v_new = fc.step_tokens(ks, vs, page, i)
        k_static.copy_(k_new)
        v_static.copy_(v_new)
        free = sess.free_pages
        out = replay()
        twin.append(k_new, v_new)
        assert torch.equal(out, twin.attend(q_static)), f"step {i}"
        if i == 0:
            assert free - sess.free_pages == sum(fc.EXPECT[page]["taken"])
            assert sess._pages == twin._pages
    rc.compare(last, out, None, f"graphed forked, page {page}")
    assert sess.totals == list(fc.lengths_at(page, fc.STEPS))
    assert sess.local_len_dev.tolist() == sess.local_lens
    assert sess._pages == twin._pages
    held = {p for row in sess._pages for p in row}
    assert sess.free_pages == twin.free_pages == sess.n_pages - len(held)
    for a, b in ((sess.k_pool, twin.k_pool), (sess.v_pool, twin.v_pool)):
        differ = (a.view(U8) != b.view(U8)).flatten(1).any(1)
        assert not differ.any(), f"pages {differ.nonzero().flatten().tolist()}"
    assert torch.equal(sess.page_table, twin.page_table)


def _drafts(ks, vs, page, t, shift=0):
    idx = torch.tensor(fc.starts(page))[:, None] + shift + \
        torch.arange(t)[None, :]
    bi = torch.arange(rc.B)[:, None]
    return (ks[bi, :, idx].permute(0, 2, 1, 3).contiguous(),
            vs[bi, :, idx].permute(0, 2, 1, 3).contiguous())


def _draft_sessions(dtype, page):
    """(to capture on: row 0 only; eager forked twin; eager, independently
    prefilled) and the fed streams."""
    sess, twin, indep = (_session(dtype, page) for _ in range(3))
    ks, vs = (t.cuda() for t in fc.fed(page, dtype))
    for s in (sess, twin):
        s.prefill(0, ks[0, :, :fc.PREFIX], vs[0, :, :fc.PREFIX])
    fc.load(indep, page, dtype, False, "cuda")
    return sess, twin, indep, ks, vs


def _fork_all(sessions, page, q):
    for s in sessions:
        if s.totals[1] == 0:
            for b in range(1, rc.B):
                s.fork(0, b, fc.starts(page)[b])
        fc.poison(s, q)


def test_graphed_step_many_on_forked_rows(ext):
    dtype, page, t = "bf16", 128, 4
    sess, twin, indep, ks, vs = _draft_sessions(dtype, page)
    q_static, k_static, v_static = _statics(t)
    replay = sess.graphed_step_many(q_static, k_static, v_static)
    g = torch.Generator().manual_seed(13)
    q = torch.randn(rc.B, rc.HQ, t, rc.D, generator=g).bfloat16().cuda()
    q1 = fc.at(page, dtype, 1).q.cuda()
    _fork_all((sess, twin, indep), page, q1)
    kd, vd = _drafts(ks, vs, page, t)
    counts = [4, 3, 1, 2]
    q_static.copy_(q)
    k_static.copy_(kd)
    v_static.copy_(vd)
    free = sess.free_pages
    out = replay(counts)
    # row 0 writes in place; rows 1 and 2 copy, row 3 opens a page
    assert free - sess.free_pages == 3
    outs = []
    for s in (twin, indep):
        s.append_many(kd, vd, counts)
        outs.append(s.attend_many(q))
    assert torch.equal(out, outs[0]) and torch.equal(out, outs[1])
    for s in (sess, twin, indep):
        for b in range(rc.B):
            s.truncate(b, fc.starts(page)[b] + 1)
    ref = indep.attend(q1)
    assert torch.equal(sess.attend(q1), ref)
    assert torch.equal(twin.attend(q1), ref)
    rc.compare(fc.at(page, dtype, 1), ref, None, "one draft kept per row")
    fc.table_matches(sess)


def test_graphed_step_tree_on_forked_rows(ext):
    dtype, page, t = "fp8", 256, 4
    sess, twin, indep, ks, vs = _draft_sessions(dtype, page)
    q_static, k_static, v_static = _statics(t)
    p_static = torch.full((rc.B, t), -1, dtype=torch.int32, device="cuda")
    replay = sess.graphed_step_tree(q_static, k_static, v_static, p_static)
    g = torch.Generator().manual_seed(17)
    q = torch.randn(rc.B, rc.HQ, t, rc.D, generator=g).bfloat16().cuda()
    q1 = fc.at(page, dtype, 1).q.cuda()
    _fork_all((sess, twin, indep), page, q1)
    kd, vd = _drafts(ks, vs, page, t)
    parents = [[-1, 0, 0, 1]] * rc.B
    counts = [4, 4, 3, 0]
    q_static.copy_(q)
    k_static.copy_(kd)
    v_static.copy_(vd)
    p_static.copy_(torch.tensor(parents, dtype=torch.int32))
    free = sess.free_pages
    out = replay(counts)
    # page 256: rows 0 and 2 copy (44 and 129 rows), row 1 then writes in place
    assert free - sess.free_pages == 2
    outs = []
    for s in (twin, indep):
        s.append_tree(kd, vd, parents, counts)
        outs.append(s.attend_tree(q))
    assert torch.equal(out, outs[0]) and torch.equal(out, outs[1])
    paths, lens = [[0, 1, 3], [0, 2], [0], []], [3, 2, 1, 0]
    for s in (sess, twin, indep):
        s.commit(paths, lens)
    ref = indep.attend(q1)
    assert torch.equal(sess.attend(q1), ref)
    assert torch.equal(twin.attend(q1), ref)
    assert sess.totals == indep.totals
    fc.table_matches(sess)
    held = [p for row in sess._pages for p in row]
    assert [held.count(p) for p in range(sess.n_pages)] == sess._refs


# --------------------------------------------------------------------------
# multi-rank (RCCL): auto-skips below 2 GPUs
# --------------------------------------------------------------------------
def _fork_rccl_worker(rank, world, port):
    import os

    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import fork_cases as fcw
    import ragged_cases as rcw
    from tree_attention_torch_amd.parallel.pg import cleanup, setup
    from tree_attention_torch_amd.session import _n_local

    device = torch.device(f"cuda:{rank}")
    setup(rank, world)
    try:
        page, dtype, block = 128, "bf16", 64
        sess = _session(dtype, page, device=device, max_tokens=rcw.CAP,
                        block=block)
        ks, vs = fcw.load(sess, page, dtype, True, device)
        last = fcw.at(page, dtype, fcw.STEPS)
        fcw.poison(sess, last.q)
        for i in range(fcw.STEPS):
            sess.append(*fcw.step_tokens(ks, vs, page, i))
        assert sess.local_lens == [_n_local(n, block, rank, world)
                                   for n in last.lengths]
        assert sess.local_len_dev.tolist() == sess.local_lens
        fcw.table_matches(sess)
        for combine in ("allgather", "allreduce"):
            out = sess.attend(last.q.to(device), combine=combine)
            torch.cuda.synchronize()
            rcw.compare(last, out, None, f"rank {rank} {combine}")
    finally:
        cleanup()


@pytest.mark.skipif(NGPU < 2, reason=f"needs >=2 GPUs, have {NGPU}")
def test_rccl_forked_session():
    import torch.multiprocessing as mp

    mp.spawn(_fork_rccl_worker, args=(NGPU, _PORT), nprocs=NGPU, join=True)
