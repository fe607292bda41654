"""Paged KV cache on the GPU: the paged instantiations of the two decode
kernels, the paged append kernel, PagedDecodeSession and its captured step,
on the needle inputs of tests/paged_cases.py (what they can see is proven on
the CPU in tests/test_paged_sensitivity.py)."""

import pytest
import torch

import paged_cases as pc
import ragged_cases as rc

pytestmark = pytest.mark.gpu

NGPU = torch.cuda.device_count() if torch.cuda.is_available() else 0
_PORT = 29660
SCALE = 1.0 / rc.D ** 0.5


@pytest.fixture(scope="module")
def ext():
    from tree_attention_torch_amd.ops import flash

    assert flash.hip_available(), "HIP extension must be built in-tree"
    return flash._load_extension()


# capacity 1024, then 4608 with its seam and its pair family
SETS = [pytest.param(n, "seam", id=str(n)) for n in pc.SETS] + \
    [pytest.param(n, "pair", id=f"{n}-pair") for n in rc.LENGTH_SETS_BIG]


def _len_dev(lengths):
    return torch.tensor(list(lengths), dtype=torch.long, device="cuda")


# --------------------------------------------------------------------------
# flash_attention_paged
# --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("page", pc.PAGES)
@pytest.mark.parametrize("lengths,family", SETS)
def test_paged_kernel(ext, lengths, family, page, dtype):
    """Meets the oracle at the suite's bars (an empty row: out = 0 and
    lse = -inf exactly), and is bit-equal to flash_attention_cache over the
    same rows laid out contiguously: the arithmetic is the same, only the
    addresses differ."""
    import needle_cases as nc

    nc.assert_default_split_plan()
    pl = pc.pool(lengths, dtype, page, family)
    rg = pl.rg
    q, lens = rg.q.cuda(), _len_dev(lengths)
    out, lse = ext.flash_attention_paged(q, pl.k_pool.cuda(), pl.v_pool.cuda(),
                                         pl.table.cuda(), lens, SCALE)
    assert out.shape == (rc.B, rc.HQ, 1, rc.D)
    assert lse.shape == (rc.B, rc.HQ, 1)
    rc.compare(rg, out, lse, f"flash_attention_paged, page {page}")
    flat = ext.flash_attention_cache(q, rg.k_cache.cuda(), rg.v_cache.cuda(),
                                     lens, SCALE)
    assert torch.equal(out, flat[0]) and torch.equal(lse, flat[1]), \
        f"paged != contiguous, {dtype} {lengths} page {page}"


@pytest.mark.parametrize("dtype", rc.DTYPES)
def test_paged_kernel_clamps_page_ids(ext, dtype):
    """Entries past a row's live pages are never read, whatever they hold;
    a live entry outside the pool reads the nearest page of the pool: wrong
    numbers at worst, never an address outside it."""
    pl = pc.pool(rc.LENGTH_SETS[0], dtype, 256)
    rg = pl.rg
    q, lens = rg.q.cuda(), _len_dev(rg.lengths)
    kp, vp = pl.k_pool.cuda(), pl.v_pool.cuda()
    want = ext.flash_attention_paged(q, kp, vp, pl.table.cuda(), lens, SCALE)

    dead = pl.table.clone()
    for b, n in enumerate(rg.lengths):
        dead[b, pc.pages_of(n, 256):] = 2 ** 31 - 1 if b % 2 else -2 ** 31
    got = ext.flash_attention_paged(q, kp, vp, dead.cuda(), lens, SCALE)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])

    # row 3 (1023 keys): logical page 1 far above the pool, page 2 below it
    high, low, edge = pl.table.clone(), pl.table.clone(), pl.table.clone()
    high[3, 1], low[3, 2] = pl.n_pages + 1000, -7
    edge[3, 1], edge[3, 2] = pl.n_pages - 1, 0
    both = high.clone()
    both[3, 2] = -7
    got = ext.flash_attention_paged(q, kp, vp, both.cuda(), lens, SCALE)
    ref = ext.flash_attention_paged(q, kp, vp, edge.cuda(), lens, SCALE)
    assert torch.equal(got[0][:3], want[0][:3])
    # NaN poison may sit in the pages read instead: compare bits
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32))
    assert torch.equal(got[1].view(torch.int32), ref[1].view(torch.int32))


def test_paged_binding_checks(ext):
    pl = pc.pool(rc.LENGTH_SETS[0], "bf16", 128)
    rg = pl.rg
    q, lens = rg.q.cuda(), _len_dev(rg.lengths)
    kp, vp, tb = pl.k_pool.cuda(), pl.v_pool.cuda(), pl.table.cuda()

    def call(q=q, kp=kp, vp=vp, tb=tb, lens=lens):
        return ext.flash_attention_paged(q, kp, vp, tb, lens, SCALE)

    with pytest.raises(RuntimeError, match="page size"):
        call(kp=kp[:, :, :64].contiguous(), vp=vp[:, :, :64].contiguous())
    with pytest.raises(RuntimeError, match="page size"):
        call(kp=kp[:, :, :96].contiguous(), vp=vp[:, :, :96].contiguous())
    with pytest.raises(RuntimeError, match="rows packed"):
        call(kp=kp[:, :, :, :64], vp=vp[:, :, :, :64])
    with pytest.raises(RuntimeError, match="pools must match"):
        call(vp=vp[:-1].contiguous())
    with pytest.raises(RuntimeError, match="int32"):
        call(tb=tb.long())
    with pytest.raises(RuntimeError, match="int32"):
        call(tb=tb[:3].contiguous())
    with pytest.raises(RuntimeError, match="int32"):
        call(tb=tb.t().contiguous().t())
    for n in (1, 2, rc.B + 1):
        with pytest.raises(RuntimeError, match="len_dev"):
            call(lens=_len_dev([5] * n))
    with pytest.raises(RuntimeError, match="len_dev"):
        call(lens=lens.int())
    with pytest.raises(RuntimeError, match="dtype"):
        call(q=q.half())
    with pytest.raises(RuntimeError, match="fp8 pool requires bf16"):
        call(q=q.half(), kp=kp.to(torch.float8_e4m3fn),
             vp=vp.to(torch.float8_e4m3fn))
    with pytest.raises(RuntimeError, match=r"G\*Tq <= 16"):
        call(q=q.expand(-1, -1, 5, -1).contiguous())
    with pytest.raises(RuntimeError, match="head_dim"):
        call(q=q[..., :64].contiguous(), kp=kp[..., :64].contiguous(),
             vp=vp[..., :64].contiguous())


# --------------------------------------------------------------------------
# kv_pool_append
# --------------------------------------------------------------------------
def _place(t, block, world):
    return (t // block) % world, block * ((t // block) // world) + t % block


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("rank,world,block", [(1, 3, 4), (0, 1, 64)])
def test_kv_pool_append(ext, dtype, rank, world, block):
    """40 masked steps into sentinel-filled pools (test_kv_cache_append's
    pattern): the stored rows are bit equal to what the host formula places
    through the table, the lengths equal the host mirror, and every other
    byte still holds the sentinel. Row 2 crosses from its first page to its
    second; row 3 runs past the table's two pages: `total` advances and
    nothing is stored."""
    bsz, hkv, d, page, max_pages, n_pages, steps = 4, 2, 128, 128, 2, 10, 40
    cap = page * max_pages
    td = rc._TD[dtype]
    g = torch.Generator().manual_seed(rc.SEED + block)
    esz = torch.empty(0, dtype=td).element_size()
    kp = torch.full((n_pages, hkv, page, d * esz), 0xA5, dtype=torch.uint8,
                    device="cuda").view(td)
    vp = torch.full((n_pages, hkv, page, d * esz), 0x5A, dtype=torch.uint8,
                    device="cuda").view(td)
    assert kp.shape == (n_pages, hkv, page, d)
    pages = [[7, 2], [0, 9], [4, 1], [8, 3]]       # 5 and 6: nobody's
    table = torch.tensor(pages, dtype=torch.int32, device="cuda")
    want_k, want_v = kp.cpu().clone(), vp.cpu().clone()
    # rows 2 and 3 start 2 and 6 keys below local positions 128 and 256
    start = [0, 3, 126 * world, 250 * world]
    total = torch.tensor(start, dtype=torch.long, device="cuda")
    # local_len starts at a value the kernel must leave alone until this
    # rank stores a token of that row
    llen = torch.tensor([0, 1, 2, 3], dtype=torch.long, device="cuda")
    h_total, h_llen = list(start), [0, 1, 2, 3]
    dropped = crossed = 0
    for i in range(steps):
        mask = [(i + b) % 3 != 0 and (b != 1 or i < 25) for b in range(bsz)]
        k_new = torch.randn(bsz, hkv, 1, d, generator=g).to(td)
        v_new = torch.randn(bsz, hkv, 1, d, generator=g).to(td)
        ext.kv_pool_append(kp, vp, table, k_new.cuda(), v_new.cuda(), total,
                           llen, torch.tensor(mask, dtype=torch.uint8).cuda(),
                           block, rank, world)
        for b in range(bsz):
            if not mask[b]:
                continue
            owner, pos = _place(h_total[b], block, world)
            if owner == rank and pos < cap:
                pid = pages[b][pos // page]
                want_k[pid, :, pos % page] = k_new[b, :, 0]
                want_v[pid, :, pos % page] = v_new[b, :, 0]
                h_llen[b] = pos + 1
                crossed += b == 2 and pos >= page
            dropped += owner == rank and pos >= cap
            h_total[b] += 1
    assert total.tolist() == h_total and llen.tolist() == h_llen
    assert dropped > 0 and crossed > 0 and h_llen[3] == cap
    assert torch.equal(kp.cpu().view(torch.uint8), want_k.view(torch.uint8))
    assert torch.equal(vp.cpu().view(torch.uint8), want_v.view(torch.uint8))


def test_kv_pool_append_checks(ext):
    kp = torch.zeros(4, 2, 128, 128, dtype=torch.bfloat16, device="cuda")
    new = torch.zeros(2, 2, 1, 128, dtype=torch.bfloat16, device="cuda")
    tb = torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    lens = torch.zeros(2, dtype=torch.long, device="cuda")
    act = torch.ones(2, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="rank"):
        ext.kv_pool_append(kp, kp.clone(), tb, new, new, lens, lens.clone(),
                           act, 4, 2, 2)
    with pytest.raises(RuntimeError, match="dtype"):
        ext.kv_pool_append(kp, kp.clone(), tb, new.half(), new.half(), lens,
                           lens.clone(), act, 4, 0, 1)
    with pytest.raises(RuntimeError, match="int64"):
        ext.kv_pool_append(kp, kp.clone(), tb, new, new, lens.int(),
                           lens.clone(), act, 4, 0, 1)
    with pytest.raises(RuntimeError, match=r"\(B,\)"):
        ext.kv_pool_append(kp, kp.clone(), tb, new, new, lens, lens.clone(),
                           act[:1], 4, 0, 1)
    with pytest.raises(RuntimeError, match="int32"):
        ext.kv_pool_append(kp, kp.clone(), tb.long(), new, new, lens,
                           lens.clone(), act, 4, 0, 1)
    with pytest.raises(RuntimeError, match="page size"):
        ext.kv_pool_append(kp[:, :, :100].contiguous(),
                           kp[:, :, :100].contiguous(), tb, new, new, lens,
                           lens.clone(), act, 4, 0, 1)
    assert not kp.any() and not lens.any()


# --------------------------------------------------------------------------
# PagedDecodeSession
# --------------------------------------------------------------------------
def _session(dtype, page, cap=rc.CAP, spare=pc.SPARE, lengths=None, **kw):
    from tree_attention_torch_amd.session import PagedDecodeSession

    # capacity = (ceil(max_tokens / block) + 1) blocks: 1024 or 4608; the
    # pool holds the pages `lengths` needs (default: every row full) + spare
    need = sum(pc.pages_of(n, page) for n in (lengths or [cap] * rc.B))
    sess = PagedDecodeSession(rc.B, rc.HKV, rc.D, max_tokens=cap - 256,
                              pool_tokens=(need + spare) * page, page=page,
                              device="cuda", kv_dtype=dtype, block=256, **kw)
    assert sess.capacity == cap and sess.n_pages == need + spare
    return sess


def _feed(sess, rg, lengths, tail=3):
    """Sequence b's first lengths[b] tokens: all but the last `tail` through
    prefill, the rest through masked appends."""
    ks, vs = (t.cuda() for t in rc.stream(rg))
    for b, n in enumerate(lengths):
        if n > tail:
            sess.prefill(b, ks[b, :, :n - tail], vs[b, :, :n - tail])
    while sess.totals != list(lengths):
        mask = [sess.totals[b] < lengths[b] for b in range(rc.B)]
        at = torch.tensor(sess.totals).clamp(max=rg.cap - 1)
        bi = torch.arange(rc.B)
        sess.append(ks[bi, :, at][:, :, None], vs[bi, :, at][:, :, None],
                    mask)
    assert sess.local_lens == list(lengths)
    assert sess.total_dev.tolist() == list(lengths)
    assert sess.local_len_dev.tolist() == list(lengths)
    assert [len(p) for p in sess._pages] == \
        [pc.pages_of(n, sess.page) for n in lengths]


def _guard(sess, rg, lengths):
    """paged_cases' poison over the session's pool, in place (a captured
    step holds its address): the guard rows at and past each row's length
    on its last live page, decoy K / NaN V on every free page, and every
    table entry past a row's live pages names a free page."""
    page, td = sess.page, sess.k_pool.dtype
    gk, gv = rc.guard_fill(rg.q.cpu(), rg.cap)
    assert sess.free_pages >= 1
    for b, n in enumerate(lengths):
        live = len(sess._pages[b])
        assert live == pc.pages_of(n, page)
        if n % page:
            pid, lo = sess._pages[b][-1], n % page
            at = (live - 1) * page
            sess.k_pool[pid, :, lo:] = gk[b, :, at + lo:at + page].to(
                device="cuda", dtype=td)
            sess.v_pool[pid, :, lo:] = gv[b, :, at + lo:at + page].to(
                device="cuda", dtype=td)
        sess.page_table[b, live:] = sess._free[0]
    for pid in sess._free:
        sess.k_pool[pid] = gk[pid % rc.B, :, :page].to(device="cuda",
                                                       dtype=td)
        sess.v_pool[pid] = float("nan")


def _stored(sess, b, n):
    """Row b's first n stored rows, through the session's own table."""
    k, _ = sess._rows(b, n)
    return k[0].cpu().view(torch.uint8)


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("page", pc.PAGES)
@pytest.mark.parametrize("lengths,family", SETS)
def test_paged_session_gpu(ext, lengths, family, page, dtype):
    rg = pc.build(lengths, dtype, page, family)
    sess = _session(dtype, page, rg.cap, lengths=lengths)
    _feed(sess, rg, lengths)
    assert sess.free_pages == pc.SPARE
    for b, n in enumerate(lengths):   # stored bytes are the ones .to() gives
        if n:
            assert torch.equal(_stored(sess, b, n),
                               rg.k[b, :, :n].view(torch.uint8))
    _guard(sess, rg, lengths)
    out = sess.attend(rg.q.cuda())
    rc.compare(rg, out, None, f"PagedDecodeSession.attend, page {page}")


def test_paged_session_gpu_generic_path(ext):
    """D = 64 and an fp32 pool do not take the paged kernel: the per-row
    gather + local_attention path, empty row included; graphed_step refuses
    them."""
    from tree_attention_torch_amd.ops.reference import flash_res_lse
    from tree_attention_torch_amd.session import PagedDecodeSession

    torch.manual_seed(3)
    for d, kvd in ((64, "bf16"), (128, "fp32")):
        b, h = 3, 2
        sess = PagedDecodeSession(b, h, d, max_tokens=512, pool_tokens=512,
                                  page=128, device="cuda", kv_dtype=kvd,
                                  block=128)
        lengths = (200, 0, 77)
        ks = torch.randn(b, h, 200, d, device="cuda").bfloat16()
        vs = torch.randn(b, h, 200, d, device="cuda").bfloat16()
        for row, n in enumerate(lengths):
            if n:
                sess.prefill(row, ks[row, :, :n - 1], vs[row, :, :n - 1])
        sess.append(ks[torch.arange(b), :, [199, 0, 76]][:, :, None],
                    vs[torch.arange(b), :, [199, 0, 76]][:, :, None],
                    [True, False, True])
        assert sess.totals == list(lengths) and sess.free_pages == 1
        q = torch.randn(b, h, 1, d, device="cuda").bfloat16()
        out = sess.attend(q)
        assert not out[1].any()
        for row in (0, 2):
            n = lengths[row]
            ref, _ = flash_res_lse(q[row:row + 1].cpu(),
                                   ks[row:row + 1, :, :n].cpu(),
                                   vs[row:row + 1, :, :n].cpu())
            torch.testing.assert_close(out[row:row + 1].cpu(), ref,
                                       rtol=2.5e-2, atol=2.5e-2)
        with pytest.raises(ValueError, match="paged cache kernel"):
            sess.graphed_step(q, ks[:, :, :1].contiguous(),
                              vs[:, :, :1].contiguous())


@pytest.mark.parametrize("dtype,page", [("bf16", 256), ("fp8", 128),
                                        ("bf16", 128), ("fp8", 256)])
def test_paged_graphed_step(ext, dtype, page):
    """One captured step replayed while row 0 goes 511 -> 512 -> 513: its
    third append opens a new page AND a new split at key 512 (the page is
    assigned eagerly, the static table carries it into the replay), row 1
    sits inactive and row 2 stays empty: every replay meets the oracle and
    is bit-equal to an eager twin session fed the same stream."""
    first = pc.build(rc.GRAPH_STEPS[0], dtype, page)
    sess, twin = (_session(dtype, page, lengths=rc.GRAPH_STEPS[-1])
                  for _ in range(2))
    for s in (sess, twin):
        _feed(s, first, rc.GRAPH_START)
    ks, vs = (t.cuda() for t in rc.stream(first))
    q_static = torch.zeros_like(first.q, device="cuda")
    k_static = torch.zeros(rc.B, rc.HKV, 1, rc.D, dtype=torch.bfloat16,
                           device="cuda")
    v_static = torch.zeros_like(k_static)
    replay = sess.graphed_step(q_static, k_static, v_static)
    # neither the warm-up nor the capture moved a length or took a page
    assert sess.totals == list(rc.GRAPH_START)
    assert sess.total_dev.tolist() == list(rc.GRAPH_START)
    assert sess.local_len_dev.tolist() == list(rc.GRAPH_START)
    assert sess.free_pages == twin.free_pages
    mask = list(rc.GRAPH_MASK)
    before = rc.GRAPH_START
    opened = []
    for lengths in rc.GRAPH_STEPS:
        rg = pc.build(lengths, dtype, page)
        bi = torch.arange(rc.B)
        at = torch.tensor(before)
        k_new, v_new = ks[bi, :, at][:, :, None], vs[bi, :, at][:, :, None]
        for s in (sess, twin):     # poison from the OLD lengths on: the
            _guard(s, rg, before)  # append lands on a guard row or free page
        q_static.copy_(rg.q)
        k_static.copy_(k_new)
        v_static.copy_(v_new)
        free = sess.free_pages
        out = replay(mask)
        opened.append(free - sess.free_pages)
        assert sess.totals == list(lengths)
        assert sess.local_len_dev.tolist() == list(lengths)
        rc.compare(rg, out, None, "graphed_step replay")
        twin.append(k_new, v_new, mask)
        eager = twin.attend(rg.q.cuda())
        assert torch.equal(out, eager), f"replay != eager twin at {lengths}"
        assert sess._pages == twin._pages
        assert torch.equal(sess.k_pool.view(torch.uint8),
                           twin.k_pool.view(torch.uint8))
        before = lengths
    assert opened == [0, 0, 1]     # key 512 of row 0


def test_paged_graphed_step_errors(ext):
    """replay() checks the host mirror before anything is launched: a row
    at its ceiling, then a pool with no page left."""
    from tree_attention_torch_amd.session import PagedDecodeSession

    sess = PagedDecodeSession(2, 2, 128, max_tokens=64, pool_tokens=256,
                              page=128, device="cuda", kv_dtype="bf16",
                              block=64)
    assert sess.capacity == 128 and sess.n_pages == 2
    new = torch.ones(2, 2, 1, 128, dtype=torch.bfloat16, device="cuda")
    q = torch.ones(2, 8, 1, 128, dtype=torch.bfloat16, device="cuda")
    sess.prefill(1, new[0].expand(2, 128, 128), new[0].expand(2, 128, 128))
    replay = sess.graphed_step(q, new, new)
    with pytest.raises(RuntimeError, match="capacity exceeded: row 1 "):
        replay()
    assert sess.totals == [0, 128] and sess.total_dev.tolist() == [0, 128]
    assert sess.free_pages == 1
    out = replay([True, False])
    assert sess.total_dev.tolist() == [1, 128] and sess.free_pages == 0
    assert torch.isfinite(out).all()

    small = PagedDecodeSession(2, 2, 128, max_tokens=512, pool_tokens=128,
                               page=128, device="cuda", kv_dtype="bf16",
                               block=64)
    replay = small.graphed_step(q, new, new)
    replay([False, True])
    with pytest.raises(RuntimeError, match="pool exhausted: row 0 "):
        replay()
    assert small.totals == [0, 1] and small.total_dev.tolist() == [0, 1]
    assert small.local_len_dev.tolist() == [0, 1]
    out = replay([False, True])
    assert small.total_dev.tolist() == [0, 2]
    assert not out[0].any() and torch.isfinite(out).all()


# --------------------------------------------------------------------------
# multi-rank (RCCL): auto-skips below 2 GPUs
# --------------------------------------------------------------------------
def _paged_rccl_worker(rank, world, port):
    import os

    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import paged_cases as pcw
    import ragged_cases as rcw
    from tree_attention_torch_amd.parallel.pg import cleanup, setup
    from tree_attention_torch_amd.session import PagedDecodeSession

    device = torch.device(f"cuda:{rank}")
    setup(rank, world)
    try:
        lengths, page = rcw.LENGTH_SETS[0], 128
        rg = pcw.build(lengths, "bf16", page)
        # half the slab a RaggedDecodeSession of this shape would reserve
        sess = PagedDecodeSession(rcw.B, rcw.HKV, rcw.D, max_tokens=2048,
                                  pool_tokens=rcw.B * 2048 // (2 * world)
                                  + rcw.B * page, page=page, device=device,
                                  kv_dtype="bf16", block=64)
        ks, vs = (t.to(device) for t in rcw.stream(rg))
        for b, n in enumerate(lengths):
            if n > 2:
                sess.prefill(b, ks[b, :, :n - 2], vs[b, :, :n - 2])
        while sess.totals != list(lengths):
            mask = [sess.totals[b] < lengths[b] for b in range(rcw.B)]
            at = torch.tensor(sess.totals).clamp(max=rcw.CAP - 1)
            bi = torch.arange(rcw.B)
            sess.append(ks[bi, :, at][:, :, None], vs[bi, :, at][:, :, None],
                        mask)
        assert sess.local_len_dev.tolist() == sess.local_lens
        assert sess.n_pages - sess.free_pages == \
            sum(pcw.pages_of(n, page) for n in sess.local_lens)
        for combine in ("allgather", "allreduce"):
            out = sess.attend(rg.q.to(device), combine=combine)
            torch.cuda.synchronize()
            rcw.compare(rg, out, None, f"rank {rank} {combine}")
    finally:
        cleanup()


@pytest.mark.skipif(NGPU < 2, reason=f"needs >=2 GPUs, have {NGPU}")
def test_rccl_paged_session():
    import torch.multiprocessing as mp

    mp.spawn(_paged_rccl_worker, args=(NGPU, _PORT), nprocs=NGPU, join=True)
