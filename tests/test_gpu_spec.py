"""Multi-token verify on the GPU: the multi-token append kernel against a
host model, the visible-length decode kernels on the needle inputs of
tests/spec_cases.py (what they can see is proven on the CPU in
tests/test_spec_sensitivity.py), and the sessions end to end: eager,
graphed, the generic fallback, slab and paged."""

import pytest
import torch

import needle_cases as nc
import paged_cases as pc
import ragged_cases as rc
import spec_cases as sc

pytestmark = pytest.mark.gpu

NGPU = torch.cuda.device_count() if torch.cuda.is_available() else 0
_PORT = 29680
PAGE = 128
SCALE = 1.0 / sc.D ** 0.5
PARAMS = [pytest.param(c, id=sc.case_id(c)) for c in sc.CASES]
LAYOUTS = ("slab", "paged")


@pytest.fixture(scope="module")
def ext():
    from tree_attention_torch_amd.ops import flash

    assert flash.hip_available(), "HIP extension must be built in-tree"
    return flash._load_extension()


def _len_dev(lengths):
    return torch.tensor(list(lengths), dtype=torch.long, device="cuda")


# --------------------------------------------------------------------------
# kv_cache_append_n / kv_pool_append_n against a host model
# --------------------------------------------------------------------------
def _place(t, block, world):
    return (t // block) % world, block * ((t // block) // world) + t % block


def _n_local(t, block, rank, world):
    return sum(1 for x in range(t) if (x // block) % world == rank)


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rank,world,block", [(1, 3, 4), (0, 1, 64)])
def test_kv_append_n(ext, dtype, layout, rank, world, block):
    """12 steps of T in {4, 3, 16, 1} with changing counts (0 included) into
    sentinel-filled storage: the stored rows are bit equal to what the host
    formula places, vis / local_len / total equal the host model after
    every step, and every other byte still holds the sentinel. At (0, 1,
    64) rows run past the slab's capacity, or the page table, and store
    nothing there."""
    bsz, hkv, d = 4, 2, 128
    td = rc._TD[dtype]
    g = torch.Generator().manual_seed(rc.SEED + block)
    esz = torch.empty(0, dtype=td).element_size()
    if layout == "slab":
        cap, start = 64, [0, 3, 30, 62]
        shape = (bsz, hkv, cap, d * esz)
    else:
        cap, start = 2 * PAGE, [0, 3, 130, 250]
        shape = (10, hkv, PAGE, d * esz)      # pages 8 and 9 belong to no row
        table_h = torch.tensor([[3, 6], [0, 5], [1, 7], [2, 4]],
                               dtype=torch.int32)
        table = table_h.cuda()
    kc = torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda").view(td)
    vc = torch.full(shape, 0x5A, dtype=torch.uint8, device="cuda").view(td)
    want_k, want_v = kc.cpu().clone(), vc.cpu().clone()
    total = torch.tensor(start, dtype=torch.long, device="cuda")
    # local_len starts at values a count of 0 must leave alone
    llen = torch.tensor([5, 6, 7, 8], dtype=torch.long, device="cuda")
    h_total, h_llen = list(start), [5, 6, 7, 8]
    overran = False
    for step in range(12):
        t = (4, 3, 16, 1)[step % 4]
        counts = [(step * 7 + b * 3) % (t + 1) for b in range(bsz)]
        counts[step % bsz] = 0 if step % 3 == 0 else counts[step % bsz]
        k_new = torch.randn(bsz, hkv, t, d, generator=g).to(td)
        v_new = torch.randn(bsz, hkv, t, d, generator=g).to(td)
        vis = torch.full((bsz, t), -7, dtype=torch.long, device="cuda")
        cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
        if layout == "slab":
            ext.kv_cache_append_n(kc, vc, k_new.cuda(), v_new.cuda(), total,
                                  llen, cnt, vis, block, rank, world)
        else:
            ext.kv_pool_append_n(kc, vc, table, k_new.cuda(), v_new.cuda(),
                                 total, llen, cnt, vis, block, rank, world)
        h_vis = []
        for b, c in enumerate(counts):
            t0 = h_total[b]
            for i in range(c):
                owner, pos = _place(t0 + i, block, world)
                if owner != rank:
                    continue
                if pos >= cap:
                    overran = True
                elif layout == "slab":
                    want_k[b, :, pos] = k_new[b, :, i]
                    want_v[b, :, pos] = v_new[b, :, i]
                else:
                    pid = int(table_h[b, pos // PAGE])
                    want_k[pid, :, pos % PAGE] = k_new[b, :, i]
                    want_v[pid, :, pos % PAGE] = v_new[b, :, i]
            h_vis.append([_n_local(t0 + (min(i, c - 1) + 1 if c else 0),
                                   block, rank, world) for i in range(t)])
            if c:
                h_llen[b] = _n_local(t0 + c, block, rank, world)
            h_total[b] = t0 + c
        assert vis.tolist() == h_vis, f"step {step}"
        assert total.tolist() == h_total and llen.tolist() == h_llen, \
            f"step {step}"
    assert overran or world > 1     # (0, 1, 64) overruns rows
    assert torch.equal(kc.cpu().view(torch.uint8), want_k.view(torch.uint8))
    assert torch.equal(vc.cpu().view(torch.uint8), want_v.view(torch.uint8))


def test_kv_append_n_checks(ext):
    kc = torch.zeros(2, 2, 8, 128, dtype=torch.bfloat16, device="cuda")
    new = torch.zeros(2, 2, 3, 128, dtype=torch.bfloat16, device="cuda")
    lens = torch.zeros(2, dtype=torch.long, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    vis = torch.zeros(2, 3, dtype=torch.long, device="cuda")

    def call(new=new, cnt=cnt, vis=vis, rank=0, world=1):
        ext.kv_cache_append_n(kc, kc.clone(), new, new, lens, lens.clone(),
                              cnt, vis, 4, rank, world)

    call()
    with pytest.raises(RuntimeError, match="rank"):
        call(rank=1)
    with pytest.raises(RuntimeError, match="T must be in 1..16"):
        big = torch.zeros(2, 2, 17, 128, dtype=torch.bfloat16, device="cuda")
        call(new=big, vis=torch.zeros(2, 17, dtype=torch.long, device="cuda"))
    with pytest.raises(RuntimeError, match="counts"):
        call(cnt=cnt.long())
    with pytest.raises(RuntimeError, match="vis"):
        call(vis=vis[:, :2].contiguous())
    with pytest.raises(RuntimeError, match="dtype"):
        call(new=new.half())


# --------------------------------------------------------------------------
# flash_attention_cache_qlen / flash_attention_paged_qlen over hand-built vis
# --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("case", PARAMS)
def test_qlen_kernels(ext, case, dtype):
    """Slab and paged meet the oracle at the suite's bars, and are bit
    equal to each other: same arithmetic, only the addresses differ."""
    nc.assert_default_split_plan()
    sp = sc.build(case, dtype)
    q, vis = sp.q.cuda(), sp.vis.cuda()
    out, lse = ext.flash_attention_cache_qlen(
        q, sp.k_cache.cuda(), sp.v_cache.cuda(), _len_dev(sp.lengths), vis,
        SCALE)
    sc.compare(sp, out, lse, "flash_attention_cache_qlen")
    pl = pc.scatter(sp, PAGE)
    out_p, lse_p = ext.flash_attention_paged_qlen(
        q, pl.k_pool.cuda(), pl.v_pool.cuda(), pl.table.cuda(),
        _len_dev(sp.lengths), vis, SCALE)
    sc.compare(sp, out_p, lse_p, "flash_attention_paged_qlen")
    assert torch.equal(out, out_p) and torch.equal(lse, lse_p)


def test_qlen_checks(ext):
    sp = sc.build(sc.CASES[0], "bf16")
    q, k, v = sp.q.cuda(), sp.k.cuda(), sp.v.cuda()
    lens, vis = _len_dev(sp.lengths), sp.vis.cuda()
    with pytest.raises(RuntimeError, match="vis"):
        ext.flash_attention_cache_qlen(q, k, v, lens, vis[:, :2].contiguous(),
                                       SCALE)
    with pytest.raises(RuntimeError, match="vis"):
        ext.flash_attention_cache_qlen(q, k, v, lens, vis.int(), SCALE)
    with pytest.raises(RuntimeError, match="len_dev"):
        ext.flash_attention_cache_qlen(q, k, v, lens[:1], vis, SCALE)
    with pytest.raises(RuntimeError, match="GQA group size"):
        ext.flash_attention_cache_qlen(
            torch.zeros(sc.B, 34, 2, sc.D, dtype=torch.bfloat16,
                        device="cuda"), k, v, lens, vis[:, :2].contiguous(),
            SCALE)


# --------------------------------------------------------------------------
# sessions
# --------------------------------------------------------------------------
def _session(layout, dtype, **kw):
    from tree_attention_torch_amd.session import (PagedDecodeSession,
                                                  RaggedDecodeSession)

    # capacity = (ceil(max_tokens / block) + 1) blocks = 1024
    if layout == "slab":
        sess = RaggedDecodeSession(sc.B, sc.HKV, sc.D, max_tokens=sc.CAP - 256,
                                   device="cuda", kv_dtype=dtype, block=256,
                                   **kw)
    else:
        sess = PagedDecodeSession(sc.B, sc.HKV, sc.D, max_tokens=sc.CAP - 256,
                                  pool_tokens=16 * PAGE, page=PAGE,
                                  device="cuda", kv_dtype=dtype, block=256,
                                  **kw)
    assert sess.capacity == sc.CAP
    return sess


def _prefill(sess, sp):
    ks, vs, kd, vd = (t.cuda() for t in sc.stream(sp))
    for b, n in enumerate(sp.starts):
        if n > sess.totals[b]:
            sess.prefill(b, ks[b, :, sess.totals[b]:n],
                         vs[b, :, sess.totals[b]:n])
    assert sess.totals == list(sp.starts)
    return kd, vd


def _guard(sess, sp, lengths):
    """The guard pattern at and past lengths[b], in place (a captured step
    holds the storage's address). Paged: also decoy K / NaN V on every free
    page, and every table entry past a row's live pages names a free page
    (tests/test_gpu_paged.py)."""
    if not hasattr(sess, "k_pool"):
        rc.write_guards(sess.k, sess.v, sp.q, lengths)
        return
    td = sess.k_pool.dtype
    gk, gv = rc.guard_fill(sp.q.cpu(), sp.cap)
    assert sess.free_pages >= 1
    for b, n in enumerate(lengths):
        live = len(sess._pages[b])
        assert live == pc.pages_of(n, PAGE)
        if n % PAGE:
            pid, lo = sess._pages[b][-1], n % PAGE
            at = (live - 1) * PAGE
            sess.k_pool[pid, :, lo:] = gk[b, :, at + lo:at + PAGE].to(
                device="cuda", dtype=td)
            sess.v_pool[pid, :, lo:] = gv[b, :, at + lo:at + PAGE].to(
                device="cuda", dtype=td)
        sess.page_table[b, live:] = sess._free[0]
    for pid in sess._free:
        sess.k_pool[pid] = gk[pid % sc.B, :, :PAGE].to(device="cuda", dtype=td)
        sess.v_pool[pid] = float("nan")


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", PARAMS)
def test_spec_session_eager(ext, case, layout, dtype):
    sp = sc.build(case, dtype)
    sess = _session(layout, dtype)
    kd, vd = _prefill(sess, sp)
    _guard(sess, sp, sp.starts)     # the drafts land on the first guard rows
    sess.append_many(kd, vd, sp.counts)
    assert sess.totals == list(sp.lengths)
    assert sess.total_dev.tolist() == list(sp.lengths)
    assert sess.local_len_dev.tolist() == list(sp.lengths)
    assert sess._vis_dev(sp.t).tolist() == sp.vis.tolist()
    _guard(sess, sp, sp.lengths)
    out = sess.attend_many(sp.q.cuda())
    sc.compare(sp, out, None, f"{layout} attend_many")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_spec_session_generic_path(ext, layout):
    """An fp32 cache does not take the zero-copy kernels: the per-row,
    per-query-position loop over local_attention meets the same oracle, and
    graphed_step_many refuses the session."""
    sp = sc.build(sc.CASES[2], "bf16")
    sess = _session(layout, "fp32")
    kd, vd = _prefill(sess, sp)
    sess.append_many(kd, vd, sp.counts)
    assert sess._vis_dev(sp.t).tolist() == sp.vis.tolist()
    _guard(sess, sp, sp.lengths)
    out = sess.attend_many(sp.q.cuda())
    sc.compare(sp, out, None, f"{layout} fp32 fallback")
    with pytest.raises(ValueError, match="does not take this session"):
        sess.graphed_step_many(sp.q.cuda(), kd, vd)


# (starts, counts) of three replays; between them every row is truncated to
# the next step's start: rejected drafts leave, row 2 drops back onto its
# first page (130 / 131 -> 128) and row 0 crosses the split seam
GRAPH_STEPS = {
    4: (((510, 62, 126, 0), (4, 2, 0, 3)),
        ((512, 64, 126, 1), (1, 4, 4, 0)),
        ((513, 68, 128, 1), (4, 4, 4, 4))),
    6: (((510, 62, 126, 0), (6, 2, 0, 3)),
        ((512, 64, 126, 1), (1, 6, 5, 0)),
        ((513, 70, 128, 1), (6, 6, 6, 6))),
}


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("t", [4, 6])
def test_graphed_step_many(ext, t, layout, dtype):
    """One captured verify step (T = 6: two attention launches) replayed
    three times with changing counts and a truncate of every row between
    replays: every replay meets the oracle and is bit-equal to an eager twin
    session fed the same stream."""
    steps = [sc.build((t,) + s, dtype) for s in GRAPH_STEPS[t]]
    sess, twin = _session(layout, dtype), _session(layout, dtype)
    for s in (sess, twin):
        _prefill(s, steps[0])
    q_static = torch.zeros_like(steps[0].q, device="cuda")
    k_static = torch.zeros(sc.B, sc.HKV, t, sc.D, dtype=torch.bfloat16,
                           device="cuda")
    v_static = torch.zeros_like(k_static)
    replay = sess.graphed_step_many(q_static, k_static, v_static)
    # neither the warm-up nor the capture moved a length
    assert sess.totals == list(steps[0].starts)
    assert sess.total_dev.tolist() == list(steps[0].starts)
    assert sess.local_len_dev.tolist() == list(steps[0].starts)
    for sp in steps:
        for s in (sess, twin):
            for b, n in enumerate(sp.starts):
                s.truncate(b, n)
            assert s.totals == list(sp.starts)
            assert s.local_len_dev.tolist() == list(sp.starts)
            _guard(s, sp, sp.starts)
        _, _, kd, vd = (x.cuda() for x in sc.stream(sp))
        q_static.copy_(sp.q)
        k_static.copy_(kd)
        v_static.copy_(vd)
        out = replay(list(sp.counts))
        assert sess.totals == list(sp.lengths)
        assert sess.local_len_dev.tolist() == list(sp.lengths)
        assert sess._vis_dev(t).tolist() == sp.vis.tolist()
        sc.compare(sp, out, None, "graphed_step_many replay")
        twin.append_many(kd, vd, sp.counts)
        eager = twin.attend_many(sp.q.cuda())
        assert torch.equal(out, eager), f"replay != eager twin at {sp.starts}"
    if layout == "paged":
        assert [len(p) for p in sess._pages] == \
            [pc.pages_of(n, PAGE) for n in steps[-1].lengths]
        assert sess.free_pages == twin.free_pages


def test_graphed_step_many_capacity(ext):
    """replay() checks the host mirror before anything is launched."""
    from tree_attention_torch_amd.session import RaggedDecodeSession

    sess = RaggedDecodeSession(2, 2, 128, max_tokens=64, device="cuda",
                               kv_dtype="bf16", block=64)
    new = torch.ones(2, 2, 3, 128, dtype=torch.bfloat16, device="cuda")
    q = torch.ones(2, 8, 3, 128, dtype=torch.bfloat16, device="cuda")
    sess.prefill(1, new[0, :, :1].expand(2, 126, 128),
                 new[0, :, :1].expand(2, 126, 128))
    replay = sess.graphed_step_many(q, new, new)
    with pytest.raises(RuntimeError, match="row 1 "):
        replay()
    assert sess.totals == [0, 126] and sess.total_dev.tolist() == [0, 126]
    out = replay([3, 2])
    assert sess.total_dev.tolist() == [3, 128]
    assert sess.local_len_dev.tolist() == [3, 128]
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_t1_equals_append_attend(ext, layout, dtype):
    """append_many with T = 1 and all-ones counts, then attend_many, is
    append then attend bit for bit, in the cache and in the output."""
    sp = sc.build((1, (510, 62, 126, 0), (1, 1, 1, 1)), dtype)
    one, many = _session(layout, dtype), _session(layout, dtype)
    for s in (one, many):
        kd, vd = _prefill(s, sp)
    one.append(kd, vd)
    many.append_many(kd, vd, [1] * sc.B)
    assert one.totals == many.totals
    assert one.local_len_dev.tolist() == many.local_len_dev.tolist()
    for s in (one, many):
        _guard(s, sp, sp.lengths)
    q = sp.q.cuda()
    out_one, out_many = one.attend(q), many.attend_many(q)
    sc.compare(sp, out_many, None, "T = 1 attend_many")
    assert torch.equal(out_one, out_many)
    for a, b in zip(one._rows(0, 511), many._rows(0, 511)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# --------------------------------------------------------------------------
# multi-rank (RCCL): auto-skips below 2 GPUs
# --------------------------------------------------------------------------
def _spec_rccl_worker(rank, world, port):
    import os

    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import spec_cases as scw
    from tree_attention_torch_amd.parallel.pg import cleanup, setup
    from tree_attention_torch_amd.session import RaggedDecodeSession

    device = torch.device(f"cuda:{rank}")
    setup(rank, world)
    try:
        sp = scw.build(scw.CASES[2], "bf16")
        # block 64: the drafts at 62 and at 510 cross owners
        sess = RaggedDecodeSession(scw.B, scw.HKV, scw.D, max_tokens=2048,
                                   device=device, kv_dtype="bf16", block=64)
        ks, vs, kd, vd = (t.to(device) for t in scw.stream(sp))
        for b, n in enumerate(sp.starts):
            if n:
                sess.prefill(b, ks[b, :, :n], vs[b, :, :n])
        sess.append_many(kd, vd, sp.counts)
        assert sess.local_len_dev.tolist() == sess.local_lens
        assert sess._vis_dev(sp.t).tolist() == sess._spec[1]
        for combine in ("allgather", "allreduce"):
            out = sess.attend_many(sp.q.to(device), combine=combine)
            torch.cuda.synchronize()
            scw.compare(sp, out, None, f"rank {rank} {combine}")
    finally:
        cleanup()


@pytest.mark.skipif(NGPU < 2, reason=f"needs >=2 GPUs, have {NGPU}")
def test_rccl_spec_session():
    import torch.multiprocessing as mp

    mp.spawn(_spec_rccl_worker, args=(NGPU, _PORT), nprocs=NGPU, join=True)
