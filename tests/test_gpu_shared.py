"""Shared-prefix decode on the GPU: flash_attention_paged_shared over
hand-built pools and tables against the fp32 oracle, its refusals, and the
scenario of tests/shared_cases.py on a PagedDecodeSession, eager, captured and
over two ranks (what the inputs can see is proven on the CPU in
tests/test_shared_sensitivity.py)."""

import os

import pytest
import torch

import needle_cases as nc
import shared_cases as sc

pytestmark = pytest.mark.gpu

NGPU = torch.cuda.device_count() if torch.cuda.is_available() else 0
_PORT = 29694
SCALE = 1.0 / sc.D ** 0.5


@pytest.fixture(scope="module")
def ext():
    from tree_attention_torch_amd.ops import flash

    assert flash.hip_available(), "HIP extension must be built in-tree"
    assert not os.environ.get("TREE_ATTN_SPLIT_BLOCKS"), \
        "the 512-key split seam assumes the default split plan"
    return flash._load_extension()


# --------------------------------------------------------------------------
# the binding
# --------------------------------------------------------------------------
def _forks(n, prompt, fork, own=1):
    """A prompt row and n - 1 forks of it at `fork`, row b with own + b
    tokens of its own."""
    return ((-1, 0, prompt + own),) + tuple(
        (0, fork, fork + own + b) for b in range(1, n))


# name -> (rows, Hq, Hkv, capacity): (G, members per group), prefix
SHAPES = {
    # (4, 4) + a lone fifth + an empty row; prefix 640 across the split seam
    "scenario_n1": (sc.scenario("fork", 1), 8, 2, 1024),
    # the same before any append: row 2's suffix is empty
    "scenario_n0": (sc.scenario("fork", 0), 8, 2, 1024),
    # (4, 3), a prefix of one page (row 2 forked at 130 holds one full page)
    "three_of_four": (((-1, 0, 201), (0, 200, 201), (0, 130, 140)), 8, 2,
                      1024),
    # (1, 16): sixteen rows in one stream
    "sixteen": (_forks(16, 700, 700), 2, 2, 1024),
    # (16, 1): one row per group, every prefix 0
    "one_per_group": (_forks(2, 700, 700), 32, 2, 1024),
    # a family of 17 at G = 1: cut into 16 and 1
    "seventeen": (_forks(17, 700, 700), 2, 2, 1024),
}


def _case(shape, page, dtype):
    rows, hq, hkv, cap = SHAPES[shape]
    if page == 1024:    # one full page of 1024 and a tail, two table entries
        rows = tuple((s, f + 1024 if f else 0, n + 1024 if n else 0)
                     for s, f, n in rows)
        cap = 2048
    return sc.build(rows, hq, hkv, page, dtype, cap)


def _run(ext, cs, tables=None):
    members, counts, prefix, start = tables or cs.tables()
    lens = torch.tensor(cs.lengths, dtype=torch.long)
    out, lse = ext.flash_attention_paged_shared(
        cs.q.cuda(), cs.k_pool.cuda(), cs.v_pool.cuda(), cs.table.cuda(),
        lens.cuda(), members.cuda(), counts.cuda(), prefix.cuda(),
        start.cuda(), SCALE)
    torch.cuda.synchronize()
    return out, lse


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("page", [128, 1024])
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp8"])
def test_binding(ext, dtype, page, shape):
    cs = _case(shape, page, dtype)
    sc.one_group_each(cs.plan, len(cs.rows))
    if shape == "seventeen":
        assert sorted(len(r) for r, _ in cs.plan) == [1, 16]
    if shape == "one_per_group":
        assert all(p == 0 for _, p in cs.plan)
    elif page == 128 and shape == "three_of_four":
        assert cs.plan == [([0, 1, 2], 128)]
    elif page == 128:
        assert cs.plan[0][1] == 640
    else:
        assert cs.plan[0][1] == 1024
    out, lse = _run(ext, cs)
    sc.compare(cs, out, lse, shape)
    # two more groups without members change nothing
    out2, lse2 = _run(ext, cs, cs.tables(len(cs.plan) + 2))
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    # and the plain paged launch agrees at the same bars
    lens = torch.tensor(cs.lengths, dtype=torch.long).cuda()
    out3, lse3 = ext.flash_attention_paged(
        cs.q.cuda(), cs.k_pool.cuda(), cs.v_pool.cuda(), cs.table.cuda(),
        lens, SCALE)
    sc.compare(cs, out3, lse3, f"{shape}, plain")


def test_corrupt_group_stays_in_its_rows(ext):
    """Member ids outside [0, B) and a count above 16 / G are clamped: the
    rows the clamped ids name get wrong numbers, every other group's rows
    still match, and the call returns."""
    rows = ((-1, 0, 200), (-1, 0, 701), (1, 700, 701), (1, 640, 641),
            (1, 700, 704), (-1, 0, 150))
    cs = sc.build(rows, 8, 2, 128, "bf16", 1024)
    assert cs.plan == [([0], 0), ([1, 2, 3, 4], 640), ([5], 0)]
    members, counts, prefix, start = cs.tables()
    counts[2] = 0
    # group 0 takes rows 0 and 5, named by ids that clamp to them
    members[0, :4] = torch.tensor([-3, 11, 0, 5], dtype=torch.int32)
    counts[0], prefix[0] = 99, 128
    members[1, :4] = torch.tensor([1, 2, 3, 4], dtype=torch.int32)
    counts[1], prefix[1] = 4, 640
    out, lse = _run(ext, cs, (members, counts, prefix, start))
    keep = torch.tensor([1, 2, 3, 4])
    nc.compare(out.cpu()[keep], lse.cpu()[keep], cs.ref_out[keep],
               cs.ref_lse[keep], cs.kind)


def test_refusals(ext):
    cs = _case("scenario_n1", 128, "bf16")
    members, counts, prefix, start = (t.cuda() for t in cs.tables())
    q, kp, vp, tb = (t.cuda() for t in (cs.q, cs.k_pool, cs.v_pool, cs.table))
    lens = torch.tensor(cs.lengths, dtype=torch.long).cuda()

    def call(**kw):
        a = dict(q=q, k_pool=kp, v_pool=vp, page_table=tb, len_dev=lens,
                 members=members, counts=counts, prefix_len=prefix,
                 start=start, scale=SCALE)
        a.update(kw)
        return ext.flash_attention_paged_shared(**a)

    call()
    bad = {
        "Tq = 1": dict(q=q.expand(-1, -1, 2, -1).contiguous()),
        "members must be": dict(members=members.long()),
        "members must be contiguous int32": dict(members=members[:, :8]
                                                 .contiguous()),
        "device": dict(members=members.cpu()),
        "counts must be": dict(counts=counts[:-1]),
        "counts must be contiguous": dict(counts=counts.long()),
        "prefix_len must be": dict(prefix_len=prefix.int()),
        "start must be": dict(start=start[:-1]),
        "start must be contiguous": dict(start=start.int()),
        "head_dim must be 128": dict(q=q[..., :64].contiguous(),
                                     k_pool=kp[..., :64].contiguous(),
                                     v_pool=vp[..., :64].contiguous()),
        "G = Hq / Hkv <= 16": dict(q=torch.zeros(len(cs.rows), 34, 1, sc.D,
                                                 dtype=torch.bfloat16,
                                                 device="cuda")),
    }
    for match, kw in bad.items():
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------
# the session
# --------------------------------------------------------------------------
def _session(dtype, page, device="cuda", **kw):
    from tree_attention_torch_amd.session import PagedDecodeSession

    kw = dict(dict(max_tokens=sc.CAP, block=256), **kw)
    return PagedDecodeSession(sc.B, sc.HKV, sc.D,
                              pool_tokens=sc.pool_pages(page) * page,
                              page=page, device=device, kv_dtype=dtype, **kw)


def _check(sess, cs, what):
    q = cs.q.to(sess.device)
    sc.poison(sess, q)
    out = sess.attend(q, shared=True)
    sc.compare(cs, out, None, what)
    sc.compare(cs, sess.attend(q), None, f"{what}, plain")
    sc.table_matches(sess)
    assert sess.local_len_dev.tolist() == sess.local_lens


# pages more than one row holds after the load / after the first step, and the
# pages that step takes. Page 128: the five prompt pages and the tail page
# (rows 0, 1, 4; row 3 copied it when it took its own tokens); rows 0 and 1
# copy the tail, row 4 then owns it, row 2 opens a page at 640. Page 256: two
# prompt pages and the tail page [512, 768) (rows 0, 1, 2, 4); rows 0, 1 and 2
# copy it.
PAGES_EXPECT = {128: dict(shared_loaded=6, shared_after=5, taken=3),
                256: dict(shared_loaded=3, shared_after=2, taken=3)}


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("page", sc.PAGES)
def test_session_eager(ext, page, dtype):
    exp = PAGES_EXPECT[page]
    sess = _session(dtype, page)
    ks, vs = sc.load(sess, "fork", dtype, "cuda")
    assert sess.shared_plan(sc.HQ) == sc.EXPECT[page]
    assert sess.shared_pages == exp["shared_loaded"]
    _check(sess, sc.at("fork", page, dtype, 0), "loaded")
    uploads = sess.shared_plan_uploads
    assert uploads == 1
    last = sc.at("fork", page, dtype, sc.STEPS)
    for i in range(sc.STEPS):
        free = sess.free_pages
        k_new, v_new = sc.step_tokens(ks, vs, "fork", i)
        sess.append(k_new, v_new, sc.ACTIVE)
        if i == 0:
            assert free - sess.free_pages == exp["taken"]
            assert sess.shared_pages == exp["shared_after"]
            _check(sess, sc.at("fork", page, dtype, 1), "step 1")
        elif i % 8 == 0:
            sess.attend(last.q.cuda(), shared=True)
    _check(sess, last, f"step {sc.STEPS}")
    assert sess.shared_plan(sc.HQ) == sc.EXPECT[page]
    assert sess.shared_plan_uploads == uploads, "steady steps upload nothing"
    sess.reset(0)
    _check(sess, sc.at("fork", page, dtype, sc.STEPS, gone=(0,)),
           "row 0 gone")
    assert sess.shared_plan_uploads == uploads + 1


@pytest.mark.parametrize("dtype,page", [("bf16", 128), ("fp8", 256)])
def test_graphed_step_shared(ext, dtype, page):
    """graphed_step(shared=True) captured while only row 0 is live; then the
    forks; replays across the copying step and a page boundary, each bit-equal
    to an eager shared=True twin; then the leader leaves under the live
    capture."""
    sess, twin = _session(dtype, page), _session(dtype, page)
    ks, vs = (t.cuda() for t in sc.fed("fork", dtype))
    for s in (sess, twin):
        s.prefill(0, ks[0, :, :sc.PROMPT], vs[0, :, :sc.PROMPT])
    q_static = torch.zeros(sc.B, sc.HQ, 1, sc.D, dtype=torch.bfloat16,
                           device="cuda")
    k_static = torch.zeros(sc.B, sc.HKV, 1, sc.D, dtype=torch.bfloat16,
                           device="cuda")
    v_static = torch.zeros_like(k_static)
    replay = sess.graphed_step(q_static, k_static, v_static, shared=True)
    assert sess.totals == [sc.PROMPT, 0, 0, 0, 0, 0]
    assert sess.shared_plan(sc.HQ) == [([b], 0) for b in range(sc.B)]
    for s in (sess, twin):     # sc.load's forks, behind the prompt
        for b, (src, fork, n) in enumerate(sc.scenario("fork", 0)):
            if src >= 0:
                s.fork(src, b, fork)
                if n > fork:
                    s.prefill(b, ks[b, :, fork:n], vs[b, :, fork:n])
    last = sc.at("fork", page, dtype, sc.STEPS)
    for s in (sess, twin):
        sc.poison(s, last.q)
    q_static.copy_(last.q)
    for i in range(sc.STEPS):
        k_new, v_new = sc.step_tokens(ks, vs, "fork", i)
        k_static.copy_(k_new)
        v_static.copy_(v_new)
        out = replay(sc.ACTIVE)
        twin.append(k_new, v_new, sc.ACTIVE)
        assert torch.equal(out, twin.attend(q_static, shared=True)), \
            f"step {i}"
        if i == 0:
            first = sc.at("fork", page, dtype, 1)
            assert sess.shared_plan(sc.HQ) == sc.EXPECT[page]
            assert sess._pages == twin._pages
    sc.compare(last, out, None, f"captured, page {page}")
    sc.table_matches(sess)
    assert first.lengths[2] == 641
    # the leader leaves: the plan changes under the live capture
    sess.reset(0)
    gone = sc.at("fork", page, dtype, sc.STEPS + 1, gone=(0,))
    sc.poison(sess, gone.q)
    q_static.copy_(gone.q)
    k_new, v_new = sc.step_tokens(ks, vs, "fork", sc.STEPS)
    k_static.copy_(k_new)
    v_static.copy_(v_new)
    out = replay([False] + list(sc.ACTIVE[1:]))
    assert sess.shared_plan(sc.HQ)[:2] == [([0], 0), ([1, 2, 3, 4],
                                                     sc.EXPECT[page][0][1])]
    sc.compare(gone, out, None, "captured, row 0 gone")


# --------------------------------------------------------------------------
# multi-rank (RCCL): auto-skips below 2 GPUs
# --------------------------------------------------------------------------
def _shared_rccl_worker(rank, world, port):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import shared_cases as scw
    from tree_attention_torch_amd.parallel.pg import cleanup, setup
    from tree_attention_torch_amd.session import _n_local

    device = torch.device(f"cuda:{rank}")
    setup(rank, world)
    try:
        page, dtype, block = 128, "bf16", 64
        sess = _session(dtype, page, device=device, block=block)
        ks, vs = scw.load(sess, "fork", dtype, device)
        last = scw.at("fork", page, dtype, scw.STEPS)
        scw.poison(sess, last.q)
        for i in range(scw.STEPS):
            sess.append(*scw.step_tokens(ks, vs, "fork", i), scw.ACTIVE)
        assert sess.local_lens == [_n_local(n, block, rank, world)
                                   for n in last.lengths]
        scw.one_group_each(sess.shared_plan(scw.HQ), scw.B)
        scw.table_matches(sess)
        for combine in ("allgather", "allreduce"):
            out = sess.attend(last.q.to(device), combine=combine, shared=True)
            torch.cuda.synchronize()
            scw.compare(last, out, None, f"rank {rank} {combine}")
    finally:
        cleanup()


@pytest.mark.skipif(NGPU < 2, reason=f"needs >=2 GPUs, have {NGPU}")
def test_rccl_shared_session():
    import torch.multiprocessing as mp

    mp.spawn(_shared_rccl_worker, args=(NGPU, _PORT), nprocs=NGPU, join=True)
