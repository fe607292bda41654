"""attend(shared=True) on the CPU (fp32 storage): the plan the rule predicts,
the oracle's numbers through the two torch passes, the upload counter, the
refusals, and world size 2 over gloo. The scenario is tests/shared_cases.py."""

import os

import pytest
import torch
import torch.multiprocessing as mp

import shared_cases as sc
from tree_attention_torch_amd.session import (PagedDecodeSession,
                                              RaggedDecodeSession, _n_local)


def _paged(page, **kw):
    kw = dict(dict(device="cpu", kv_dtype="fp32", block=256,
                   max_tokens=sc.CAP), **kw)
    n_pages = sc.pool_pages(page)
    return PagedDecodeSession(sc.B, sc.HKV, sc.D, pool_tokens=n_pages * page,
                              page=page, **kw)


def _loaded(page, layout="fork", **kw):
    sess = _paged(page, **kw)
    ks, vs = sc.load(sess, layout, "bf16")
    return sess, ks, vs


def _step(sess, ks, vs, layout, i):
    k_new, v_new = sc.step_tokens(ks, vs, layout, i)
    sess.append(k_new, v_new, sc.ACTIVE)


def _check(sess, layout, page, n, what=""):
    """shared=True against the oracle and against the plain attend."""
    cs = sc.at(layout, page, "bf16", n)
    assert tuple(sess.totals) == cs.lengths
    q = cs.q.float()
    sc.poison(sess, q)
    out = sess.attend(q, shared=True)
    sc.compare(cs, out, None, f"{what} n={n}")
    torch.testing.assert_close(out, sess.attend(q))
    sc.table_matches(sess)


# ---- the plan ----
@pytest.mark.parametrize("layout", sc.LAYOUTS)
@pytest.mark.parametrize("page", sc.PAGES)
def test_plan_of_the_scenario(layout, page):
    sess, ks, vs = _loaded(page, layout)
    assert sess.shared_plan(sc.HQ) == sc.EXPECT[page]
    # the helper's own statement of the rule agrees on the session's pages
    assert sess.shared_plan(sc.HQ) == sc.plan_of(
        sess._pages, sess.local_lens, sess._refs, page, 16 // (sc.HQ // sc.HKV))
    for i in range(sc.STEPS):
        _step(sess, ks, vs, layout, i)
        plan = sess.shared_plan(sc.HQ)
        sc.one_group_each(plan, sc.B)
        assert plan == sc.EXPECT[page], f"step {i + 1}"


# (event, what the rule predicts at page 128 / 256). P: the five / two full
# pages of the prompt every fork holds.
#   reset(0): the four forks are one family and tie: one group, led by row 1.
#   truncate(1, 300): row 1 keeps 2 / 1 full pages, sorts first (its run of
#     shared pages is a prefix of the others') and leads the group of four,
#     whose common run is row 1's; row 4 is cut off alone.
#   fork(1, 5, 650): a fork of a fork holds the same P pages: six rows, cut
#     into four and two.
#   Hq = 16 (two rows per group): a family of five is cut 2 + 2 + 1.
#   Hq = 2 (sixteen per group): one group of five.
EVENTS = {
    "reset_leader": {128: [([0], 0), ([1, 2, 3, 4], 640), ([5], 0)],
                     256: [([0], 0), ([1, 2, 3, 4], 512), ([5], 0)]},
    "truncate_member": {128: [([1, 0, 2, 3], 256), ([4], 0), ([5], 0)],
                        256: [([1, 0, 2, 3], 256), ([4], 0), ([5], 0)]},
    "fork_of_fork": {128: [([0, 1, 2, 3], 640), ([4, 5], 640)],
                     256: [([0, 1, 2, 3], 512), ([4, 5], 512)]},
    "two_per_group": {128: [([0, 1], 640), ([2, 3], 640), ([4], 0), ([5], 0)],
                      256: [([0, 1], 512), ([2, 3], 512), ([4], 0), ([5], 0)]},
    "sixteen_per_group": {128: [([0, 1, 2, 3, 4], 640), ([5], 0)],
                          256: [([0, 1, 2, 3, 4], 512), ([5], 0)]},
}


@pytest.mark.parametrize("event", sorted(EVENTS))
@pytest.mark.parametrize("page", sc.PAGES)
def test_plan_after(event, page):
    sess, _, _ = _loaded(page)
    hq = sc.HQ
    if event == "reset_leader":
        sess.reset(0)
    elif event == "truncate_member":
        sess.truncate(1, 300)
    elif event == "fork_of_fork":
        sess.fork(1, 5, 650)
    elif event == "two_per_group":
        hq = 16
    elif event == "sixteen_per_group":
        hq = 2
    plan = sess.shared_plan(hq)
    sc.one_group_each(plan, sc.B)
    assert plan == EVENTS[event][page]
    # and the two passes still give what the plain attend gives
    q = torch.randn(sc.B, hq, 1, sc.D, generator=torch.Generator().manual_seed(3))
    torch.testing.assert_close(sess.attend(q, shared=True), sess.attend(q))


def test_plan_arguments():
    sess, _, _ = _loaded(128)
    for bad in (0, 3, 34):
        with pytest.raises(ValueError, match="shared_plan"):
            sess.shared_plan(bad)
    assert sess.shared_plan() == sess.shared_plan(sc.HKV)


# ---- outputs and the upload counter ----
@pytest.mark.parametrize("layout", sc.LAYOUTS)
@pytest.mark.parametrize("page", sc.PAGES)
def test_outputs_and_uploads(layout, page):
    sess, ks, vs = _loaded(page, layout)
    assert sess.shared_plan_uploads == 0
    _check(sess, layout, page, 0, layout)
    assert sess.shared_plan_uploads == 1
    _step(sess, ks, vs, layout, 0)          # the copying step
    _check(sess, layout, page, 1, layout)
    steady = sess.shared_plan_uploads
    q = sc.at(layout, page, "bf16", sc.STEPS).q.float()
    for i in range(1, sc.STEPS):
        _step(sess, ks, vs, layout, i)
        if i % 16 == 0 or i > sc.STEPS - 4:
            sess.attend(q, shared=True)
    _check(sess, layout, page, sc.STEPS, layout)
    assert sess.shared_plan_uploads == steady, \
        "a steady decode step uploads nothing"
    sess.fork(1, 5, 650)
    sess.attend(q, shared=True)
    assert sess.shared_plan_uploads == steady + 1, "a fork moves the plan"
    sess.reset(0)
    out = sess.attend(q, shared=True)
    assert sess.shared_plan_uploads == steady + 2, "a reset moves the plan"
    assert torch.equal(out[0], torch.zeros_like(out[0]))
    torch.testing.assert_close(out, sess.attend(q))


# ---- refusals ----
def test_refusals():
    slab = RaggedDecodeSession(sc.B, sc.HKV, sc.D, max_tokens=sc.CAP,
                               device="cpu", kv_dtype="fp32")
    q = torch.zeros(sc.B, sc.HQ, 1, sc.D)
    with pytest.raises(ValueError, match="slab shares nothing"):
        slab.attend(q, shared=True)
    with pytest.raises(ValueError, match="slab shares nothing"):
        slab.graphed_step(q, q[:, :sc.HKV], q[:, :sc.HKV], shared=True)
    assert slab.attend(q).shape == q.shape      # shared=False: as before
    sess, _, _ = _loaded(128)
    with pytest.raises(ValueError, match="one query per row"):
        sess.attend(torch.zeros(sc.B, sc.HQ, 2, sc.D), shared=True)
    with pytest.raises(ValueError, match="Hq/Hkv"):
        sess.attend(torch.zeros(sc.B, 34, 1, sc.D), shared=True)
    with pytest.raises(ValueError, match="needs a GPU"):
        sess.graphed_step(q, q[:, :sc.HKV], q[:, :sc.HKV], shared=True)
    for fn in (sess.attend_many, sess.attend_tree):
        with pytest.raises(TypeError):
            fn(q, shared=True)


# ---- world size 2 ----
def _worker(rank, world, port):
    import sys

    import torch.distributed as dist

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        page, block, layout = 128, 64, "fork"
        sess, ks, vs = _loaded(page, layout, block=block)

        def look(n):
            cs = sc.at(layout, page, "bf16", n)
            want = [_n_local(t, block, rank, world) for t in sess.totals]
            assert sess.local_lens == want
            plan = sess.shared_plan(sc.HQ)
            sc.one_group_each(plan, sc.B)
            q = cs.q.float()
            sc.poison(sess, q)
            out = sess.attend(q, shared=True, combine="allgather")
            sc.compare(cs, out, None, f"rank {rank} n={n}")
            torch.testing.assert_close(out, sess.attend(q, combine="allgather"))

        look(0)
        # blocks of 64 tokens: the ranks hold different numbers of local
        # tokens of a row, hence of full pages; the group's prefix is the
        # shortest member's
        rows, prefix = sess.shared_plan(sc.HQ)[0]
        assert sorted(rows) == [0, 1, 2, 3]
        assert prefix == min(_n_local(t, block, rank, world) // page
                             for t in sess.totals[:4]) * page > 0
        for i in range(sc.STEPS):
            _step(sess, ks, vs, layout, i)
            if i == 0:
                look(1)
        look(sc.STEPS)
    finally:
        dist.destroy_process_group()


def test_shared_ws2():
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 2, 29787))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
