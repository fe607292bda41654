"""Multi-token verify on the CPU: append_many / attend_many / truncate of
RaggedDecodeSession and PagedDecodeSession against the fp32 oracle on each
query's own prefix, single rank and under gloo at world sizes 2 and 4."""

import os
import random

import pytest
import torch
import torch.multiprocessing as mp

from tree_attention_torch_amd.ops.reference import flash_res_lse
from tree_attention_torch_amd.session import (PagedDecodeSession,
                                              RaggedDecodeSession, _n_local)

B, HKV, HQ, D, T_MAX = 3, 2, 4, 16, 200


def _make(kind, block=4, max_tokens=256, **kw):
    if kind == "paged":
        return PagedDecodeSession(B, HKV, D, max_tokens=max_tokens,
                                  pool_tokens=kw.pop("pool_tokens", 2048),
                                  page=128, device="cpu", kv_dtype="fp32",
                                  block=block, **kw)
    return RaggedDecodeSession(B, HKV, D, max_tokens=max_tokens, device="cpu",
                               kv_dtype="fp32", block=block, **kw)


def _streams(seed=0):
    g = torch.Generator().manual_seed(seed)
    ks = torch.randn(B, HKV, T_MAX, D, generator=g)
    vs = torch.randn(B, HKV, T_MAX, D, generator=g)
    return ks, vs


def _check_mirror(sess):
    assert sess.total_dev.tolist() == sess.totals
    assert sess.local_len_dev.tolist() == sess.local_lens
    assert sess.local_lens == [
        _n_local(t, sess.block, sess.rank, sess.world) for t in sess.totals]


def _verify_step(sess, ks, vs, t, counts, gen, combine="auto"):
    """One append_many + attend_many, checked against the oracle: query i
    of row b sees global tokens [0, before[b] + min(i, c - 1)] (c = 0: the
    whole sequence)."""
    before = list(sess.totals)
    k_new = torch.stack([ks[b, :, n:n + t] for b, n in enumerate(before)])
    v_new = torch.stack([vs[b, :, n:n + t] for b, n in enumerate(before)])
    sess.append_many(k_new, v_new, counts)
    cl = [t] * B if counts is None else list(counts)
    assert sess.totals == [n + c for n, c in zip(before, cl)]
    _check_mirror(sess)
    q = torch.randn(B, HQ, t, D, generator=gen)
    out = sess.attend_many(q, combine=combine)
    assert out.shape == (B, HQ, t, D)
    for b in range(B):
        for i in range(t):
            n = before[b] + (min(i, cl[b] - 1) + 1 if cl[b] else 0)
            if n == 0:
                assert not out[b, :, i].any(), (b, i)
                continue
            ref, _ = flash_res_lse(q[b:b + 1, :, i:i + 1], ks[b:b + 1, :, :n],
                                   vs[b:b + 1, :, :n])
            torch.testing.assert_close(out[b:b + 1, :, i:i + 1], ref,
                                       rtol=1e-5, atol=1e-5)
    return before, cl


def _run_steps(sess, seed, combine="auto"):
    """Prompts, then verify steps of T in {1, 3, 4, 6} with changing counts,
    each followed by a truncate to a random number of accepted drafts."""
    ks, vs = _streams(seed)
    rng = random.Random(seed)      # the same draws on every rank
    gen = torch.Generator().manual_seed(seed + 1)
    for b, n in enumerate((0, 5, 127)):
        if n:
            sess.prefill(b, ks[b, :, :n], vs[b, :, :n])
    for step, t in enumerate((3, 4, 6, 1, 4, 3)):
        counts = None if step == 0 else [rng.randint(0, t) for _ in range(B)]
        before, cl = _verify_step(sess, ks, vs, t, counts, gen, combine)
        for b in range(B):
            keep = rng.randint(0, cl[b])
            sess.truncate(b, before[b] + keep)
        _check_mirror(sess)
    # what is left is exactly the accepted prefix of every stream
    q = torch.randn(B, HQ, 1, D, generator=gen)
    out = sess.attend(q, combine=combine)
    for b, n in enumerate(sess.totals):
        if n == 0:
            assert not out[b].any()
            continue
        ref, _ = flash_res_lse(q[b:b + 1], ks[b:b + 1, :, :n],
                               vs[b:b + 1, :, :n])
        torch.testing.assert_close(out[b:b + 1], ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("kind", ["ragged", "paged"])
def test_spec_session_single_rank_cpu(kind):
    _run_steps(_make(kind), seed=0)


def _worker(rank, world, port, kind):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # block 2: the drafts of one step cross owners
        sess = _make(kind, block=2)
        assert (sess.rank, sess.world) == (rank, world)
        _run_steps(sess, seed=3, combine="allgather")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,kind,port", [(2, "ragged", 29781),
                                             (4, "ragged", 29782),
                                             (2, "paged", 29783)])
def test_spec_session_sharded_gloo(world, kind, port):
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, world, port, kind))
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


@pytest.mark.parametrize("kind", ["ragged", "paged"])
def test_truncate_equals_fresh_session(kind):
    """Verify 4 drafts, accept (2, 0, 3) of them: a T = 1 attend equals a
    fresh session fed only the accepted tokens, bit for bit."""
    ks, vs = _streams(5)
    starts, accept = (126, 0, 9), (2, 0, 3)
    sess, fresh = _make(kind), _make(kind)
    for b, n in enumerate(starts):
        if n:
            sess.prefill(b, ks[b, :, :n], vs[b, :, :n])
    k_new = torch.stack([ks[b, :, n:n + 4] for b, n in enumerate(starts)])
    v_new = torch.stack([vs[b, :, n:n + 4] for b, n in enumerate(starts)])
    sess.append_many(k_new, v_new, [4, 4, 3])
    for b in range(B):
        sess.truncate(b, starts[b] + accept[b])
        n = starts[b] + accept[b]
        if n:
            fresh.prefill(b, ks[b, :, :n], vs[b, :, :n])
    assert sess.totals == fresh.totals
    assert sess.local_lens == fresh.local_lens
    _check_mirror(sess)
    q = torch.randn(B, HQ, 1, D)
    assert torch.equal(sess.attend(q), fresh.attend(q))
    with pytest.raises(RuntimeError, match="attend_many"):
        sess.attend_many(torch.randn(B, HQ, 4, D))   # the lengths moved
    with pytest.raises(ValueError, match="truncate"):
        sess.truncate(0, sess.totals[0] + 1)
    with pytest.raises(ValueError, match="truncate"):
        sess.truncate(0, -1)


def test_paged_truncate_hands_pages_back():
    ks, vs = _streams(6)
    sess = _make("paged", block=256, max_tokens=512)
    sess.prefill(0, ks[0, :, :126], vs[0, :, :126])
    sess.prefill(2, ks[2, :, :10], vs[2, :, :10])
    assert [len(p) for p in sess._pages] == [1, 0, 1]
    free = sess.free_pages
    k_new = torch.stack([ks[b, :, n:n + 4] for b, n in enumerate(sess.totals)])
    sess.append_many(k_new, k_new, [4, 0, 4])    # row 0: 126 -> 130
    assert len(sess._pages[0]) == 2 and sess.free_pages == free - 1
    second = sess._pages[0][1]
    sess.truncate(0, 129)                         # still on the second page
    assert sess._pages[0][1] == second and sess.free_pages == free - 1
    sess.truncate(0, 128)                         # exactly one page
    assert len(sess._pages[0]) == 1 and sess.free_pages == free
    assert sess._free[-1] == second               # the next one handed out
    sess.append_many(k_new, k_new, [0, 1, 0])     # row 1's first page
    assert sess._pages[1] == [second]
    assert int(sess.page_table[1, 0]) == second
    sess.truncate(1, 0)
    assert sess._pages[1] == [] and sess._free[-1] == second
    # reset keeps its behaviour
    held = list(sess._pages[0])
    sess.reset(0)
    assert sess._pages[0] == [] and sess._free[-1] == held[0]


def _state(sess):
    st = [list(sess.totals), list(sess.local_lens), sess.total_dev.clone(),
          sess.local_len_dev.clone()]
    if isinstance(sess, PagedDecodeSession):
        st += [list(sess._free), [list(p) for p in sess._pages],
               sess.k_pool.clone(), sess.page_table.clone()]
    else:
        st += [sess.k.clone(), sess.v.clone()]
    return st


def _same_state(a, b):
    return all(torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y
               for x, y in zip(a, b))


def test_capacity_error_raises_before_any_state_moves():
    sess = RaggedDecodeSession(2, 2, 16, max_tokens=8, device="cpu",
                               kv_dtype="fp32", block=4)
    assert sess.capacity == 12
    sess.k.zero_(), sess.v.zero_()
    one = torch.ones(2, 2, 4, 16)
    sess.append_many(one, one, [4, 4])
    sess.append_many(one, one, [2, 4])
    sess.append_many(one, one, [0, 2])
    assert sess.totals == [6, 10]
    before = _state(sess)
    with pytest.raises(RuntimeError, match=r"capacity exceeded: row 1 "):
        sess.append_many(2 * one, 2 * one, [4, 3])   # row 0 fits, row 1 not
    assert _same_state(before, _state(sess))
    sess.append_many(one, one, [4, 2])               # this much still fits
    assert sess.totals == [10, 12]


def test_pool_exhausted_raises_before_any_state_moves():
    sess = PagedDecodeSession(2, 2, 16, max_tokens=512, pool_tokens=256,
                              page=128, device="cpu", kv_dtype="fp32",
                              block=256)
    assert sess.n_pages == 2
    sess.k_pool.zero_(), sess.v_pool.zero_()
    row = torch.ones(2, 127, 16)
    sess.prefill(0, row, row)
    sess.prefill(1, row, row)
    assert sess.free_pages == 0
    one = torch.ones(2, 2, 4, 16)
    before = _state(sess)
    with pytest.raises(RuntimeError, match=r"pool exhausted: row 0 "):
        sess.append_many(one, one, [2, 1])   # row 0 needs a page, none free
    assert _same_state(before, _state(sess))
    sess.append_many(one, one, [1, 1])       # the last slot of each page
    assert sess.totals == [128, 128] and sess.free_pages == 0


def test_argument_errors():
    sess = _make("ragged")
    k3 = torch.zeros(B, HKV, 3, D)
    with pytest.raises(RuntimeError, match="attend_many"):
        sess.attend_many(torch.zeros(B, HQ, 3, D))   # before any append_many
    with pytest.raises(ValueError, match="append_many"):
        sess.append_many(torch.zeros(B, HKV, 17, D), torch.zeros(B, HKV, 17, D))
    with pytest.raises(ValueError, match="append_many"):
        sess.append_many(k3[:, :, :0], k3[:, :, :0])
    with pytest.raises(ValueError, match="append_many"):
        sess.append_many(k3, k3[:, :, :2])
    with pytest.raises(ValueError, match="append_many"):
        sess.append_many(k3[:2], k3[:2])
    with pytest.raises(ValueError, match=r"counts\[1\] = 4"):
        sess.append_many(k3, k3, [3, 4, 0])
    with pytest.raises(ValueError, match=r"counts\[0\] = -1"):
        sess.append_many(k3, k3, [-1, 0, 0])
    with pytest.raises(ValueError, match="counts has 2"):
        sess.append_many(k3, k3, [1, 1])
    assert sess.totals == [0, 0, 0]
    sess.append_many(k3, k3, torch.tensor([3, 1, 0]))
    assert sess.totals == [3, 1, 0]
    with pytest.raises(ValueError, match="T = 3"):
        sess.attend_many(torch.zeros(B, HQ, 4, D))   # a wrong T
    with pytest.raises(ValueError, match="attend_many"):
        sess.attend_many(torch.zeros(B + 1, HQ, 3, D))
    out = sess.attend_many(torch.zeros(B, HQ, 3, D))
    assert not out[2].any()      # a sequence with no token gives zeros
