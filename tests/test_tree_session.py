"""Tree-shaped drafts on the CPU: append_tree / attend_tree / commit of
RaggedDecodeSession and PagedDecodeSession against the fp32 oracle on each
query's own ancestors (the needle inputs of tests/tree_cases.py and random
trees), single rank and under gloo at world size 2 with block 4."""

import os
import random

import pytest
import torch
import torch.multiprocessing as mp

import ragged_cases as rc
import tree_cases as tc

from tree_attention_torch_amd.ops.reference import flash_res_lse
from tree_attention_torch_amd.session import (PagedDecodeSession,
                                              RaggedDecodeSession, _n_local)

B, HKV, HQ, D = 3, 2, 4, 16
PARAMS = [pytest.param(c, id=tc.case_id(c)) for c in tc.CASES]
KINDS = ("ragged", "paged")


def _make(kind, block=4, max_tokens=256, batch=B, hkv=HKV, d=D, **kw):
    if kind == "paged":
        return PagedDecodeSession(batch, hkv, d, max_tokens=max_tokens,
                                  pool_tokens=kw.pop("pool_tokens", 2048),
                                  page=128, device="cpu", kv_dtype="fp32",
                                  block=block, **kw)
    return RaggedDecodeSession(batch, hkv, d, max_tokens=max_tokens,
                               device="cpu", kv_dtype="fp32", block=block,
                               **kw)


def _check_mirror(sess):
    assert sess.total_dev.tolist() == sess.totals
    assert sess.local_len_dev.tolist() == sess.local_lens
    assert sess.local_lens == [
        _n_local(t, sess.block, sess.rank, sess.world) for t in sess.totals]


# --------------------------------------------------------------------------
# the needle cases
# --------------------------------------------------------------------------
def _case_session(kind, tr):
    # capacity = (ceil(max_tokens / block) + 1) blocks = 1024
    sess = _make(kind, block=256, max_tokens=tc.CAP - 256, batch=tc.B,
                 hkv=tc.HKV, d=tc.D)
    assert sess.capacity == tc.CAP
    ks, vs, kd, vd = tc.stream(tr)
    for b, n in enumerate(tr.starts):
        if n:
            sess.prefill(b, ks[b, :, :n], vs[b, :, :n])
    return sess, kd, vd


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", PARAMS)
def test_tree_session_meets_the_oracle(case, kind):
    tr = tc.build(case, "bf16")
    sess, kd, vd = _case_session(kind, tr)
    parents = tc.parents_tensor(tr) if kind == "paged" else \
        [list(p) for p in tr.parents]
    sess.append_tree(kd, vd, parents, tr.counts)
    assert sess.totals == list(tr.lengths)
    _check_mirror(sess)
    base, mask = sess._tree_dev(tr.t)
    assert base.tolist() == tr.base.tolist()
    assert mask.tolist() == tr.bits.tolist()
    if kind == "ragged":
        rc.write_guards(sess.k, sess.v, tr.q, tr.lengths)
    out = sess.attend_tree(tr.q)
    tc.compare(tr, out, None, f"{kind} attend_tree")


@pytest.mark.parametrize("kind", KINDS)
def test_chain_tree_is_append_many_bit_for_bit(kind):
    tr = tc.build(tc.CASES[0], "bf16")
    assert tr.counts == (tr.t,) * tc.B
    tree, kd, vd = _case_session(kind, tr)
    many, _, _ = _case_session(kind, tr)
    tree.append_tree(kd, vd, tc.parents_tensor(tr))
    many.append_many(kd, vd)
    assert tree.totals == many.totals and tree.local_lens == many.local_lens
    for b, n in enumerate(tree.local_lens):
        for x, y in zip(tree._rows(b, n), many._rows(b, n)):
            assert torch.equal(x, y)
    assert torch.equal(tree.attend_tree(tr.q), many.attend_many(tr.q))


# --------------------------------------------------------------------------
# random trees: verify, commit a path, compare with the accepted stream
# --------------------------------------------------------------------------
def _anc(parents, i):
    out = []
    while i >= 0:
        out.append(i)
        i = parents[i]
    return out


def _oracle(q, k, v):
    """q (1, Hq, 1, D) over k / v (Hkv, n, D)."""
    return flash_res_lse(q, k[None], v[None])[0]


def _tree_step(sess, acc, t, counts, rng, gen, combine, as_tensor):
    """One append_tree + attend_tree + commit on random trees, each checked
    against the oracle over the accepted stream acc[b] = (k, v) (Hkv, n, D)
    plus the query's own ancestors; acc is advanced by the committed path."""
    parents = [[rng.randint(-1, j - 1) for j in range(t)] for _ in range(B)]
    k_new = torch.randn(B, HKV, t, D, generator=gen)
    v_new = torch.randn(B, HKV, t, D, generator=gen)
    before = list(sess.totals)
    assert before == [a[0].shape[1] for a in acc]
    sess.append_tree(
        k_new, v_new,
        torch.tensor(parents, dtype=torch.int32) if as_tensor else parents,
        counts)
    cl = [t] * B if counts is None else list(counts)
    assert sess.totals == [n + c for n, c in zip(before, cl)]
    _check_mirror(sess)
    q = torch.randn(B, HQ, t, D, generator=gen)
    out = sess.attend_tree(q, combine=combine)
    assert out.shape == (B, HQ, t, D)
    for b in range(B):
        for i in range(t):
            idx = sorted(_anc(parents[b], i)) if i < cl[b] else []
            k = torch.cat([acc[b][0], k_new[b][:, idx]], dim=1)
            v = torch.cat([acc[b][1], v_new[b][:, idx]], dim=1)
            if k.shape[1] == 0:
                assert not out[b, :, i].any(), (b, i)
                continue
            torch.testing.assert_close(
                out[b:b + 1, :, i:i + 1], _oracle(q[b:b + 1, :, i:i + 1], k, v),
                rtol=1e-5, atol=1e-5)
    # accept a random node's path (or nothing)
    paths, lens = [], []
    for b in range(B):
        leaf = rng.randint(-1, cl[b] - 1)
        path = _anc(parents[b], leaf)[::-1] if leaf >= 0 else []
        paths.append(path)
        lens.append(len(path))
        acc[b] = (torch.cat([acc[b][0], k_new[b][:, path]], dim=1),
                  torch.cat([acc[b][1], v_new[b][:, path]], dim=1))
    if as_tensor:
        paths = torch.tensor([p + [0] * (t - len(p)) for p in paths],
                             dtype=torch.int32)
    sess.commit(paths, lens)
    assert sess.totals == [n + m for n, m in zip(before, lens)]
    _check_mirror(sess)
    with pytest.raises(RuntimeError, match="attend_tree"):
        sess.attend_tree(q)          # the pending tree is gone
    q1 = torch.randn(B, HQ, 1, D, generator=gen)
    out = sess.attend(q1, combine=combine)
    for b in range(B):
        if acc[b][0].shape[1] == 0:
            assert not out[b].any()
            continue
        torch.testing.assert_close(out[b:b + 1], _oracle(q1[b:b + 1], *acc[b]),
                                   rtol=1e-5, atol=1e-5)


def _run_steps(sess, seed, combine="auto"):
    g = torch.Generator().manual_seed(seed)
    rng = random.Random(seed)      # the same draws on every rank
    gen = torch.Generator().manual_seed(seed + 1)
    acc = []
    for b, n in enumerate((0, 5, 127)):
        k, v = torch.randn(HKV, n, D, generator=g), \
            torch.randn(HKV, n, D, generator=g)
        if n:
            sess.prefill(b, k, v)
        acc.append((k, v))
    for step, t in enumerate((3, 4, 6, 16, 1, 4)):
        counts = None if step == 0 else [rng.randint(0, t) for _ in range(B)]
        _tree_step(sess, acc, t, counts, rng, gen, combine,
                   as_tensor=step % 2 == 1)
    return acc


@pytest.mark.parametrize("kind", KINDS)
def test_tree_session_single_rank_cpu(kind):
    sess = _make(kind)
    acc = _run_steps(sess, seed=0)
    # what is stored is, bit for bit, what a fresh session holds that was
    # fed only the accepted tokens
    fresh = _make(kind)
    for b, (k, v) in enumerate(acc):
        if k.shape[1]:
            fresh.prefill(b, k, v)
    assert sess.totals == fresh.totals and sess.local_lens == fresh.local_lens
    for b, n in enumerate(sess.local_lens):
        for x, y in zip(sess._rows(b, n), fresh._rows(b, n)):
            assert torch.equal(x, y)
    q = torch.randn(B, HQ, 1, D)
    assert torch.equal(sess.attend(q), fresh.attend(q))
    if kind == "paged":
        assert sess.free_pages == fresh.free_pages


def _worker(rank, world, port, kind):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # block 4: the nodes of one step cross owners several times
        sess = _make(kind, block=4)
        assert (sess.rank, sess.world) == (rank, world)
        _run_steps(sess, seed=3, combine="allgather")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,kind,port", [(2, "ragged", 29791),
                                             (2, "paged", 29793)])
def test_tree_session_sharded_gloo(world, kind, port):
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, world, port, kind))
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


def test_paged_commit_hands_pages_back():
    g = torch.Generator().manual_seed(7)
    sess = _make("paged", block=256, max_tokens=512)
    twin = _make("paged", block=256, max_tokens=512)
    k0 = torch.randn(HKV, 126, D, generator=g)
    for s in (sess, twin):
        s.prefill(0, k0, k0)
    free = sess.free_pages
    new = torch.randn(B, HKV, 6, D, generator=g)
    parents = [[-1, 0, 0, 1, 2, 2]] * B
    sess.append_tree(new, new, parents, [6, 0, 3])     # row 0: 126 -> 132
    assert len(sess._pages[0]) == 2 and sess.free_pages == free - 2
    sess.commit([[0, 2], [], [0, 1]], [2, 0, 1])       # row 0: 128, one page
    assert sess.totals == [128, 0, 1]
    assert len(sess._pages[0]) == 1 and sess.free_pages == free - 1
    twin.prefill(0, new[0][:, [0, 2]], new[0][:, [0, 2]])
    twin.prefill(2, new[2][:, [0]], new[2][:, [0]])
    assert sess.free_pages == twin.free_pages
    assert [len(p) for p in sess._pages] == [len(p) for p in twin._pages]
    for b, n in enumerate(sess.local_lens):
        for x, y in zip(sess._rows(b, n), twin._rows(b, n)):
            assert torch.equal(x, y)
    sess.append_tree(new, new, parents, [6, 6, 6])
    sess.commit([[]] * B, [0, 0, 0])                   # reject every draft
    assert sess.totals == [128, 0, 1] and sess.free_pages == twin.free_pages


# --------------------------------------------------------------------------
# errors
# --------------------------------------------------------------------------
def test_stale_tree():
    sess = _make("ragged")
    k3 = torch.zeros(B, HKV, 3, D)
    q3 = torch.zeros(B, HQ, 3, D)
    chain = [[-1, 0, 1]] * B
    with pytest.raises(RuntimeError, match="attend_tree"):
        sess.attend_tree(q3)                 # before any append_tree
    with pytest.raises(RuntimeError, match="commit"):
        sess.commit([[0]] * B, [1] * B)
    stale = (
        lambda: sess.append_many(k3, k3, [1, 0, 0]),
        lambda: sess.append(k3[:, :, :1], k3[:, :, :1]),
        lambda: sess.prefill(1, k3[0], k3[0]),
        lambda: sess.reset(0),
        lambda: sess.truncate(2, 1),
    )
    for move in stale:
        sess.append_tree(k3, k3, chain)
        sess.attend_tree(q3)
        with pytest.raises(RuntimeError, match="attend_many"):
            sess.attend_many(q3)             # append_tree cleared the chain
        move()
        with pytest.raises(RuntimeError, match="attend_tree"):
            sess.attend_tree(q3)
        with pytest.raises(RuntimeError, match="commit"):
            sess.commit([[0]] * B, [1] * B)
    sess.append_tree(k3, k3, chain)
    with pytest.raises(ValueError, match="T = 3"):
        sess.attend_tree(torch.zeros(B, HQ, 4, D))


def test_tree_is_stale_when_the_lengths_come_back_to_the_same_totals():
    """truncate + append_many that land on the totals the tree left: the
    cache rows under the tree's masks are new, so the tree is gone."""
    sess = _make("ragged")
    k3 = torch.zeros(B, HKV, 3, D)
    sess.append_tree(k3, k3, [[-1, 0, 0]] * B)
    for b in range(B):
        sess.truncate(b, 0)
    sess.append_many(k3 + 1, k3 + 1)
    assert sess.totals == [3] * B
    with pytest.raises(RuntimeError, match="attend_tree"):
        sess.attend_tree(torch.zeros(B, HQ, 3, D))
    with pytest.raises(RuntimeError, match="commit"):
        sess.commit([[0]] * B, [1] * B)


def test_bad_parents_name_the_row():
    sess = _make("ragged")
    k3 = torch.zeros(B, HKV, 3, D)
    with pytest.raises(ValueError, match=r"parents\[1\]\[2\] = 2 .*row 1"):
        sess.append_tree(k3, k3, [[-1, 0, 1], [-1, 0, 2], [-1, 0, 1]])
    with pytest.raises(ValueError, match=r"parents\[2\]\[0\] = -2 .*row 2"):
        sess.append_tree(k3, k3, [[-1, 0, 1], [-1, 0, 1], [-2, 0, 1]])
    with pytest.raises(ValueError, match=r"parents\[0\] has 2 entries"):
        sess.append_tree(k3, k3, [[-1, 0], [-1, 0, 1], [-1, 0, 1]])
    with pytest.raises(ValueError, match="parents has 2 rows"):
        sess.append_tree(k3, k3, [[-1, 0, 1]] * 2)
    with pytest.raises(ValueError, match="parents must be a"):
        sess.append_tree(k3, k3, torch.zeros(B, 3, dtype=torch.long))
    with pytest.raises(ValueError, match="parents must be a"):
        sess.append_tree(k3, k3, torch.zeros(B, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="append_tree"):
        sess.append_tree(torch.zeros(B, HKV, 17, D), torch.zeros(B, HKV, 17, D),
                         [[-1] * 17] * B)
    with pytest.raises(ValueError, match=r"counts\[1\] = 4"):
        sess.append_tree(k3, k3, [[-1, 0, 1]] * B, [3, 4, 0])
    assert sess.totals == [0, 0, 0] and sess._tree is None
    # a short row is fine where the count does not reach past it
    sess.append_tree(k3, k3, [[-1, 0], [-1, 0, 1], []], [2, 3, 0])
    assert sess.totals == [2, 3, 0]


def test_bad_paths_name_the_row():
    sess = _make("ragged")
    k4 = torch.zeros(B, HKV, 4, D)
    parents = [[-1, 0, 0, 2]] * B

    def fresh():
        for b in range(B):
            sess.reset(b)
        sess.append_tree(k4, k4, parents, [4, 4, 2])

    fresh()
    with pytest.raises(ValueError, match=r"paths\[1\]\[1\] = 3 .*row 1"):
        sess.commit([[0, 2, 3], [0, 3], [0]], [3, 2, 1])   # 3 hangs off 2
    with pytest.raises(ValueError, match=r"paths\[0\]\[0\] = 2 .*row 0"):
        sess.commit([[2, 3], [0], [0]], [2, 1, 1])         # no root
    with pytest.raises(ValueError, match=r"paths\[2\]\[1\] = 2 .*row 2"):
        sess.commit([[0], [0], [0, 2]], [1, 1, 2])         # past the count
    with pytest.raises(ValueError, match=r"lens\[2\] = 3 .*row 2"):
        sess.commit([[0], [0], [0, 1, 1]], [1, 1, 3])
    with pytest.raises(ValueError, match=r"lens\[0\] = -1"):
        sess.commit([[0], [0], [0]], [-1, 1, 1])
    with pytest.raises(ValueError, match=r"paths\[1\] has 1 entries"):
        sess.commit([[0], [0], [0]], [1, 2, 1])
    with pytest.raises(ValueError, match="lens has 2"):
        sess.commit([[0], [0], [0]], [1, 1])
    with pytest.raises(ValueError, match="paths must be a"):
        sess.commit(torch.zeros(B, 4, dtype=torch.long), [1, 1, 1])
    assert sess.totals == [4, 4, 2] and sess._tree is not None
    sess.commit([[0, 2, 3], [0, 1], []], [3, 2, 0])
    assert sess.totals == [3, 2, 0]
    _check_mirror(sess)


def _state(sess):
    st = [list(sess.totals), list(sess.local_lens), sess.total_dev.clone(),
          sess.local_len_dev.clone(), sess._tree]
    if isinstance(sess, PagedDecodeSession):
        st += [list(sess._free), [list(p) for p in sess._pages],
               sess.k_pool.clone(), sess.page_table.clone()]
    else:
        st += [sess.k.clone(), sess.v.clone()]
    return st


def _same_state(a, b):
    return all(torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y
               for x, y in zip(a, b))


def test_capacity_error_names_the_row_before_any_state_moves():
    sess = RaggedDecodeSession(2, 2, 16, max_tokens=8, device="cpu",
                               kv_dtype="fp32", block=4)
    assert sess.capacity == 12
    sess.k.zero_(), sess.v.zero_()
    one = torch.ones(2, 2, 4, 16)
    star = [[-1] * 4] * 2
    sess.append_tree(one, one, star, [4, 4])
    sess.commit([[0], [1]], [1, 1])
    sess.prefill(1, one[0, :, :1].expand(2, 9, 16), one[0, :, :1].expand(2, 9, 16))
    assert sess.totals == [1, 10]
    before = _state(sess)
    with pytest.raises(RuntimeError, match=r"capacity exceeded: row 1 "):
        sess.append_tree(2 * one, 2 * one, star, [4, 3])
    assert _same_state(before, _state(sess))
    sess.append_tree(one, one, star, [4, 2])
    assert sess.totals == [5, 12]


def test_pool_exhausted_names_the_row_before_any_state_moves():
    sess = PagedDecodeSession(2, 2, 16, max_tokens=512, pool_tokens=256,
                              page=128, device="cpu", kv_dtype="fp32",
                              block=256)
    sess.k_pool.zero_(), sess.v_pool.zero_()
    row = torch.ones(2, 127, 16)
    sess.prefill(0, row, row)
    sess.prefill(1, row, row)
    assert sess.free_pages == 0
    one = torch.ones(2, 2, 4, 16)
    before = _state(sess)
    with pytest.raises(RuntimeError, match=r"pool exhausted: row 0 "):
        sess.append_tree(one, one, [[-1, 0, 0, 0]] * 2, [2, 1])
    assert _same_state(before, _state(sess))
