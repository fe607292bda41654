"""Tree-shaped drafts on the GPU: the tree append and commit kernels against
a host model, the ancestor-mask decode kernels on the needle inputs of
tests/tree_cases.py (what they can see is proven on the CPU in
tests/test_tree_sensitivity.py), and the sessions end to end: eager, graphed,
the generic fallback, slab and paged."""

from functools import lru_cache

import pytest
import torch

import needle_cases as nc
import paged_cases as pc
import ragged_cases as rc
import tree_cases as tc

pytestmark = pytest.mark.gpu

NGPU = torch.cuda.device_count() if torch.cuda.is_available() else 0
_PORT = 29690
PAGE = 128
SCALE = 1.0 / tc.D ** 0.5
PARAMS = [pytest.param(c, id=tc.case_id(c)) for c in tc.CASES]
LAYOUTS = ("slab", "paged")


@pytest.fixture(scope="module")
def ext():
    from tree_attention_torch_amd.ops import flash

    assert flash.hip_available(), "HIP extension must be built in-tree"
    return flash._load_extension()


def _len_dev(lengths):
    return torch.tensor(list(lengths), dtype=torch.long, device="cuda")


def _i32(x):
    return torch.as_tensor(x).to(device="cuda", dtype=torch.int32).contiguous()


# --------------------------------------------------------------------------
# kv_*_append_tree / kv_*_commit_path against a host model
# --------------------------------------------------------------------------
def _place(t, block, world):
    return (t // block) % world, block * ((t // block) // world) + t % block


def _n_local(t, block, rank, world):
    return sum(1 for x in range(t) if (x // block) % world == rank)


def _walk_mask(t0, c, parents, i, cap, block, rank, world):
    """The clamped walk of kv_append_tree_kernel from node i: the local slots
    of the nodes this rank owns and stored."""
    if i >= c:
        return 0
    m, n, base = 0, i, _n_local(t0, block, rank, world)
    while n >= 0:
        owner, pos = _place(t0 + n, block, world)
        if owner == rank and pos < cap:
            m |= 1 << (_n_local(t0 + n + 1, block, rank, world) - 1 - base)
        n = min(max(parents[n], -1), n - 1)
    return m


class _Store:
    """Sentinel-filled storage, slab or paged, with its host image."""

    def __init__(self, layout, dtype):
        self.layout, self.td = layout, rc._TD[dtype]
        bsz, hkv, d = 4, 2, 128
        esz = torch.empty(0, dtype=self.td).element_size()
        if layout == "slab":
            self.cap, self.start = 64, [0, 3, 30, 62]
            shape = (bsz, hkv, self.cap, d * esz)
        else:
            self.cap, self.start = 2 * PAGE, [0, 3, 130, 250]
            shape = (10, hkv, PAGE, d * esz)   # pages 8 and 9 belong to no row
            self.table_h = torch.tensor([[3, 6], [0, 5], [1, 7], [2, 4]],
                                        dtype=torch.int32)
            self.table = self.table_h.cuda()
        self.kc = torch.full(shape, 0xA5, dtype=torch.uint8,
                             device="cuda").view(self.td)
        self.vc = torch.full(shape, 0x5A, dtype=torch.uint8,
                             device="cuda").view(self.td)
        self.want_k, self.want_v = self.kc.cpu().clone(), self.vc.cpu().clone()

    def args(self):
        if self.layout == "slab":
            return (self.kc, self.vc)
        return (self.kc, self.vc, self.table)

    def put(self, b, pos, k_row, v_row):
        """The host image of a store at local position pos of row b; False
        past the capacity (nothing is stored there)."""
        if pos >= self.cap:
            return False
        if self.layout == "slab":
            self.want_k[b, :, pos], self.want_v[b, :, pos] = k_row, v_row
        else:
            pid = int(self.table_h[b, pos // PAGE])
            self.want_k[pid, :, pos % PAGE] = k_row
            self.want_v[pid, :, pos % PAGE] = v_row
        return True

    def check(self):
        assert torch.equal(self.kc.cpu().view(torch.uint8),
                           self.want_k.view(torch.uint8))
        assert torch.equal(self.vc.cpu().view(torch.uint8),
                           self.want_v.view(torch.uint8))


@pytest.mark.parametrize("commit", [False, True], ids=["append", "commit"])
@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("rank,world,block", [(1, 3, 4), (0, 1, 64)])
def test_kv_append_tree_and_commit(ext, dtype, layout, rank, world, block,
                                   commit):
    """12 steps of T in {4, 3, 16, 1} with changing counts (0 included) and
    random valid parents into sentinel-filled storage: the stored rows are
    bit equal to what the host formula places, base / mask / local_len /
    total equal the host model after every step, and every other byte still
    holds the sentinel. With `commit` every step is followed by a commit of
    random source rows (out-of-range entries and lengths are clamped). At
    (0, 1, 64) rows run past the slab's capacity, or the page table, and
    store nothing there."""
    import random

    bsz, hkv, d = 4, 2, 128
    st = _Store(layout, dtype)
    g = torch.Generator().manual_seed(rc.SEED + block)
    rng = random.Random(rc.SEED + block)
    append = ext.kv_cache_append_tree if layout == "slab" else \
        ext.kv_pool_append_tree
    commit_path = ext.kv_cache_commit_path if layout == "slab" else \
        ext.kv_pool_commit_path
    total = torch.tensor(st.start, dtype=torch.long, device="cuda")
    # local_len starts at values a count of 0 must leave alone
    llen = torch.tensor([5, 6, 7, 8], dtype=torch.long, device="cuda")
    h_total, h_llen = list(st.start), [5, 6, 7, 8]
    overran = False
    for step in range(12):
        t = (4, 3, 16, 1)[step % 4]
        counts = [(step * 7 + b * 3) % (t + 1) for b in range(bsz)]
        counts[step % bsz] = 0 if step % 3 == 0 else counts[step % bsz]
        parents = [[rng.randint(-1, j - 1) for j in range(t)]
                   for _ in range(bsz)]
        k_new = torch.randn(bsz, hkv, t, d, generator=g).to(st.td)
        v_new = torch.randn(bsz, hkv, t, d, generator=g).to(st.td)
        k_dev, v_dev = k_new.cuda(), v_new.cuda()
        base = torch.full((bsz,), -7, dtype=torch.long, device="cuda")
        mask = torch.full((bsz, t), -7, dtype=torch.int32, device="cuda")
        cnt = _i32(counts)
        append(*st.args(), k_dev, v_dev, total, llen, cnt, _i32(parents),
               base, mask, block, rank, world)
        h_base, h_mask = [], []
        for b, c in enumerate(counts):
            t0 = h_total[b]
            for i in range(c):
                owner, pos = _place(t0 + i, block, world)
                if owner == rank and not st.put(b, pos, k_new[b, :, i],
                                                v_new[b, :, i]):
                    overran = True
            h_base.append(_n_local(t0, block, rank, world))
            h_mask.append([_walk_mask(t0, c, parents[b], i, st.cap, block,
                                      rank, world) for i in range(t)])
            if c:
                h_llen[b] = _n_local(t0 + c, block, rank, world)
            h_total[b] = t0 + c
        assert base.tolist() == h_base and mask.tolist() == h_mask, \
            f"step {step}"
        assert total.tolist() == h_total and llen.tolist() == h_llen, \
            f"step {step}"
        if not commit:
            continue
        path = [[rng.randint(-2, t + 1) for _ in range(t)]
                for _ in range(bsz)]
        plen = [rng.randint(-1, t + 1) for _ in range(bsz)]
        commit_path(*st.args(), k_dev, v_dev, total, llen, cnt, _i32(path),
                    _i32(plen), block, rank, world)
        for b, c in enumerate(counts):
            t0 = h_total[b] - c
            n = min(max(plen[b], 0), c)
            for i in range(n):
                src = min(max(path[b][i], 0), t - 1)
                owner, pos = _place(t0 + i, block, world)
                if owner == rank:
                    st.put(b, pos, k_new[b, :, src], v_new[b, :, src])
            if c:
                h_llen[b] = _n_local(t0 + n, block, rank, world)
            h_total[b] = t0 + n
        assert total.tolist() == h_total and llen.tolist() == h_llen, \
            f"commit after step {step}"
    assert commit or overran or world > 1     # (0, 1, 64) overruns rows
    st.check()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_malformed_parents_terminate(ext, layout):
    """Entries >= j and < -1 are clamped into [-1, j - 1]: the walk ends and
    yields the clamped walk's mask."""
    st = _Store(layout, "bf16")
    t, bsz = 16, 4
    parents = [[5] * t, [-9] * t, list(range(t)), [j + 3 for j in range(t)]]
    counts = [16, 16, 7, 16]
    total = torch.tensor(st.start, dtype=torch.long, device="cuda")
    llen = torch.zeros(bsz, dtype=torch.long, device="cuda")
    new = torch.zeros(bsz, 2, t, 128, dtype=st.td, device="cuda")
    base = torch.full((bsz,), -7, dtype=torch.long, device="cuda")
    mask = torch.full((bsz, t), -7, dtype=torch.int32, device="cuda")
    append = ext.kv_cache_append_tree if layout == "slab" else \
        ext.kv_pool_append_tree
    append(*st.args(), new, new, total, llen, _i32(counts), _i32(parents),
           base, mask, 64, 0, 1)
    want = [[_walk_mask(st.start[b], counts[b], parents[b], i, st.cap, 64, 0,
                        1) for i in range(t)] for b in range(bsz)]
    assert mask.tolist() == want
    assert base.tolist() == st.start
    # row 1 is a star, row 0 hangs every node past 5 off node 5
    assert want[1][:4] == [1, 2, 4, 8]
    assert want[0][9] == (1 << 9) | 0b111111


def test_append_tree_and_commit_checks(ext):
    kc = torch.zeros(2, 2, 8, 128, dtype=torch.bfloat16, device="cuda")
    new = torch.zeros(2, 2, 3, 128, dtype=torch.bfloat16, device="cuda")
    lens = torch.zeros(2, dtype=torch.long, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
    par = torch.full((2, 3), -1, dtype=torch.int32, device="cuda")
    base = torch.zeros(2, dtype=torch.long, device="cuda")
    mask = torch.zeros(2, 3, dtype=torch.int32, device="cuda")

    def call(new=new, cnt=cnt, par=par, base=base, mask=mask, rank=0,
             world=1):
        ext.kv_cache_append_tree(kc, kc.clone(), new, new, lens, lens.clone(),
                                 cnt, par, base, mask, 4, rank, world)

    call()
    with pytest.raises(RuntimeError, match="rank"):
        call(rank=1)
    big = torch.zeros(2, 2, 17, 128, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError, match="T must be in 1..16"):
        call(new=big)
    with pytest.raises(RuntimeError, match="counts"):
        call(cnt=cnt.long())
    with pytest.raises(RuntimeError, match="parents"):
        call(par=par.long())
    with pytest.raises(RuntimeError, match="parents"):
        call(par=par[:, :2].contiguous())
    with pytest.raises(RuntimeError, match="base"):
        call(base=base.int())
    with pytest.raises(RuntimeError, match="mask"):
        call(mask=mask.long())
    with pytest.raises(RuntimeError, match="mask"):
        call(mask=mask.cpu())
    with pytest.raises(RuntimeError, match="dtype"):
        call(new=new.half())

    def commit(new=new, cnt=cnt, path=par, plen=cnt):
        ext.kv_cache_commit_path(kc, kc.clone(), new, new, lens, lens.clone(),
                                 cnt, path, plen, 4, 0, 1)

    commit()
    with pytest.raises(RuntimeError, match="T must be in 1..16"):
        commit(new=big)
    with pytest.raises(RuntimeError, match="counts"):
        commit(cnt=cnt.long())
    with pytest.raises(RuntimeError, match="path must"):
        commit(path=par.long())
    with pytest.raises(RuntimeError, match="path_len"):
        commit(plen=cnt[:1].contiguous())
    with pytest.raises(RuntimeError, match="dtype"):
        commit(new=new.half())


# --------------------------------------------------------------------------
# flash_attention_cache_tree / flash_attention_paged_tree over hand-built
# base / mask
# --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("case", PARAMS)
def test_tree_kernels(ext, case, dtype):
    """Slab and paged meet the oracle at the suite's bars, and are bit
    equal to each other: same arithmetic, only the addresses differ. On the
    chain every row is bit equal to the visible-length kernel."""
    nc.assert_default_split_plan()
    tr = tc.build(case, dtype)
    q, base, mask = tr.q.cuda(), tr.base.cuda(), _i32(tr.bits)
    kc, vc = tr.k_cache.cuda(), tr.v_cache.cuda()
    out, lse = ext.flash_attention_cache_tree(q, kc, vc, _len_dev(tr.lengths),
                                              base, mask, SCALE)
    tc.compare(tr, out, lse, "flash_attention_cache_tree")
    pl = pc.scatter(tr, PAGE)
    out_p, lse_p = ext.flash_attention_paged_tree(
        q, pl.k_pool.cuda(), pl.v_pool.cuda(), pl.table.cuda(),
        _len_dev(tr.lengths), base, mask, SCALE)
    tc.compare(tr, out_p, lse_p, "flash_attention_paged_tree")
    assert torch.equal(out, out_p) and torch.equal(lse, lse_p)
    if tc.case_id(case) == "chain":
        assert tr.counts == (tr.t,) * tc.B
        vis = (tr.base[:, None] + torch.arange(1, tr.t + 1)[None, :]).cuda()
        out_q, lse_q = ext.flash_attention_cache_qlen(
            q, kc, vc, _len_dev(tr.lengths), vis.contiguous(), SCALE)
        assert torch.equal(out, out_q) and torch.equal(lse, lse_q)


def test_tree_kernel_checks(ext):
    tr = tc.build(tc.CASES[0], "bf16")
    q, k, v = tr.q.cuda(), tr.k.cuda(), tr.v.cuda()
    lens, base, mask = _len_dev(tr.lengths), tr.base.cuda(), _i32(tr.bits)

    def call(q=q, lens=lens, base=base, mask=mask):
        return ext.flash_attention_cache_tree(q, k, v, lens, base, mask,
                                              SCALE)

    call()
    with pytest.raises(RuntimeError, match="mask"):
        call(mask=mask[:, :2].contiguous())
    with pytest.raises(RuntimeError, match="mask"):
        call(mask=mask.long())
    with pytest.raises(RuntimeError, match="mask"):
        call(mask=mask.t().contiguous().t())
    with pytest.raises(RuntimeError, match="base"):
        call(base=base.int())
    with pytest.raises(RuntimeError, match="base"):
        call(base=base[:2].contiguous())
    with pytest.raises(RuntimeError, match="len_dev"):
        call(lens=lens[:1])
    with pytest.raises(RuntimeError, match="T must be in 1..16"):
        call(q=torch.zeros(tc.B, tc.HQ, 17, tc.D, dtype=torch.bfloat16,
                           device="cuda"),
             mask=torch.zeros(tc.B, 17, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="GQA group size"):
        call(q=torch.zeros(tc.B, 34, 4, tc.D, dtype=torch.bfloat16,
                           device="cuda"))
    pl = pc.scatter(tr, PAGE)
    with pytest.raises(RuntimeError, match="mask"):
        ext.flash_attention_paged_tree(
            q, pl.k_pool.cuda(), pl.v_pool.cuda(), pl.table.cuda(), lens,
            base, mask.long(), SCALE)


# --------------------------------------------------------------------------
# sessions
# --------------------------------------------------------------------------
def _session(layout, dtype, **kw):
    from tree_attention_torch_amd.session import (PagedDecodeSession,
                                                  RaggedDecodeSession)

    # capacity = (ceil(max_tokens / block) + 1) blocks = 1024
    if layout == "slab":
        sess = RaggedDecodeSession(tc.B, tc.HKV, tc.D, max_tokens=tc.CAP - 256,
                                   device="cuda", kv_dtype=dtype, block=256,
                                   **kw)
    else:
        sess = PagedDecodeSession(tc.B, tc.HKV, tc.D, max_tokens=tc.CAP - 256,
                                  pool_tokens=16 * PAGE, page=PAGE,
                                  device="cuda", kv_dtype=dtype, block=256,
                                  **kw)
    assert sess.capacity == tc.CAP
    return sess


def _prefill(sess, tr):
    ks, vs, kd, vd = (t.cuda() for t in tc.stream(tr))
    for b, n in enumerate(tr.starts):
        if n > sess.totals[b]:
            sess.prefill(b, ks[b, :, sess.totals[b]:n],
                         vs[b, :, sess.totals[b]:n])
    assert sess.totals == list(tr.starts)
    return kd, vd


def _guard(sess, tr, lengths):
    """The guard pattern at and past lengths[b], in place (a captured step
    holds the storage's address). Paged: also decoy K / NaN V on every free
    page, and every table entry past a row's live pages names a free page
    (tests/test_gpu_spec.py)."""
    if not hasattr(sess, "k_pool"):
        rc.write_guards(sess.k, sess.v, tr.q, lengths)
        return
    td = sess.k_pool.dtype
    gk, gv = rc.guard_fill(tr.q.cpu(), tr.cap)
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
        sess.k_pool[pid] = gk[pid % tc.B, :, :PAGE].to(device="cuda", dtype=td)
        sess.v_pool[pid] = float("nan")


def _check_tree_state(sess, tr):
    assert sess.totals == list(tr.lengths)
    assert sess.total_dev.tolist() == list(tr.lengths)
    assert sess.local_len_dev.tolist() == list(tr.lengths)
    base, mask = sess._tree_dev(tr.t)
    assert base.tolist() == tr.base.tolist()
    assert mask.tolist() == tr.bits.tolist()


@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", PARAMS)
def test_tree_session_eager(ext, case, layout, dtype):
    tr = tc.build(case, dtype)
    sess = _session(layout, dtype)
    kd, vd = _prefill(sess, tr)
    _guard(sess, tr, tr.starts)     # the nodes land on the first guard rows
    parents = tc.parents_tensor(tr, "cuda") if layout == "slab" else \
        [list(p) for p in tr.parents]
    sess.append_tree(kd, vd, parents, tr.counts)
    _check_tree_state(sess, tr)
    _guard(sess, tr, tr.lengths)
    out = sess.attend_tree(tr.q.cuda())
    tc.compare(tr, out, None, f"{layout} attend_tree")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_tree_session_generic_path(ext, layout):
    """An fp32 cache does not take the zero-copy kernels: the per-row,
    per-query gather over local_attention meets the same oracle, and
    graphed_step_tree refuses the session."""
    tr = tc.build(tc.CASES[2], "bf16")
    sess = _session(layout, "fp32")
    kd, vd = _prefill(sess, tr)
    sess.append_tree(kd, vd, tc.parents_tensor(tr, "cuda"), tr.counts)
    _check_tree_state(sess, tr)
    _guard(sess, tr, tr.lengths)
    out = sess.attend_tree(tr.q.cuda())
    tc.compare(tr, out, None, f"{layout} fp32 fallback")
    with pytest.raises(ValueError, match="does not take this session"):
        sess.graphed_step_tree(tr.q.cuda(), kd, vd,
                               tc.parents_tensor(tr, "cuda"))


# three replays per T: (counts, parents per row, the path committed after
# the replay). Starts follow from the commits: row 0 crosses the split seam,
# row 2 drops back onto its first page (131 -> 128), paths that are no prefix
# of the nodes ([0, 2]) move a node's K/V to another position.
_T4 = ((-1, 0, 0, 2), tc.STAR4, tc.CHAIN4, (-1, -1, 0, 1))
_C6 = (-1, 0, 1, 2, 3, 4)
_B6 = (-1, -1, 0, 1, 2, 3)
GRAPH_START = (510, 62, 126, 0)
GRAPH_STEPS = {
    4: (((4, 2, 0, 3), (_T4[0],) * 4, ([0, 2], [0, 1], [], [0])),
        ((1, 4, 4, 0), (_T4[1], _T4[2], _T4[0], _T4[1]),
         ([0], [0, 1, 2, 3], [0, 2], [])),
        ((4, 4, 4, 4), (_T4[3], _T4[0], _T4[3], _T4[2]),
         ([1, 3], [0, 2, 3], [], [0, 1, 2, 3]))),
    6: (((6, 2, 0, 3), (tc.TWO6,) * 4, ([0, 2], [0, 1], [], [0])),
        ((1, 6, 5, 0), (tc.TWO6, _C6, tc.TWO6, _B6),
         ([0], [0, 1, 2, 3, 4, 5], [0, 2], [])),
        ((6, 6, 6, 6), (tc.TWO6, _B6, _C6, tc.TWO6),
         ([0, 2, 5], [1, 3, 5], [], [0, 1, 3]))),
}


@lru_cache(maxsize=None)
def _graph_steps(t, dtype):
    """The three Tree inputs of GRAPH_STEPS[t], each over the streams the
    commit before it leaves."""
    (k, v), starts, steps = rc.kv(dtype), GRAPH_START, []
    for counts, parents, paths in GRAPH_STEPS[t]:
        tr = tc.build_from((t, starts, counts, parents), dtype, k, v)
        steps.append(tr)
        k, v, starts = tc.committed(tr, paths, [len(p) for p in paths])
    return steps, (k, v, starts)


@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("t", [4, 6])
def test_graphed_step_tree(ext, t, layout, dtype):
    """One captured tree step (T = 6: two attention launches) replayed three
    times with another tree and other counts each time and a commit between
    replays: every replay meets the oracle and is bit-equal to an eager twin
    session fed the same stream; after the last commit both hold, bit for
    bit, the accepted tokens."""
    steps, (k_end, v_end, ends) = _graph_steps(t, dtype)
    sess, twin = _session(layout, dtype), _session(layout, dtype)
    for s in (sess, twin):
        _prefill(s, steps[0])
    q_static = torch.zeros_like(steps[0].q, device="cuda")
    k_static = torch.zeros(tc.B, tc.HKV, t, tc.D, dtype=torch.bfloat16,
                           device="cuda")
    v_static = torch.zeros_like(k_static)
    p_static = torch.full((tc.B, t), -1, dtype=torch.int32, device="cuda")
    replay = sess.graphed_step_tree(q_static, k_static, v_static, p_static)
    # neither the warm-up nor the capture moved a length
    assert sess.totals == list(steps[0].starts)
    assert sess.total_dev.tolist() == list(steps[0].starts)
    assert sess.local_len_dev.tolist() == list(steps[0].starts)
    for tr, (_, _, paths) in zip(steps, GRAPH_STEPS[t]):
        for s in (sess, twin):
            assert s.totals == list(tr.starts)
            assert s.local_len_dev.tolist() == list(tr.starts)
            _guard(s, tr, tr.starts)
        _, _, kd, vd = (x.cuda() for x in tc.stream(tr))
        q_static.copy_(tr.q)
        k_static.copy_(kd)
        v_static.copy_(vd)
        p_static.copy_(tc.parents_tensor(tr))
        out = replay(list(tr.counts))
        _check_tree_state(sess, tr)
        tc.compare(tr, out, None, "graphed_step_tree replay")
        twin.append_tree(kd, vd, [list(p) for p in tr.parents], tr.counts)
        eager = twin.attend_tree(tr.q.cuda())
        assert torch.equal(out, eager), f"replay != eager twin at {tr.starts}"
        lens = [len(p) for p in paths]
        padded = [list(p) + [0] * (t - len(p)) for p in paths]
        sess.commit(_i32(padded), lens)       # the sampler's device tensor
        twin.commit([list(p) for p in paths], lens)
    for s in (sess, twin):
        assert s.totals == list(ends)
        assert s.total_dev.tolist() == list(ends)
        assert s.local_len_dev.tolist() == list(ends)
    td = rc._TD[dtype]
    for b, n in enumerate(ends):
        if n == 0:
            continue
        want = (k_end[b:b + 1, :, :n].to(td), v_end[b:b + 1, :, :n].to(td))
        for got_s, got_t, w in zip(sess._rows(b, n), twin._rows(b, n), want):
            assert torch.equal(got_s.cpu().view(torch.uint8),
                               w.contiguous().view(torch.uint8)), b
            assert torch.equal(got_t.cpu().view(torch.uint8),
                               w.contiguous().view(torch.uint8)), b
    if layout == "paged":
        assert [len(p) for p in sess._pages] == \
            [pc.pages_of(n, PAGE) for n in ends]
        assert sess.free_pages == twin.free_pages


def test_graphed_step_tree_capacity(ext):
    """replay() checks the host mirror before anything is launched."""
    from tree_attention_torch_amd.session import RaggedDecodeSession

    sess = RaggedDecodeSession(2, 2, 128, max_tokens=64, device="cuda",
                               kv_dtype="bf16", block=64)
    new = torch.ones(2, 2, 3, 128, dtype=torch.bfloat16, device="cuda")
    q = torch.ones(2, 8, 3, 128, dtype=torch.bfloat16, device="cuda")
    par = _i32([[-1, 0, 0]] * 2)
    sess.prefill(1, new[0, :, :1].expand(2, 126, 128),
                 new[0, :, :1].expand(2, 126, 128))
    replay = sess.graphed_step_tree(q, new, new, par)
    with pytest.raises(RuntimeError, match="row 1 "):
        replay()
    assert sess.totals == [0, 126] and sess.total_dev.tolist() == [0, 126]
    out = replay([3, 2])
    assert sess.total_dev.tolist() == [3, 128]
    assert sess.local_len_dev.tolist() == [3, 128]
    assert torch.isfinite(out).all()
    sess.commit([[0, 2], [0]], [2, 1])
    assert sess.total_dev.tolist() == [2, 127]
    assert sess.local_len_dev.tolist() == [2, 127]


# --------------------------------------------------------------------------
# multi-rank (RCCL): auto-skips below 2 GPUs
# --------------------------------------------------------------------------
def _tree_rccl_worker(rank, world, port):
    import os

    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import tree_cases as tcw
    from tree_attention_torch_amd.parallel.pg import cleanup, setup
    from tree_attention_torch_amd.session import RaggedDecodeSession

    device = torch.device(f"cuda:{rank}")
    setup(rank, world)
    try:
        tr = tcw.build(tcw.CASES[2], "bf16")
        # block 64: the nodes at 62 and at 510 cross owners
        sess = RaggedDecodeSession(tcw.B, tcw.HKV, tcw.D, max_tokens=2048,
                                   device=device, kv_dtype="bf16", block=64)
        ks, vs, kd, vd = (t.to(device) for t in tcw.stream(tr))
        for b, n in enumerate(tr.starts):
            if n:
                sess.prefill(b, ks[b, :, :n], vs[b, :, :n])
        sess.append_tree(kd, vd, tcw.parents_tensor(tr, device), tr.counts)
        assert sess.local_len_dev.tolist() == sess.local_lens
        bases, masks = sess._tree_host(sess._tree)
        base_dev, mask_dev = sess._tree_dev(tr.t)
        assert base_dev.tolist() == bases and mask_dev.tolist() == masks
        for combine in ("allgather", "allreduce"):
            out = sess.attend_tree(tr.q.to(device), combine=combine)
            torch.cuda.synchronize()
            tcw.compare(tr, out, None, f"rank {rank} {combine}")
    finally:
        cleanup()


@pytest.mark.skipif(NGPU < 2, reason=f"needs >=2 GPUs, have {NGPU}")
def test_rccl_tree_session():
    import torch.multiprocessing as mp

    mp.spawn(_tree_rccl_worker, args=(NGPU, _PORT), nprocs=NGPU, join=True)
