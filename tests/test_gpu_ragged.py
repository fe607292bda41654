"""Ragged batched decode on the GPU: per-row lengths in the zero-copy cache
kernel, the device-side append kernel, RaggedDecodeSession and its captured
step, on the needle inputs of tests/ragged_cases.py (what they can see is
proven on the CPU in tests/test_ragged_sensitivity.py)."""

import pytest
import torch

import ragged_cases as rc

pytestmark = pytest.mark.gpu

NGPU = torch.cuda.device_count() if torch.cuda.is_available() else 0
_PORT = 29640


@pytest.fixture(scope="module")
def ext():
    from tree_attention_torch_amd.ops import flash

    assert flash.hip_available(), "HIP extension must be built in-tree"
    return flash._load_extension()


# capacity 1024, then 4608 with its seam and its pair family
SETS = [pytest.param(n, "seam", id=str(n))
        for n in rc.LENGTH_SETS + rc.LENGTH_SETS_BIG] + \
    [pytest.param(n, "pair", id=f"{n}-pair") for n in rc.LENGTH_SETS_BIG]


def _len_dev(lengths):
    return torch.tensor(list(lengths), dtype=torch.long, device="cuda")


# --------------------------------------------------------------------------
# flash_attention_cache with one length per batch row
# --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("lengths,family", SETS)
def test_cache_kernel_per_row_lengths(ext, lengths, family, dtype):
    """Capacity 1024 (two splits) and 4608 (nine: rows of 4097, 0, 513 and
    2560 keys leave none, all, seven and four trailing splits empty)."""
    import needle_cases as nc

    nc.assert_default_split_plan()
    rg = rc.build(lengths, dtype, family)
    assert rg.k_cache.shape[2] == rc.cap_of(lengths)
    out, lse = ext.flash_attention_cache(
        rg.q.cuda(), rg.k_cache.cuda(), rg.v_cache.cuda(), _len_dev(lengths),
        1.0 / rc.D ** 0.5)
    assert out.shape == (rc.B, rc.HQ, 1, rc.D)
    rc.compare(rg, out, lse, "flash_attention_cache, (B,) lengths")


@pytest.mark.parametrize("dtype", rc.DTYPES)
def test_cache_kernel_one_length_for_the_batch(ext, dtype):
    """A one-element length tensor still serves every row of a B = 4 batch,
    and equals a (B,) tensor filled with that value bit for bit."""
    rg = rc.build(rc.LENGTH_SETS[0], dtype)
    q, k, v = rg.q.cuda(), rg.k.cuda(), rg.v.cuda()   # no guards: 700 live
    scale = 1.0 / rc.D ** 0.5
    one = ext.flash_attention_cache(q, k, v, _len_dev([700]), scale)
    per_row = ext.flash_attention_cache(q, k, v, _len_dev([700] * rc.B),
                                        scale)
    assert torch.isfinite(one[0]).all()
    assert torch.equal(one[0], per_row[0]) and torch.equal(one[1], per_row[1])


def test_cache_kernel_rejects_other_length_shapes(ext):
    rg = rc.build(rc.LENGTH_SETS[0], "bf16")
    q, k, v = rg.q.cuda(), rg.k.cuda(), rg.v.cuda()
    for n in (2, rc.B + 1):
        with pytest.raises(RuntimeError, match="len_dev"):
            ext.flash_attention_cache(q, k, v, _len_dev([5] * n), 0.1)


# --------------------------------------------------------------------------
# kv_cache_append
# --------------------------------------------------------------------------
def _place(t, block, world):
    return (t // block) % world, block * ((t // block) // world) + t % block


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("rank,world,block", [(1, 3, 4), (0, 1, 64)])
def test_kv_cache_append(ext, dtype, rank, world, block):
    """40 masked steps into sentinel-filled caches: the stored rows are bit
    equal to what the host formula places, the lengths equal the host
    mirror, and every other byte still holds the sentinel. At (0, 1, 64)
    the rows that run past the capacity advance `total` and store
    nothing."""
    bsz, hkv, d, cap, steps = 4, 2, 128, 64, 40
    td = rc._TD[dtype]
    g = torch.Generator().manual_seed(rc.SEED + block)
    esz = torch.empty(0, dtype=td).element_size()
    kc = torch.full((bsz, hkv, cap, d * esz), 0xA5, dtype=torch.uint8,
                    device="cuda").view(td)
    vc = torch.full((bsz, hkv, cap, d * esz), 0x5A, dtype=torch.uint8,
                    device="cuda").view(td)
    assert kc.shape == (bsz, hkv, cap, d)
    want_k, want_v = kc.cpu().clone(), vc.cpu().clone()
    start = [0, 3, 30, 62]
    total = torch.tensor(start, dtype=torch.long, device="cuda")
    # local_len starts at a value the kernel must leave alone until this
    # rank stores a token of that row
    llen = torch.tensor([0, 1, 2, 3], dtype=torch.long, device="cuda")
    h_total, h_llen = list(start), [0, 1, 2, 3]
    for i in range(steps):
        mask = [(i + b) % 3 != 0 and (b != 1 or i < 25) for b in range(bsz)]
        k_new = torch.randn(bsz, hkv, 1, d, generator=g).to(td)
        v_new = torch.randn(bsz, hkv, 1, d, generator=g).to(td)
        ext.kv_cache_append(kc, vc, k_new.cuda(), v_new.cuda(), total, llen,
                            torch.tensor(mask, dtype=torch.uint8).cuda(),
                            block, rank, world)
        for b in range(bsz):
            if not mask[b]:
                continue
            owner, pos = _place(h_total[b], block, world)
            if owner == rank and pos < cap:
                want_k[b, :, pos] = k_new[b, :, 0]
                want_v[b, :, pos] = v_new[b, :, 0]
                h_llen[b] = pos + 1
            h_total[b] += 1
    assert total.tolist() == h_total and llen.tolist() == h_llen
    assert max(h_total) > cap or world > 1     # (0, 1, 64) overruns rows
    assert torch.equal(kc.cpu().view(torch.uint8), want_k.view(torch.uint8))
    assert torch.equal(vc.cpu().view(torch.uint8), want_v.view(torch.uint8))


def test_kv_cache_append_checks(ext):
    kc = torch.zeros(2, 2, 8, 128, dtype=torch.bfloat16, device="cuda")
    new = torch.zeros(2, 2, 1, 128, dtype=torch.bfloat16, device="cuda")
    lens = torch.zeros(2, dtype=torch.long, device="cuda")
    act = torch.ones(2, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="rank"):
        ext.kv_cache_append(kc, kc.clone(), new, new, lens, lens.clone(),
                            act, 4, 2, 2)
    with pytest.raises(RuntimeError, match="dtype"):
        ext.kv_cache_append(kc, kc.clone(), new.half(), new.half(), lens,
                            lens.clone(), act, 4, 0, 1)
    with pytest.raises(RuntimeError, match="int64"):
        ext.kv_cache_append(kc, kc.clone(), new, new, lens.int(),
                            lens.clone(), act, 4, 0, 1)
    with pytest.raises(RuntimeError, match=r"\(B,\)"):
        ext.kv_cache_append(kc, kc.clone(), new, new, lens, lens.clone(),
                            act[:1], 4, 0, 1)
    assert not kc.any() and not lens.any()


# --------------------------------------------------------------------------
# RaggedDecodeSession
# --------------------------------------------------------------------------
def _session(dtype, cap=rc.CAP, **kw):
    from tree_attention_torch_amd.session import RaggedDecodeSession

    # capacity = (ceil(max_tokens / block) + 1) blocks: 1024 or 4608
    sess = RaggedDecodeSession(rc.B, rc.HKV, rc.D, max_tokens=cap - 256,
                               device="cuda", kv_dtype=dtype, block=256, **kw)
    assert sess.capacity == cap
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


def _guard(sess, rg, lengths):
    """The guard pattern over the session's rows at and past each length,
    in place: a captured step holds the cache's address."""
    rc.write_guards(sess.k, sess.v, rg.q, lengths)


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("lengths,family", SETS)
def test_ragged_session_gpu(ext, lengths, family, dtype):
    rg = rc.build(lengths, dtype, family)
    sess = _session(dtype, rg.cap)
    _feed(sess, rg, lengths)
    for b, n in enumerate(lengths):   # stored bytes are the ones .to() gives
        assert torch.equal(sess.k[b, :, :n].cpu().view(torch.uint8),
                           rg.k[b, :, :n].view(torch.uint8))
    _guard(sess, rg, lengths)
    out = sess.attend(rg.q.cuda())
    rc.compare(rg, out, None, "RaggedDecodeSession.attend")


def test_ragged_session_gpu_generic_path(ext):
    """D = 64 does not take the zero-copy kernel: the per-row loop over
    local_attention, empty row included; graphed_step refuses it."""
    from tree_attention_torch_amd.ops.reference import flash_res_lse
    from tree_attention_torch_amd.session import RaggedDecodeSession

    torch.manual_seed(3)
    b, h, d = 3, 2, 64
    sess = RaggedDecodeSession(b, h, d, max_tokens=512, device="cuda",
                               kv_dtype="bf16", block=128)
    lengths = (200, 0, 77)
    ks = torch.randn(b, h, 200, d, device="cuda").bfloat16()
    vs = torch.randn(b, h, 200, d, device="cuda").bfloat16()
    for row, n in enumerate(lengths):
        if n:
            sess.prefill(row, ks[row, :, :n - 1], vs[row, :, :n - 1])
    sess.append(ks[torch.arange(b), :, [199, 0, 76]][:, :, None],
                vs[torch.arange(b), :, [199, 0, 76]][:, :, None],
                [True, False, True])
    assert sess.totals == list(lengths)
    q = torch.randn(b, h, 1, d, device="cuda").bfloat16()
    out = sess.attend(q)
    assert not out[1].any()
    for row in (0, 2):
        n = lengths[row]
        ref, _ = flash_res_lse(q[row:row + 1].cpu(),
                               ks[row:row + 1, :, :n].cpu(),
                               vs[row:row + 1, :, :n].cpu())
        torch.testing.assert_close(out[row:row + 1].cpu(), ref, rtol=2.5e-2,
                                   atol=2.5e-2)
    with pytest.raises(ValueError, match="zero-copy"):
        sess.graphed_step(q, ks[:, :, :1].contiguous(),
                          vs[:, :, :1].contiguous())


@pytest.mark.parametrize("dtype", rc.DTYPES)
def test_ragged_graphed_step(ext, dtype):
    """One captured step replayed while row 0 crosses the split seam
    (511 -> 512 -> 513), row 1 sits inactive and row 2 stays empty: every
    replay meets the oracle and is bit-equal to an eager twin session fed
    the same stream."""
    first = rc.build(rc.GRAPH_STEPS[0], dtype)
    sess, twin = _session(dtype), _session(dtype)
    for s in (sess, twin):
        _feed(s, first, rc.GRAPH_START)
    ks, vs = (t.cuda() for t in rc.stream(first))
    q_static = torch.zeros_like(first.q, device="cuda")
    k_static = torch.zeros(rc.B, rc.HKV, 1, rc.D, dtype=torch.bfloat16,
                           device="cuda")
    v_static = torch.zeros_like(k_static)
    replay = sess.graphed_step(q_static, k_static, v_static)
    # neither the warm-up nor the capture moved a length
    assert sess.totals == list(rc.GRAPH_START)
    assert sess.total_dev.tolist() == list(rc.GRAPH_START)
    assert sess.local_len_dev.tolist() == list(rc.GRAPH_START)
    mask = list(rc.GRAPH_MASK)
    before = rc.GRAPH_START
    for lengths in rc.GRAPH_STEPS:
        rg = rc.build(lengths, dtype)
        bi = torch.arange(rc.B)
        at = torch.tensor(before)
        k_new, v_new = ks[bi, :, at][:, :, None], vs[bi, :, at][:, :, None]
        for s in (sess, twin):     # guards from the OLD lengths on: the
            _guard(s, rg, before)  # append lands on the first guard row
        q_static.copy_(rg.q)
        k_static.copy_(k_new)
        v_static.copy_(v_new)
        out = replay(mask)
        assert sess.totals == list(lengths)
        assert sess.local_len_dev.tolist() == list(lengths)
        rc.compare(rg, out, None, "graphed_step replay")
        twin.append(k_new, v_new, mask)
        eager = twin.attend(rg.q.cuda())
        assert torch.equal(out, eager), f"replay != eager twin at {lengths}"
        assert torch.equal(sess.k.view(torch.uint8), twin.k.view(torch.uint8))
        before = lengths


def test_ragged_graphed_step_capacity(ext):
    """replay() checks the host mirror before anything is launched."""
    from tree_attention_torch_amd.session import RaggedDecodeSession

    sess = RaggedDecodeSession(2, 2, 128, max_tokens=64, device="cuda",
                               kv_dtype="bf16", block=64)
    new = torch.ones(2, 2, 1, 128, dtype=torch.bfloat16, device="cuda")
    q = torch.ones(2, 8, 1, 128, dtype=torch.bfloat16, device="cuda")
    sess.prefill(1, new[0].expand(2, 128, 128), new[0].expand(2, 128, 128))
    replay = sess.graphed_step(q, new, new)
    with pytest.raises(RuntimeError, match="row 1 "):
        replay()
    assert sess.totals == [0, 128] and sess.total_dev.tolist() == [0, 128]
    out = replay([True, False])
    assert sess.total_dev.tolist() == [1, 128]
    assert torch.isfinite(out).all()


# --------------------------------------------------------------------------
# multi-rank (RCCL): auto-skips below 2 GPUs
# --------------------------------------------------------------------------
def _ragged_rccl_worker(rank, world, port):
    import os

    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import ragged_cases as rcw
    from tree_attention_torch_amd.parallel.pg import cleanup, setup
    from tree_attention_torch_amd.session import RaggedDecodeSession

    device = torch.device(f"cuda:{rank}")
    setup(rank, world)
    try:
        lengths = rcw.LENGTH_SETS[0]
        rg = rcw.build(lengths, "bf16")
        sess = RaggedDecodeSession(rcw.B, rcw.HKV, rcw.D, max_tokens=2048,
                                   device=device, kv_dtype="bf16", block=64)
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
        for combine in ("allgather", "allreduce"):
            out = sess.attend(rg.q.to(device), combine=combine)
            torch.cuda.synchronize()
            rcw.compare(rg, out, None, f"rank {rank} {combine}")
    finally:
        cleanup()


@pytest.mark.skipif(NGPU < 2, reason=f"needs >=2 GPUs, have {NGPU}")
def test_rccl_ragged_session():
    import torch.multiprocessing as mp

    mp.spawn(_ragged_rccl_worker, args=(NGPU, _PORT), nprocs=NGPU, join=True)
