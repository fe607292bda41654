"""RaggedDecodeSession on the CPU: per-sequence lengths, masked appends,
slot reuse, capacity and block-cyclic sharding, against the fp32 oracle on
each row's own prefix."""

import os
import random

import pytest
import torch
import torch.multiprocessing as mp

from tree_attention_torch_amd.ops.reference import flash_res_lse
from tree_attention_torch_amd.session import RaggedDecodeSession


def _check_rows(sess, q, ks, vs, out):
    """attend() row b == the oracle over sequence b's own prefix; a row
    that holds no token is all zeros."""
    for b, n in enumerate(sess.totals):
        if n == 0:
            assert not out[b].any(), f"row {b} is empty but not zero"
            continue
        ref, _ = flash_res_lse(q[b:b + 1], ks[b][None, :, :n],
                               vs[b][None, :, :n])
        torch.testing.assert_close(out[b:b + 1], ref, rtol=1e-5, atol=1e-5)


def _check_mirror(sess):
    assert sess.total_dev.tolist() == sess.totals
    assert sess.local_len_dev.tolist() == sess.local_lens


def test_ragged_session_single_rank_cpu():
    torch.manual_seed(0)
    b, h, d, t_max = 3, 4, 32, 64
    sess = RaggedDecodeSession(b, h, d, max_tokens=512, device="cpu",
                               kv_dtype="fp32", block=8)
    # what each sequence holds, in order (rows grow at their own pace)
    ks = [torch.randn(h, t_max, d) for _ in range(b)]
    vs = [torch.randn(h, t_max, d) for _ in range(b)]
    for row, n in enumerate((0, 9, 20)):
        if n:   # (Hkv, T, D) and (1, Hkv, T, D) are both accepted
            if row == 1:
                sess.prefill(row, ks[row][:, :n], vs[row][:, :n])
            else:
                sess.prefill(row, ks[row][None, :, :n], vs[row][None, :, :n])
    assert sess.totals == [0, 9, 20]
    _check_mirror(sess)
    out = sess.attend(torch.randn(b, h, 1, d))
    assert not out[0].any()

    def step(mask):
        k_new = torch.stack([ks[r][:, sess.totals[r]:sess.totals[r] + 1]
                             for r in range(b)])
        v_new = torch.stack([vs[r][:, sess.totals[r]:sess.totals[r] + 1]
                             for r in range(b)])
        sess.append(k_new, v_new, mask)
        _check_mirror(sess)
        q = torch.randn(b, h, 1, d)
        _check_rows(sess, q, ks, vs, sess.attend(q))

    for i in range(30):
        # row 1 idles on odd steps; the three accepted mask types
        mask = [True, i % 2 == 0, True]
        step(None if all(mask) and i % 4 == 0 else
             torch.tensor(mask) if i % 3 == 0 else mask)
    assert sess.totals == [30, 24, 50]

    sess.reset(2)
    assert sess.totals == [30, 24, 0] and sess.local_lens[2] == 0
    _check_mirror(sess)
    q = torch.randn(b, h, 1, d)
    out = sess.attend(q)
    _check_rows(sess, q, ks, vs, out)
    assert not out[2].any()
    for i in range(10):    # the slot is reused from length 0
        step([False, i % 2 == 1, True])
    assert sess.totals == [30, 29, 10]


def test_ragged_session_capacity_names_the_row():
    torch.manual_seed(1)
    sess = RaggedDecodeSession(2, 2, 16, max_tokens=8, device="cpu",
                               kv_dtype="fp32", block=4)
    assert sess.capacity == 12      # 3 blocks of 4
    k1 = torch.randn(2, 2, 1, 16)
    for _ in range(10):
        sess.append(k1, k1)
    for _ in range(2):
        sess.append(k1, k1, [False, True])
    assert sess.totals == [10, 12]
    before = (sess.k.clone(), sess.v.clone(), list(sess.totals),
              list(sess.local_lens))
    with pytest.raises(RuntimeError, match=r"capacity exceeded: row 1 "):
        sess.append(2 * k1, 2 * k1)         # row 0 has room, row 1 has none
    # nothing was stored for ANY row on that call
    assert torch.equal(sess.k[:, :, :12], before[0][:, :, :12])
    assert torch.equal(sess.v[:, :, :12], before[1][:, :, :12])
    assert sess.totals == before[2] and sess.local_lens == before[3]
    _check_mirror(sess)
    sess.append(k1, k1, [True, False])      # row 0 alone still fits
    assert sess.totals == [11, 12]
    with pytest.raises(RuntimeError, match=r"row 1 "):
        sess.prefill(1, k1[0], k1[0])
    with pytest.raises(ValueError, match="active"):
        sess.append(k1, k1, [True])


def test_ragged_session_rejects_mx():
    for name in ("mx", "fp8_mx"):
        with pytest.raises(ValueError, match="MX"):
            RaggedDecodeSession(2, 2, 128, max_tokens=128, device="cpu",
                                kv_dtype=name, block=64)


def _worker(rank, world, port, combine):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.manual_seed(0)
        b, h, d, t_max = 4, 2, 16, 40
        sess = RaggedDecodeSession(b, h, d, max_tokens=256, device="cpu",
                                   kv_dtype="fp32", block=4)
        ks = [torch.randn(h, t_max, d) for _ in range(b)]
        vs = [torch.randn(h, t_max, d) for _ in range(b)]
        for row, n in enumerate((0, 3, 9, 21)):
            if n:
                sess.prefill(row, ks[row][:, :n], vs[row][:, :n])
        assert sess.totals == [0, 3, 9, 21]
        # block 4, world 2: tokens 0..3 live on rank 0 alone
        assert sess.local_lens[1] == (3 if rank == 0 else 0)
        masks = ([False, False, True, True], [False, True, True, False],
                 [False, False, False, True], [False, False, True, True],
                 [False, False, True, False], [False, False, True, True])
        for mask in masks:
            k_new = torch.stack([ks[r][:, sess.totals[r]:sess.totals[r] + 1]
                                 for r in range(b)])
            v_new = torch.stack([vs[r][:, sess.totals[r]:sess.totals[r] + 1]
                                 for r in range(b)])
            sess.append(k_new, v_new, mask)
            _check_mirror(sess)
            q = torch.randn(b, h, 1, d)
            out = sess.attend(q, combine=combine)
            _check_rows(sess, q, ks, vs, out)
        assert sess.totals == [0, 4, 14, 25]
        # row 0 never held a token; row 1's four tokens all sit on rank 0
        assert sess.local_lens[0] == 0
        assert sess.local_lens[1] == (4 if rank == 0 else 0)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("combine,port", [("allgather", 29761),
                                          ("allreduce", 29762)])
def test_ragged_session_sharded_ws2(combine, port):
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 2, port, combine))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("block", [1, 4])
def test_ragged_block_cyclic_ownership(world, block):
    """Replay a random mask sequence through every rank's host formula:
    token t of sequence b is stored on rank (t // block) % world at local
    position block * ((t // block) // world) + t % block (the module
    docstring's layout), and nowhere else."""
    rng = random.Random(1000 * world + block)
    b, h, d, steps = 3, 1, 4, 40
    sessions = [RaggedDecodeSession(b, h, d, max_tokens=steps + 8,
                                    device="cpu", kv_dtype="fp32",
                                    block=block) for _ in range(world)]
    for r, s in enumerate(sessions):   # no process group in this process
        s.rank, s.world = r, world
        s.k.fill_(-1.0)
        s.v.fill_(-1.0)
    # sequence 1 starts from a prompt that ends inside a block
    for s in sessions:
        prompt = torch.arange(5, dtype=torch.float32)[None, :, None]
        s.prefill(1, (1000 + prompt).expand(h, 5, d),
                  (1000 + prompt).expand(h, 5, d))
    for _ in range(steps):
        mask = [rng.random() < 0.6 for _ in range(b)]
        for s in sessions:
            # the token's value names its sequence and global index
            tok = torch.tensor([1000.0 * row + s.totals[row]
                                for row in range(b)])
            k_new = tok[:, None, None, None].expand(b, h, 1, d)
            s.append(k_new, k_new, mask)
    totals = sessions[0].totals
    assert all(s.totals == totals for s in sessions)
    for r, s in enumerate(sessions):
        want = torch.full_like(s.k, -1.0)
        for row in range(b):
            owned = 0
            for t in range(totals[row]):
                if (t // block) % world == r:
                    pos = block * ((t // block) // world) + t % block
                    want[row, :, pos] = 1000.0 * row + t
                    owned += 1
            assert s.local_lens[row] == owned, (r, row)
        assert torch.equal(s.k, want), f"rank {r}: misplaced token"
        assert torch.equal(s.v, want)
        assert s.local_len_dev.tolist() == s.local_lens
