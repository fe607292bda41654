"""ta.mla_decode_paged and ta.PagedMlaSession on CPU tensors: fp64 reference,
argument rejections, and two gloo ranks against the unsharded session."""

import os

import pytest
import torch
import torch.multiprocessing as mp

import tree_attention_torch_amd as ta
from mla_paged_cases import chain, check, paged, ref64, session_walk

LENS = [0, 1, 64, 65, 128, 129, 257, 1000]


@pytest.mark.parametrize("page", [128, 512])
def test_seams(page):
    rows, pool, table = paged(LENS, page)
    q = torch.randn(len(LENS), 16, 1, 576).bfloat16()
    out, lse = ta.mla_decode_paged(q, pool, table, torch.tensor(LENS))
    assert (out[0] == 0).all() and (lse[0] == -float("inf")).all()
    check(out, lse, *ref64(q, rows))


@pytest.mark.parametrize("explicit", [False, True])
def test_multi_token(explicit):
    lens, tq = [130, 300, 65], 5
    rows, pool, table = paged(lens, 128, seed=1)
    q = torch.randn(3, 16, tq, 576).bfloat16()
    vis = [[7, 0, n, 64, n - 2] for n in lens] if explicit else None
    out, lse = ta.mla_decode_paged(
        q, pool, table, torch.tensor(lens),
        vis=torch.tensor(vis) if explicit else None, softmax_scale=0.1352)
    check(out, lse, *ref64(q, rows, vis or chain(lens, tq), 0.1352))


def test_rejections():
    rows, pool, table = paged([5], 128)
    q, lens = torch.zeros(1, 16, 2, 576).bfloat16(), torch.tensor([5])
    bad = [
        dict(q=q[..., :512]), dict(q=q.repeat(1, 1, 9, 1)),
        dict(q=q.repeat(1, 9, 1, 1)), dict(pool=pool[:, :, :100]),
        dict(pool=pool.half()), dict(page_table=table.long()),
        dict(page_table=table.repeat(2, 1)), dict(kv_lens=lens.repeat(2)),
        dict(vis=torch.zeros(1, 3, dtype=torch.long)),
    ]
    for kw in bad:
        args = dict(q=q, pool=pool, page_table=table, kv_lens=lens, vis=None)
        args.update(kw)
        with pytest.raises(ValueError):
            ta.mla_decode_paged(**args)
    with pytest.raises(NotImplementedError):   # the slab entry keeps its contract
        ta.mla_decode(q, rows[0][None, None])
    sess = ta.PagedMlaSession(1, 100, device="cpu")
    for call in (lambda: sess.fork(0, 0), lambda: sess.graphed_step_many(q, q),
                 lambda: ta.PagedMlaSession(1, 100, dtype="fp8", device="cpu")):
        with pytest.raises(NotImplementedError):
            call()


def test_session():
    session_walk("cpu")


def _worker(rank, port, path):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        got = session_walk("cpu", block=64)   # checks against fp64 inside
        torch.testing.assert_close(got, torch.load(path), rtol=1e-5, atol=1e-5)
    finally:
        dist.destroy_process_group()


def test_session_ws2(tmp_path):
    path = str(tmp_path / "unsharded.pt")
    torch.save(session_walk("cpu", block=64), path)
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 29871, path)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    for p in procs:
        assert p.exitcode == 0, f"worker failed with exit code {p.exitcode}"
