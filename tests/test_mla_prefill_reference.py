"""ta.mla_prefill_paged and PagedMlaSession.attend_prefill on CPU tensors: fp64
reference, argument rejections, and two gloo ranks against one."""

import os

import pytest
import torch
import torch.multiprocessing as mp

import tree_attention_torch_amd as ta
from mla_paged_cases import chain, check, paged, ref64


@pytest.mark.parametrize("hq,t,lens,vis", [
    (16, 9, [130, 300, 65], None),
    (8, 70, [200], None),
    (16, 9, [130, 300, 65], [7, 0, 10 ** 6, 64, 65, 128, 129, 60, 1]),
])
def test_entry(hq, t, lens, vis):
    rows, pool, table = paged(lens, 128, seed=1)
    q = torch.randn(len(lens), hq, t, 576).bfloat16()
    vis = vis and [[min(v, n) for v in vis] for n in lens]
    out, lse = ta.mla_prefill_paged(q, pool, table, torch.tensor(lens),
                                    vis=vis and torch.tensor(vis))
    check(out, lse, *ref64(q, rows, vis or chain(lens, t)))


def test_rejections():
    rows, pool, table = paged([5], 128)
    q, lens = torch.zeros(1, 16, 20, 576).bfloat16(), torch.tensor([5])
    for kw in (dict(q=q[..., :512]), dict(q=q[:, :, :0]),
               dict(q=q.repeat(1, 9, 1, 1)), dict(pool=pool[:, :, :100]),
               dict(pool=pool.half()), dict(page_table=table.long()),
               dict(page_table=table.repeat(2, 1)),
               dict(kv_lens=lens.repeat(2)),
               dict(vis=torch.zeros(1, 3, dtype=torch.long))):
        args = dict(q=q, pool=pool, page_table=table, kv_lens=lens)
        args.update(kw)
        with pytest.raises(ValueError):
            ta.mla_prefill_paged(**args)
    sess = ta.PagedMlaSession(1, 100, device="cpu")
    sess.prefill(0, rows[0])
    for bad in (q, q[0, :, :3, :512]):   # more queries than tokens; width
        with pytest.raises(ValueError):
            sess.attend_prefill(0, bad)


def walk(block=256, dtype="bf16"):
    """prefill 130 + 70 rows, attend_prefill over the last 70."""
    g = torch.Generator().manual_seed(5)
    mirror = torch.randn(200, 576, generator=g).bfloat16()
    q = torch.randn(16, 70, 576, generator=g).bfloat16()
    sess = ta.PagedMlaSession(2, 600, page=128, block=block, dtype=dtype,
                              device="cpu")
    sess.prefill(1, mirror[:130])
    sess.prefill(1, mirror[130:])
    state = (list(sess.totals), sess.free_pages)
    out = sess.attend_prefill(1, q)
    assert state == (list(sess.totals), sess.free_pages)
    return out, ref64(q[None], [mirror], chain([200], 70))[0]


def test_session():
    out, want = walk()
    check(out, None, want, None)


def _worker(rank, port, path):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        out, want = walk(block=64)
        check(out, None, want, None)
        torch.testing.assert_close(out, torch.load(path), rtol=1e-5, atol=1e-5)
    finally:
        dist.destroy_process_group()


def test_session_ws2(tmp_path):
    path = str(tmp_path / "unsharded.pt")
    torch.save(walk(block=64)[0], path)
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 29873, path)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    for p in procs:
        assert p.exitcode == 0, f"worker failed with exit code {p.exitcode}"
