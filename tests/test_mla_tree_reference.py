"""Tree drafts of ta.PagedMlaSession and mla_decode_paged(tree=) on CPU
tensors: the session walk against fp64, two gloo ranks against the unsharded
walk, and the rejections of tree=."""

import os

import pytest
import torch
import torch.multiprocessing as mp

import tree_attention_torch_amd as ta
from mla_paged_cases import paged
from mla_tree_cases import tree_walk


@pytest.mark.parametrize("dtype", ["bf16", "fp8_block"])
def test_session(dtype):
    tree_walk("cpu", dtype)


def _worker(rank, port, path):
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      RANK=str(rank))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    try:
        got = tree_walk("cpu", block=64)   # checks against fp64 inside
        torch.testing.assert_close(got, torch.load(path), rtol=1e-5, atol=1e-5)
    finally:
        dist.destroy_process_group()


def test_session_ws2(tmp_path):
    path = str(tmp_path / "unsharded.pt")
    torch.save(tree_walk("cpu", block=64), path)
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, 29873, path)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
    for p in procs:
        assert p.exitcode == 0, f"worker failed with exit code {p.exitcode}"


def test_rejections():
    _, pool, table = paged([5], 128)
    q, lens = torch.zeros(1, 16, 2, 576).bfloat16(), torch.tensor([5])
    base, mask = torch.tensor([3]), torch.zeros(1, 2, dtype=torch.int32)
    ta.mla_decode_paged(q, pool, table, lens, tree=(base, mask))
    bad = [
        dict(tree=(base, mask), vis=torch.zeros(1, 2, dtype=torch.long)),
        dict(tree=(base.int(), mask)), dict(tree=(base, mask.long())),
        dict(tree=(base.repeat(2), mask)), dict(tree=(base, mask[:, :1])),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            ta.mla_decode_paged(q, pool, table, lens, **kw)
