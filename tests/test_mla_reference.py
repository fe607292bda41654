"""ta.mla_decode / ta.tree_mla_decode on CPU tensors (the fp32 oracle
reference.mla_reference) against an fp64 masked softmax, and the argument
checks of the public entry."""

import math

import pytest
import torch

import tree_attention_torch_amd as ta


def ref64(q, ckv, lens=None):
    s = torch.matmul(q.double(), ckv.double().transpose(-2, -1)) / math.sqrt(576)
    if lens is not None:
        dead = torch.arange(ckv.shape[2])[None, :] >= lens[:, None]
        s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    return (torch.matmul(torch.softmax(s, -1), ckv.double()[..., :512]),
            torch.logsumexp(s, -1))


@pytest.fixture(scope="module")
def qc():
    g = torch.Generator().manual_seed(0)
    return (torch.randn(2, 40, 1, 576, generator=g).bfloat16(),
            torch.randn(2, 1, 333, 576, generator=g).bfloat16())


@pytest.mark.parametrize("lens", [None, [65, 333]])
def test_cpu_matches_fp64(qc, lens):
    q, ckv = qc
    lens = None if lens is None else torch.tensor(lens)
    out, lse = ta.mla_decode(q, ckv, kv_lens=lens)
    assert out.shape == (2, 40, 1, 512) and out.dtype == torch.float32
    ro, rl = ref64(q, ckv, lens)
    torch.testing.assert_close(out.double(), ro, rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(lse.double(), rl, rtol=1e-5, atol=1e-5)


def test_empty_row(qc):
    q, ckv = qc
    out, lse = ta.mla_decode(q, ckv, kv_lens=torch.tensor([0, 5]))
    assert (out[0] == 0).all() and (lse[0] == float("-inf")).all()


def test_shard_algebra_and_tree(qc):
    q, ckv = qc
    whole = ta.mla_decode(q, ckv)
    parts = [ta.mla_decode(q, ckv[:, :, :100]), ta.mla_decode(q, ckv[:, :, 100:])]
    out, lse = ta.combine_partials(torch.stack([p[0] for p in parts]),
                                   torch.stack([p[1] for p in parts]))
    torch.testing.assert_close(out, whole[0], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(lse, whole[1], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(ta.tree_mla_decode(q, ckv), whole[0])


@pytest.mark.parametrize("qs,cs,exc", [
    ((1, 8, 1, 512), (1, 1, 9, 512), ValueError),
    ((1, 8, 1, 576), (1, 1, 9, 512), ValueError),
    ((1, 8, 2, 576), (1, 1, 9, 576), NotImplementedError),
    ((1, 129, 1, 576), (1, 1, 9, 576), ValueError),
])
def test_rejected(qs, cs, exc):
    with pytest.raises(exc, match="576|Tq|128"):
        ta.mla_decode(torch.zeros(qs), torch.zeros(cs))
