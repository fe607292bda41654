"""ta.mla_prefill_paged(..., compute="fp8") on CPU tensors: the host oracle of
fa_mla_prefill_fp8_kernel (fp32 over the dequantized rows and the e4m3-rounded
queries) against ref64, and what the keyword refuses."""

import pytest
import torch

import tree_attention_torch_amd as ta
from mla_fp8_cases import deq, paged_fp8, spread
from mla_paged_cases import chain, check, paged, ref64


@pytest.mark.parametrize("hq,t,lens", [(16, 9, [130, 300, 65]),
                                       (8, 70, [200])])
def test_entry(hq, t, lens):
    rows, pool, table = paged_fp8(lens, 128, seed=1)
    q = spread(torch.randn(len(lens), hq, t, 576)).bfloat16()
    out, lse = ta.mla_prefill_paged(q, pool, table, torch.tensor(lens),
                                    compute="fp8")
    check(out, lse, *ref64(deq(q), rows, chain(lens, t)))
    # the rounding is real: the unrounded call differs
    plain, _ = ta.mla_prefill_paged(q, pool, table, torch.tensor(lens))
    assert not torch.equal(plain, out)


def test_rejections():
    lens = torch.tensor([5])
    q = torch.zeros(1, 16, 3, 576).bfloat16()
    _, pool8, table8 = paged_fp8([5], 128)
    with pytest.raises(ValueError):
        ta.mla_prefill_paged(q, pool8, table8, lens, compute="bf16")
    _, pool, table = paged([5], 128)
    with pytest.raises(ValueError):
        ta.mla_prefill_paged(q, pool, table, lens, compute="fp8")
    with pytest.raises(NotImplementedError):   # fp16 q over fp8_block
        ta.mla_prefill_paged(q.half(), pool8, table8, lens, compute="fp8")
    sess = ta.PagedMlaSession(1, 100, device="cpu")
    sess.prefill(0, torch.zeros(5, 576).bfloat16())
    with pytest.raises(ValueError):
        sess.attend_prefill(0, q[0], compute="fp8")
