"""The fp8_block latent store on the CPU: quantizer round trip, the paged
decode route over a uint8 pool and a PagedMlaSession(dtype="fp8_block") walk."""

import pytest
import torch

import tree_attention_torch_amd as ta
from mla_fp8_cases import paged_fp8, session_walk, spread
from mla_paged_cases import check, ref64
from tree_attention_torch_amd.ops.flash import MLA_FP8_ROW
from tree_attention_torch_amd.quant import dequantize_mla_fp8, quantize_mla_fp8


@pytest.mark.parametrize("shape", [(576,), (3, 5, 576)])
def test_round_trip(shape):
    x = spread(torch.randn(*shape).bfloat16().reshape(-1, 576)).reshape(shape)
    rows = quantize_mla_fp8(x)
    assert rows.shape == shape[:-1] + (MLA_FP8_ROW,) and rows.dtype == torch.uint8
    back = dequantize_mla_fp8(rows)
    assert back.shape == shape and back.dtype == torch.float32
    assert torch.equal(back[..., 512:], x[..., 512:].float())
    lat = x[..., :512].float().reshape(*shape[:-1], 4, 128)
    err = (back[..., :512].reshape(lat.shape) - lat).abs()
    assert (err <= 2.0 ** -4 * lat.abs().amax(-1, keepdim=True)).all()
    zero = quantize_mla_fp8(torch.zeros(576))
    assert (zero[:512] == 0).all() and (dequantize_mla_fp8(zero) == 0).all()
    assert torch.equal(zero[512:528].view(torch.float32),
                       torch.full((4,), 2.0 ** -100 / 448))


@pytest.mark.parametrize("tq", [1, 3])
def test_decode_paged_cpu(tq):
    lens = [0, 1, 129, 300]
    rows, pool, table = paged_fp8(lens, 128)
    q = torch.randn(len(lens), 16, tq, 576).bfloat16()
    vis = [[7, 0, n + 9][:tq] for n in lens] if tq > 1 else None
    out, lse = ta.mla_decode_paged(q, pool, table, torch.tensor(lens),
                                   vis=None if vis is None else torch.tensor(vis))
    want = None if vis is None else [[min(v, n) for v in r]
                                     for r, n in zip(vis, lens)]
    check(out, lse, *ref64(q, rows, want))
    with pytest.raises(NotImplementedError):   # the rotary columns are bf16
        ta.mla_decode_paged(q.half(), pool, table, torch.tensor(lens))
    with pytest.raises(ValueError):
        ta.mla_decode_paged(q, pool[..., :576], table, torch.tensor(lens))


def test_session():
    session_walk("cpu")
    with pytest.raises(NotImplementedError):
        ta.PagedMlaSession(1, 100, dtype="fp8", device="cpu")
