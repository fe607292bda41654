"""fa_mla_decode_kernel through ta.mla_decode against an fp64 masked softmax
over the rounded inputs, at the smallest shapes at which the shared-row
design can fail: tile and chunk seams, part-filled head slabs, two head
groups, ragged lengths over a strided cache, and needles that tell the two
products' keys and columns apart."""

import math

import pytest
import torch

import tree_attention_torch_amd as ta
from needle_cases import BARS

pytestmark = pytest.mark.gpu

OUT_BAR, LSE_BAR = BARS["half"]
BF16, FP16 = torch.bfloat16, torch.float16


def ref64(q, ckv, lens=None, scale=None):
    """softmax(q ckv^T * scale) ckv[:, :512] in fp64; keys >= lens[b] masked."""
    scale = scale or 1.0 / math.sqrt(576)
    k = ckv.double().cpu().nan_to_num(0.0)
    s = torch.matmul(q.double().cpu(), k.transpose(-2, -1)) * scale
    if lens is not None:
        dead = torch.arange(k.shape[2])[None, :] >= torch.as_tensor(lens)[:, None]
        s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.clamp(min=-1e300).unsqueeze(-1)).nan_to_num(0.0)
    return torch.matmul(p, k[..., :512]), lse


def data(b, hq, tkv, dtype=BF16, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, hq, 1, 576, generator=g).to(dtype)
    ckv = torch.randn(b, 1, tkv, 576, generator=g).to(dtype)
    return q, ckv


def check(out, lse, ro, rl):
    print("max |out err|", (out.double().cpu() - ro).abs().max().item(),
          "max |lse err|", (lse.double().cpu() - rl).abs().max().item())
    torch.testing.assert_close(out.double().cpu(), ro, rtol=OUT_BAR, atol=OUT_BAR)
    torch.testing.assert_close(lse.double().cpu(), rl, rtol=LSE_BAR, atol=LSE_BAR)


@pytest.mark.parametrize("hq", [16, 40, 64, 128])
@pytest.mark.parametrize("tkv", [1, 63, 64, 65, 129, 513, 1000])
def test_seams(tkv, hq):
    q, ckv = data(2, hq, tkv)
    out, lse = ta.mla_decode(q.cuda(), ckv.cuda())
    assert out.shape == (2, hq, 1, 512) and lse.shape == (2, hq, 1)
    check(out, lse, *ref64(q, ckv))


@pytest.mark.parametrize("dtype,scale", [(FP16, None), (BF16, 0.1352)])
def test_dtype_and_scale(dtype, scale):
    q, ckv = data(2, 32, 200, dtype)
    out, lse = ta.mla_decode(q.cuda(), ckv.cuda(), softmax_scale=scale)
    check(out, lse, *ref64(q, ckv, scale=scale))


def test_forced_splits():
    # 128-key chunks, the last holding 44 keys
    q, ckv = data(2, 40, 300)
    o3, l3 = ta.mla_decode(q.cuda(), ckv.cuda(), splits=3)
    o1, l1 = ta.mla_decode(q.cuda(), ckv.cuda(), splits=1)
    check(o3, l3, *ref64(q, ckv))
    check(o3, l3, o1.double().cpu(), l1.double().cpu())


def test_ragged_strided():
    lens = [0, 65, 200]
    q, _ = data(3, 40, 1)
    buf = torch.randn(3, 1, 256, 576, generator=torch.Generator().manual_seed(1))
    buf = buf.to(BF16)
    for b, n in enumerate(lens):
        buf[b, :, n:] = float("nan")
    ckv = buf.cuda()[:, :, :200]
    out, lse = ta.mla_decode(q.cuda(), ckv, kv_lens=torch.tensor(lens).cuda())
    assert (out[0] == 0).all() and (lse[0] == float("-inf")).all()
    assert torch.isfinite(out[1:]).all() and torch.isfinite(lse[1:]).all()
    ro, rl = ref64(q, buf[:, :, :200], lens)
    check(out[1:], lse[1:], ro[1:], rl[1:])


@pytest.mark.parametrize("hq", [16, 64])
def test_needle(hq):
    # q[h] = ckv[j_h]: the target scores |row|^2 / 24 ~ 24, the rest ~ N(0, 1)
    _, ckv = data(1, hq, 130, seed=2)
    j = torch.tensor([0, 63, 64, 129]).repeat(hq // 4)
    q = ckv[0, 0, j][None, :, None, :].contiguous()
    ro, _ = ref64(q, ckv)
    want = ckv[0, 0, j, :512].double()[None, :, None, :]
    s = torch.matmul(q.double(), ckv.double().transpose(-2, -1)) / 24.0
    assert (torch.softmax(s, -1)[0, torch.arange(hq), 0, j] > 1 - 1e-6).all()
    out, _ = ta.mla_decode(q.cuda(), ckv.cuda())
    torch.testing.assert_close(out.double().cpu(), want, rtol=OUT_BAR, atol=OUT_BAR)
    torch.testing.assert_close(ro, want, rtol=OUT_BAR, atol=OUT_BAR)


def test_shard_algebra():
    q, ckv = data(2, 40, 1000)
    qd, cd = q.cuda(), ckv.cuda()
    halves = [ta.mla_decode(qd, cd[:, :, :500]), ta.mla_decode(qd, cd[:, :, 500:])]
    out, lse = ta.combine_partials(torch.stack([h[0] for h in halves]),
                                   torch.stack([h[1] for h in halves]))
    whole = ta.mla_decode(qd, cd)
    check(out, lse, whole[0].double().cpu(), whole[1].double().cpu())
    check(out, lse, *ref64(q, ckv))
