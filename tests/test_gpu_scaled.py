"""kv_dtype="fp8_scaled" on the GPU: append, attend and the graphed step."""

import pytest
import torch

import scaled_cases as sc
from needle_cases import BARS
from tree_attention_torch_amd.quant import quantize_rows_fp8

pytestmark = pytest.mark.gpu
KINDS = ["slab", 128, 256]
POISON = 0x7F   # e4m3 NaN


def _session(kind):
    """A GPU session whose every payload byte and scale is NaN."""
    sess = sc.session(kind, device="cuda")
    for t in (sess._kv, sess.v_pool if kind != "slab" else sess.v):
        t.view(torch.uint8).fill_(POISON)
    sess.k_scale.fill_(float("nan")), sess.v_scale.fill_(float("nan"))
    return sess


def _token(x, t):
    return x[:, t][None].repeat(sc.B, 1, 1).unsqueeze(2).cuda().contiguous()


@pytest.mark.parametrize("kind", KINDS)
def test_append_kernel_equals_oracle(kind):
    """One by one across the page boundary at 128; rows 1, 3 inactive."""
    k, v = sc.make_kv()[3]
    sess = _session(kind)
    for b in (0, 1, 2):
        sess.prefill(b, k[:, :126], v[:, :126])
    for t in range(126, 131):
        sess.append(_token(k, t), _token(v, t),
                    active=[True, False, True, False])
    assert sess.total_dev.tolist() == sess.totals == [131, 126, 131, 0]
    assert sess.local_len_dev.tolist() == sess.local_lens == sess.totals
    want = [t[:, :131] for x in (k, v) for t in quantize_rows_fp8(x)]
    for b in (0, 2):
        for got, ref in zip(sc.stored(sess, b, 131), want):
            if ref.dtype != torch.float32:
                got, ref = got.view(torch.uint8), ref.view(torch.uint8)
            assert torch.equal(got, ref)
    # untouched: row 1 behind its 126 tokens, and (slab) all of row 3
    for b, lo in ((1, 126), (3, 0)) if kind == "slab" else ((1, 126),):
        k8, ks, v8, vs = sc.stored(sess, b, 128)
        assert all((t.view(torch.uint8)[:, lo:] == POISON).all()
                   for t in (k8, v8))
        assert ks[:, lo:].isnan().all() and vs[:, lo:].isnan().all()


@pytest.mark.parametrize("g_heads", [1, 4])
@pytest.mark.parametrize("kind", KINDS)
def test_attend_matches_fp64(kind, g_heads):
    """The project's fp8 output bar (4e-2, rtol = atol) against fp64 attention
    of the same q over the dequantized stored rows."""
    seqs = sc.make_kv()
    q = sc.make_q(seqs, g_heads)
    sess = _session(kind)
    sc.fill(sess, seqs)
    ref, probs = sc.attention_f64(q, sc.stored_rows(sess))
    sc.check_spread(probs)
    out = sess.attend(q.cuda()).cpu()
    assert torch.isfinite(out).all() and (out[0] == 0).all()
    torch.testing.assert_close(out.double(), ref, rtol=BARS["fp8"][0],
                               atol=BARS["fp8"][0])


@pytest.mark.parametrize("kind", KINDS)
def test_graphed_step_equals_eager(kind):
    seqs = sc.make_kv()
    k, v = seqs[3]
    q = sc.make_q(seqs, 4).cuda()
    graphed, eager = _session(kind), _session(kind)
    for sess in (graphed, eager):
        for b, n in enumerate((127, 0, 126, 300)):
            if n:
                sess.prefill(b, k[:, :n], v[:, :n])
    qs, ks, vs = torch.zeros_like(q), _token(k, 0), _token(v, 0)
    replay = graphed.graphed_step(qs, ks, vs)
    for step in range(3):
        qs.copy_(q * (1 + step))
        ks.copy_(_token(k, 400 + step))
        vs.copy_(_token(v, 400 + step))
        got = replay().clone()
        eager.append(ks.clone(), vs.clone())
        assert torch.equal(got, eager.attend(qs)), step
    assert graphed.local_len_dev.tolist() == [130, 3, 129, 303]
