"""kv_dtype="fp8_scaled" on the CPU: the quantizer oracle and the sessions."""

import pytest
import torch

import scaled_cases as sc
from tree_attention_torch_amd.quant import (dequantize_rows_fp8,
                                            quantize_rows_fp8)
from tree_attention_torch_amd.session import (DecodeSession,
                                              RaggedDecodeSession)


def test_quantizer_roundtrip():
    k, _ = sc.make_kv()[3]
    x = torch.cat([k[0].float(), torch.zeros(1, sc.D)])
    payload, scale = quantize_rows_fp8(x)
    dq = dequantize_rows_fp8(payload, scale)
    assert torch.isfinite(dq).all() and torch.isfinite(scale.log()).all()
    # 3 mantissa bits, plus half the smallest subnormal of the scaled row
    assert ((x - dq).abs() <= x.abs() / 16 + scale[:, None] * 2.0 ** -10).all()
    assert (dq[-1] == 0).all() and scale[-1] > 0
    assert dq[sc.OUTLIER_AT].abs().max() > 2900


@pytest.mark.parametrize("kind", ["slab", 128, 256])
def test_cpu_session_matches_fp64(kind):
    seqs = sc.make_kv()
    q = sc.make_q(seqs, 4)
    sess = sc.session(kind)
    sc.fill(sess, seqs)
    assert sess.local_lens == list(sc.LENS)
    rows = sc.stored_rows(sess)
    ref, probs = sc.attention_f64(q, rows)
    sc.check_spread(probs)
    out = sess.attend(q)
    # fp32 scores: 2^-24 * (|q_i k_i| summing to ~300) * sqrt(128); |p v| ~ 6
    torch.testing.assert_close(out.double(), ref, rtol=2e-3, atol=2e-3)
    assert (out[0] == 0).all()
    assert torch.equal(rows[3][0],
                       dequantize_rows_fp8(*quantize_rows_fp8(seqs[3][0])))
    # why the format exists: the same input through plain e4m3
    plain = sc.session(kind, "fp8")
    sc.fill(plain, seqs)
    assert not torch.isfinite(plain.attend(q)).all()


@pytest.mark.parametrize("kind", ["slab", 128])
def test_out_of_scope_raises(kind):
    sess = sc.session(kind)
    q = torch.zeros(sc.B, sc.HKV, 1, sc.D, dtype=torch.bfloat16)
    kv = torch.zeros(sc.B, sc.HKV, 2, sc.D, dtype=torch.bfloat16)
    for call in (lambda: sess.append_many(kv, kv), lambda: sess.attend_many(q),
                 lambda: sess.truncate(0, 0), lambda: sess.fork(0, 1),
                 lambda: sess.append_tree(kv, kv, [[-1, 0]] * sc.B),
                 lambda: sess.attend_tree(q), lambda: sess.commit([], []),
                 lambda: sess.attend(q, shared=True)):
        with pytest.raises(NotImplementedError, match="fp8_scaled"):
            call()
    with pytest.raises(NotImplementedError, match="fp8_scaled"):
        DecodeSession(1, sc.HKV, sc.D, 64, device="cpu",
                      kv_dtype="fp8_scaled")
    with pytest.raises(ValueError, match="head_dim 128"):
        RaggedDecodeSession(1, sc.HKV, 64, 64, device="cpu",
                            kv_dtype="fp8_scaled")
