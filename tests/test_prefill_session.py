"""attend_prefill of the ragged and paged sessions: a forked prefix plus a
prefilled suffix, the suffix's queries against the fp64 reference over the
concatenated tokens (tests/prefill_cases.py)."""

import pytest
import torch

import prefill_cases as pc
from tree_attention_torch_amd.session import (PagedDecodeSession,
                                              RaggedDecodeSession)

PREFIX, SUFFIX, G = 200, 150, 4


def _session(kind, device, kv_dtype):
    kw = dict(max_tokens=512, device=device, kv_dtype=kv_dtype, block=64)
    if kind == "paged":
        return PagedDecodeSession(2, pc.HKV, pc.D, pool_tokens=1024, page=128,
                                  **kw)
    return RaggedDecodeSession(2, pc.HKV, pc.D, **kw)


def _forked(kind, device, kv_dtype, dtype):
    """Row 0 holds the prefix; row 1 forks it and prefills the suffix.
    Returns the session and (q, k, v, vis) of the suffix over all tokens."""
    q, k, v, vis = pc.make(PREFIX, SUFFIX, (0, 1, 64), dtype, G, aimed=False)
    sess = _session(kind, device, kv_dtype)
    kd, vd = k.to(device), v.to(device)
    sess.prefill(0, kd[:, :PREFIX], vd[:, :PREFIX])
    sess.fork(0, 1)
    sess.prefill(1, kd[:, PREFIX:], vd[:, PREFIX:])
    return sess, (q, k, v, vis)


@pytest.mark.parametrize("kind", ["ragged", "paged"])
def test_attend_prefill_cpu(kind):
    sess, (q, k, v, vis) = _forked(kind, "cpu", "fp32", torch.float32)
    before = (list(sess.totals), list(sess.local_lens),
              getattr(sess, "free_pages", None))
    out = sess.attend_prefill(1, q)
    ref, _ = pc.reference(q, k, v, vis)
    assert out.shape == (1, pc.HKV * G, SUFFIX, pc.D)
    assert out.dtype == torch.float32
    torch.testing.assert_close(out[0].double(), ref, rtol=1e-4, atol=1e-5)
    # (Hq, T, D) or (1, Hq, T, D); a scale of the caller's
    half = sess.attend_prefill(1, q[None], softmax_scale=0.5 * pc.SCALE)
    ref_half, _ = pc.reference(q, k, v, vis, 0.5 * pc.SCALE)
    torch.testing.assert_close(half[0].double(), ref_half, rtol=1e-4,
                               atol=1e-5)
    assert before == (sess.totals, sess.local_lens,
                      getattr(sess, "free_pages", None))
    assert sess.total_dev.tolist() == sess.totals
    for bad_b, bad_q in ((2, q), (-1, q), (1, q[:, :, :64]), (1, q[:3]),
                         (1, q[None, None]),
                         (0, torch.zeros(8, PREFIX + 1, pc.D))):
        with pytest.raises(ValueError):
            sess.attend_prefill(bad_b, bad_q)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["ragged", "paged"])
def test_attend_prefill_gpu(kind):
    """Page 128, prefix 200, suffix 150, G = 4: the kernel path agrees with
    the CPU session and with the fp64 reference inside the prefill bars."""
    sess, (q, k, v, vis) = _forked(kind, "cuda", "bf16", torch.bfloat16)
    out = sess.attend_prefill(1, q.cuda())[0].cpu()
    cpu, _ = _forked(kind, "cpu", "bf16", torch.bfloat16)
    ref, _ = pc.reference(q, k, v, vis)
    torch.testing.assert_close(out, cpu.attend_prefill(1, q)[0], **pc.OUT_TOL)
    torch.testing.assert_close(out.double(), ref, **pc.OUT_TOL)
    assert sess.total_dev.tolist() == sess.totals == [PREFIX, PREFIX + SUFFIX]


@pytest.mark.gpu
@pytest.mark.parametrize("kv_dtype", ["fp8", "fp8_scaled"])
def test_attend_prefill_fp8_raises(kv_dtype):
    sess = _session("paged", "cuda", kv_dtype)
    kv = torch.randn(pc.HKV, 8, pc.D, device="cuda")
    sess.prefill(0, kv, kv)
    with pytest.raises(NotImplementedError):
        sess.attend_prefill(0, torch.zeros(8, 4, pc.D, device="cuda",
                                           dtype=torch.bfloat16))
