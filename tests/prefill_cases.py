"""Inputs and the reference of the chunked-prefill tests: T queries of one
sequence over the local keys a rank holds, fp64 masked softmax on the
rounded inputs."""

import torch

D, HKV = 128, 2
SCALE = 1.0 / D ** 0.5
AIM = 5.0   # aimed queries are AIM * key: with randn keys the aimed score is
            # ~56 and beats every visible one by > 24 in the cases that aim
            # (checked on the CPU), so the aimed key would weigh > 0.99
# the project's two-byte prefill bars (tests/test_gpu_kernels.py)
OUT_TOL = dict(rtol=2.5e-2, atol=2.5e-2)
LSE_TOL = dict(rtol=1e-3, atol=1e-3)


def make(t0, t, rwb, dtype, g, aimed, seed=0):
    """The last t of t0 + t tokens query what (rank, world, block) = rwb owns
    of them: q (HKV * g, t, D), local k / v (HKV, n, D), vis (t,) int64 by a
    brute-force count. aimed: query i is AIM * k[first key it must NOT see],
    or the last visible key where there is none."""
    rank, world, block = rwb
    gen = torch.Generator().manual_seed(1234 + seed)
    own = [x for x in range(t0 + t) if (x // block) % world == rank]
    vis = torch.tensor([sum(1 for x in own if x <= t0 + i) for i in range(t)])
    k = torch.randn(HKV, len(own), D, generator=gen).to(dtype)
    v = torch.randn(HKV, len(own), D, generator=gen).to(dtype)
    q = torch.randn(HKV * g, t, D, generator=gen).to(dtype)
    if aimed:
        tgt = vis.clamp(max=len(own) - 1)
        q = (AIM * k[:, tgt].float()).to(dtype).repeat_interleave(g, dim=0)
    return q, k, v, vis


def reference(q, k, v, vis, scale=SCALE):
    """fp64 (out (Hq, T, D), lse (Hq, T)); a query with vis = 0 gets out = 0,
    lse = -inf."""
    g = q.shape[0] // k.shape[0]
    kd = k.double().repeat_interleave(g, dim=0)
    vd = v.double().repeat_interleave(g, dim=0)
    s = q.double() @ kd.transpose(-1, -2) * scale
    hidden = torch.arange(k.shape[1])[None, :] >= vis[:, None]
    s = s.masked_fill(hidden, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.clamp_min(-1e300)[..., None])
    return p @ vd, lse
