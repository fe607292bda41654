"""GPU (MI355X) needle tests: the shared case table of tests/needle_cases.py
through the real entry points, compared with the fp32 oracle by the same
`compare` (and bars) that tests/test_needle_sensitivity.py proves sensitive
on the CPU: every row of the table rejects a causal mask off by one, a
dropped or admitted tail key, V rows exchanged across each seam it names, a
wrong GQA head map and a transposed (head, row) batch; every row with B > 1
a batch index dropped from a KV base, exchanged in an output offset or decoded
transposed with the head; every row with a softmax scale of its own a kernel
that ignores it.

The many-split rows (S = 3 .. 63 splits: 1100 .. 8193 keys, and two rows
of 40000) put a needle in every split and on both sides of every split seam,
and their `pair` family puts two targets in different splits at weights
0.67..0.82 / 0.18..0.33, so the combine must weigh two live splits right;
on the CPU they reject a dropped split, out partials exchanged, a combine
that stops after its first group of splits, an unweighted mean, base-2
weights, weights from the neighbouring row, a seam counted twice or not at
all, and a live length rounded to a chunk. The seams come from
needle_cases.split_plan, which mirrors the binding's split heuristic with
TREE_ATTN_SPLIT_BLOCKS unset: the `ext` fixture asserts that it is.

Each query row is gain * K[target], so `out` names the key that was read.
A failure prints the worst row's target key, the nearest seam and the family
(docs/NEEDLE_TESTS.md lists which seams each kernel has).

Guard rows (decoy K, NaN V) are ordinary allocated memory and NaN is data:
nothing here reads or writes out of bounds on purpose.
"""

import os
import subprocess
import sys

import pytest
import torch

import needle_cases as nc

pytestmark = pytest.mark.gpu

KERNEL_ROUTES = ("decode", "decode_fp8", "decode_d64", "decode_narrow",
                 "mx_hw", "spec") + nc.PREFILL_ROUTES


def _params(routes):
    out = []
    for c in nc.CASES:
        if c.route not in routes:
            continue
        for fam in c.families:
            out.append(pytest.param(c, fam, False, id=f"{c.id}-{fam}"))
            if c.guard:
                out.append(pytest.param(c, fam, True,
                                        id=f"{c.id}-{fam}-guarded"))
    return out


@pytest.fixture(scope="module")
def ext():
    from tree_attention_torch_amd.ops import flash

    assert flash.hip_available(), "HIP extension must be built in-tree"
    nc.assert_default_split_plan()
    return flash._load_extension()


@pytest.mark.parametrize("case,family,use_guard", _params(KERNEL_ROUTES))
def test_needle_kernel(ext, monkeypatch, case, family, use_guard):
    monkeypatch.delenv("TREE_ATTN_MX_DECODE", raising=False)
    nd = nc.build(case, family)
    out, lse = nc.run_kernel(nd, use_guard)
    assert torch.isfinite(out).all(), f"{case.id} [{family}]: non-finite out"
    nc.check(nd, out, lse, "guarded" if use_guard else "plain")


@pytest.mark.parametrize("case,family,use_guard", _params(("mx_dequant",)))
def test_needle_mx_dequant(ext, monkeypatch, case, family, use_guard):
    """TREE_ATTN_MX_DECODE=dequant: the bf16-compute MX decode variant (the
    binding reads the flag on every call)."""
    monkeypatch.setenv("TREE_ATTN_MX_DECODE", "dequant")
    nd = nc.build(case, family)
    out, lse = nc.run_kernel(nd)
    assert torch.isfinite(out).all()
    nc.check(nd, out, lse, "dequant")


_CACHE = [c for c in nc.CASES if c.route == "cache"]


@pytest.mark.parametrize("case", _CACHE, ids=[c.id for c in _CACHE])
def test_needle_cache(ext, case):
    """ext.flash_attention_cache: live length from device memory over a
    cache of capacity 1024 (two splits) or 4608 (nine: the trailing ones
    empty by the live length) whose every row at and past the live length
    holds the guard pattern. One row read past the live length is a NaN (or
    a decoy that outscores the needle 4x), not 1/T of extra weight."""
    for fam in case.families:
        nd = nc.build(case, fam)
        out, lse = nc.run_cache(nd)
        assert torch.isfinite(out).all() and torch.isfinite(lse).all(), \
            f"{case.id}: guard rows past live length {case.tkv} leaked"
        nc.check(nd, out, lse, f"cache live={case.tkv}")


def test_needle_cache_graph_replay(ext):
    """DecodeSession.graphed_attend: capture once, replay at live lengths
    511, 512, 513 (around the 512-key split seam) with the guard pattern
    kept behind the live length."""
    from tree_attention_torch_amd.session import DecodeSession

    cases = [next(c for c in _CACHE if c.dtype == "bf16" and c.tkv == n)
             for n in (511, 512, 513)]
    sess = DecodeSession(1, 2, 128, max_tokens=768, device="cuda",
                         kv_dtype="bf16", block=256)
    assert sess.k.shape[2] == nc.CACHE_CAP

    def load(nd):
        kc, vc = nc.cache_buffers(nd)
        sess.k.copy_(kc)
        sess.v.copy_(vc)
        sess.local_len = sess.total = nd.case.tkv
        sess.sync_len()

    nd0 = nc.build(cases[0], "seam")
    load(nd0)
    q_static = nd0.q.cuda().clone()
    replay, _ = sess.graphed_attend(q_static)
    for c in cases:
        nd = nc.build(c, "seam")
        load(nd)
        q_static.copy_(nd.q.cuda())
        out = replay()
        torch.cuda.synchronize()
        assert torch.isfinite(out).all(), f"replay at {c.tkv}: guard leaked"
        nc.check(nd, out, None, f"graph replay live={c.tkv}")


@pytest.mark.parametrize("flag,val", [
    ("TREE_ATTN_PREFILL6", "7"), ("TREE_ATTN_PREFILL6", "0"),
])
def test_needle_prefill_env_variants(ext, flag, val):
    """The env-latched bf16 prefill kernels on the prefill rows of the table
    (every family, plain and guarded). The route flag is latched at first
    call, so each flag gets a fresh child process with its own timeout.
    TREE_ATTN_PREFILL6=7 names the default fa_prefill7_kernel and
    TREE_ATTN_PREFILL6=0 is the fallback fa_prefill2_kernel."""
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    repo = os.path.dirname(tests_dir)
    code = (f"import sys; sys.path.insert(0, {tests_dir!r}); "
            "import needle_cases; needle_cases.run_variant_rows()")
    env = {k: v for k, v in os.environ.items()
           if not k.startswith("TREE_ATTN_PREFILL")}
    env[flag] = val
    env["PYTHONPATH"] = os.pathsep.join(
        p for p in (repo, os.environ.get("PYTHONPATH")) if p)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0 and "NEEDLES_OK" in r.stdout, \
        f"{flag}={val}: exit {r.returncode}\n{r.stdout[-3000:]}\n" \
        f"{r.stderr[-3000:]}"


_REMAP = [pytest.param(c, f, id=f"{c.id}-{f}") for c in nc.remap_cases()
          for f in c.families]


@pytest.mark.parametrize("case,family", _REMAP)
def test_needle_prefill_remap_off(ext, monkeypatch, case, family):
    """TREE_ATTN_REMAP=0: fa_prefill7_kernel's plain block -> (batch, head,
    q-block) decode on the rows that take the XCD remap by default (B*Hq in
    {8, 24}) and on the B*Hq = 12 row. The launcher reads the flag on every
    call."""
    monkeypatch.setenv("TREE_ATTN_REMAP", "0")
    nd = nc.build(case, family)
    out, lse = nc.run_kernel(nd)
    assert torch.isfinite(out).all(), f"{case.id} [{family}]: non-finite out"
    nc.check(nd, out, lse, "TREE_ATTN_REMAP=0")


_SESSION = [c for c in nc.CASES if c.route == "session"]
_SESSIONS = {}


def _filled_session(case):
    """One DecodeSession per (kv dtype, length), shared by its rows and left
    unchanged: the row's K/V stream through prefill() and seven append()s,
    then what the session STORED of it, read back as fp32."""
    from tree_attention_torch_amd.quant import (dequantize_k_mx,
                                                dequantize_v_mx)
    from tree_attention_torch_amd.session import DecodeSession

    key = (case.dtype, case.tkv)
    if key in _SESSIONS:
        return _SESSIONS[key]
    stream = nc.build(case, "seam")
    k, v = stream.k.cuda(), stream.v.cuda()
    sess = DecodeSession(case.b, case.hkv, case.d, max_tokens=768,
                         device="cuda", kv_dtype=case.dtype, block=256)
    n0 = case.tkv - 7
    sess.prefill(k[:, :, :n0], v[:, :, :n0])
    for t in range(n0, case.tkv):
        sess.append(k[:, :, t:t + 1], v[:, :, t:t + 1])
    assert sess.total == sess.local_len == case.tkv
    if case.dtype == "mx":
        n, tail = sess.q_len, sess.tail_len
        assert (n, tail) == (case.tkv // 64 * 64, case.tkv % 64)
        kf = torch.cat([
            dequantize_k_mx(sess.k[:, :, :n].contiguous().cpu(),
                            sess.ks[:, :, :n].contiguous().cpu()),
            sess.k_tail[:, :, :tail].float().cpu()], 2)
        vf = torch.cat([
            dequantize_v_mx(sess.v[:, :, :n].contiguous().cpu(),
                            sess.vs[:, :, :n // 32].contiguous().cpu()),
            sess.v_tail[:, :, :tail].float().cpu()], 2)
    else:
        assert sess.k.shape[2] == nc.CACHE_CAP
        kf = sess.k[:, :, :case.tkv].float().cpu()
        vf = sess.v[:, :, :case.tkv].float().cpu()
    # the stored KV is the stream in the cache's format (e4m3 keeps 3
    # mantissa bits: half a step is 2^-4), batch by batch
    tol = 0.0 if case.dtype == "bf16" else 0.07
    torch.testing.assert_close(kf, stream.k.float(), rtol=tol, atol=tol)
    torch.testing.assert_close(vf, stream.v.float(), rtol=tol, atol=tol)
    _SESSIONS[key] = (sess, kf, vf)
    return _SESSIONS[key]


@pytest.mark.parametrize("case", _SESSION, ids=[c.id for c in _SESSION])
def test_needle_session(ext, monkeypatch, case):
    """DecodeSession(2, 2, 128) at world size 1, kv_dtype bf16 / fp8 / mx,
    576 tokens (MX: nine quantized windows) and 600 (MX: plus a 24-token
    bf16 staging tail): q = gain * K_stored[target], attend(q) and
    attend(q, softmax_scale=0.05) against flash_res_lse over the KV the
    session stored. attend() hands back no lse, so the local partial's lse
    (the only output that shows a scale that was ignored) is compared too."""
    from tree_attention_torch_amd.ops.reference import flash_res_lse
    from tree_attention_torch_amd.parallel.combine import combine_partials

    monkeypatch.delenv("TREE_ATTN_MX_DECODE", raising=False)
    sess, kf, vf = _filled_session(case)
    nd = nc.build_from(case, "seam", None, None, None, kf, vf)
    n = sess.q_len if case.dtype == "mx" else case.tkv
    ref = flash_res_lse(nd.ref_q, kf[:, :, :n], vf[:, :, :n], nd.scale)
    if n < case.tkv:
        # the MX kernel rounds Q to e4m3 (nd.ref_q); the bf16 kernel of the
        # staging tail reads the query as it is
        tail = flash_res_lse(nd.q.float(), kf[:, :, n:], vf[:, :, n:],
                             nd.scale)
        ref = combine_partials(torch.stack([ref[0], tail[0]]),
                               torch.stack([ref[1], tail[1]]))
    q = nd.q.cuda()
    scale_arg = (case.scale,) if case.scale else ()
    out = sess.attend(q, *scale_arg)
    assert torch.isfinite(out).all(), f"{case.id}: non-finite out"
    nc.check(nd, out, None, "attend", ref=ref)
    out_l, lse_l = sess._local_partial(q, *(scale_arg or (None,)))
    nc.check(nd, out_l, lse_l, "local partial", ref=ref)


_SHARDED = [pytest.param(c, f, id=f"{c.id}-{f}") for c in nc.CASES
            if c.cuts for f in c.families]


@pytest.mark.parametrize("case,family", _SHARDED)
def test_needle_ranks_emulated(ext, monkeypatch, case, family):
    """Ranks emulated on one GPU: the KV cut at uneven points that are no
    tile multiples, local_attention(_mx) per shard with the global q_offset
    and that shard's kv_offset, merged by combine_partials. One shard is
    fully masked for some rows and partly masked for others. The merge must
    equal the oracle AND the unsharded kernel call."""
    monkeypatch.delenv("TREE_ATTN_MX_DECODE", raising=False)
    nd = nc.build(case, family)
    (out, lse), (w_out, w_lse) = nc.run_sharded(nd)
    assert torch.isfinite(out).all()
    nc.check(nd, out, lse, f"merged shards {case.cuts}")
    nc.check(nd, w_out, w_lse, "unsharded")
    nc.compare(out, lse, w_out, w_lse, case.kind)
