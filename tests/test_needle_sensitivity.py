"""CPU proof that the needle case table (tests/needle_cases.py) can see the
errors it is for. No GPU: an fp64 oracle is MUTATED (mask off by one, key
dropped or admitted, V rows exchanged, head map or row order wrong) and
compared with ops/reference.flash_res_lse through the very `compare` the GPU
tests use (tests/test_gpu_needles.py), at the suite's unchanged bars.

For every row of the shared table:

* the unmutated oracle equals the reference to 1e-5,
* every applicable mutant is REJECTED on at least one family of the row's
  set - a condition, not a measurement: a row that lets one through fails,
* an oracle that emulates the kernel's arithmetic (inputs in the storage
  dtype, P rounded to bf16/fp16/e4m3 before PV, Q rounded to e4m3 for fp8
  and MX) stays INSIDE `compare`, so the bars are reachable.
"""

import pytest
import torch

import needle_cases as nc

CASE_IDS = [c.id for c in nc.CASES]


def _oracle(nd, **kw):
    return nc.oracle(nd.ref_q, nd.ref_k, nd.ref_v, causal=nd.causal,
                     q_offset=nd.q_offset, kv_offset=nd.kv_offset,
                     scale=nd.scale, **kw)


def test_table_covers_the_routes():
    routes = {c.route for c in nc.CASES}
    assert routes == {"decode", "decode_fp8", "decode_d64", "decode_narrow",
                      "mx_hw", "mx_dequant", "spec", "cache",
                      "prefill", "prefill_d64", "prefill_fp8", "prefill_mx",
                      "sharded", "sharded_mx", "session"}
    assert all(c.tkv <= 1024 for c in nc.CASES)
    assert nc.variant_cases(), "the env-variant children need prefill rows"
    # the emulated-rank prefill rows must reach the prefill kernels through
    # local_attention (small head counts would loop the decode kernel)
    from tree_attention_torch_amd.ops.flash import (decode_loop_chunks,
                                                    mx_decode_shaped)
    for c in nc.CASES:
        if c.cuts and c.tq > 16:
            assert decode_loop_chunks(c.tq, c.hq // c.hkv, c.b, c.hq) == 0
            assert not mx_decode_shaped(c.hq, c.hkv, c.tq)
        if c.route == "spec":
            assert decode_loop_chunks(c.tq, c.hq // c.hkv, c.b, c.hq) > 1
        # only B = 1, Hkv = 1 hides the strides of a guarded view
        assert not c.guard or (c.b == 1 and c.hkv == 1)
    assert any(c.route == "spec" and c.b > 1 for c in nc.CASES)
    # every route runs with B > 1 and with a softmax scale of its own
    for route in routes:
        assert any(c.route == route and c.b > 1 for c in nc.CASES), route
        if not route.startswith("sharded"):
            assert any(c.route == route and c.scale for c in nc.CASES), route
    # the gen7/gen9 remap: B*Hq % 8 == 0 with b = 0 only, with one 8-group
    # holding both batches, with an 8-group that straddles two batches
    # (Hq % 8 != 0), and the other branch with B > 1
    for dt in ("bf16", "fp16"):
        bh = {(c.b, c.hq) for c in nc.CASES
              if c.route == "prefill" and c.dtype == dt}
        assert {(1, 8), (2, 4), (2, 12), (3, 4)} <= bh
    assert {(c.b, c.hq) for c in nc.remap_cases()} >= \
        {(1, 8), (2, 4), (2, 12), (3, 4)}


@pytest.mark.parametrize("case", nc.CASES, ids=CASE_IDS)
def test_needles_are_one_hot(case):
    """The construction works: every row's output is its target's V row and
    lse is the target's score (the other keys add < 0.1). first_masked is
    left out: its target is hidden, so the correct answer is diffuse and
    only a kernel that admits the hidden key turns one-hot."""
    for fam in (f for f in case.families if f != "first_masked"):
        nd = nc.build(case, fam)
        out, lse = nc.reference(case, fam)
        assert nd.targets.shape == (case.b, case.hq, case.tq)
        assert nd.scale == case.softmax_scale
        want = nc.take_rows(nd.ref_v, case, nd.targets)
        tscore = (nd.ref_q * nc.take_rows(nd.ref_k, case, nd.targets)
                  ).sum(-1) * nd.scale
        # D=32 needles score 11.3 against ~1000 keys of N(0, 2): still > 90 %
        tol = 0.05 if case.d >= 64 else 0.6
        assert (out - want).abs().max() < tol, (case.id, fam)
        assert ((lse - tscore) >= -1e-4).all() and \
            (lse - tscore).max() < (0.1 if case.d >= 64 else 0.5)


@pytest.mark.parametrize("case", nc.CASES, ids=CASE_IDS)
def test_oracle_equals_reference(case):
    for fam in case.families:
        nd = nc.build(case, fam)
        out, lse = _oracle(nd)
        ref_out, ref_lse = nc.reference(case, fam)
        torch.testing.assert_close(out.float(), ref_out, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(lse.float(), ref_lse, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("case", nc.CASES, ids=CASE_IDS)
def test_every_mutant_is_rejected(case):
    muts = nc.mutants(case)
    assert muts, f"{case.id}: no mutant applies, the row proves nothing"
    through = []
    for mut in muts:
        caught = False
        for fam in case.families:
            nd = nc.build(case, fam)
            guard = nc.guard_rows(nd, 1) if mut == "past_end" else None
            out, lse = _oracle(nd, mutant=mut, guard=guard)
            if nc.rejected(out, lse, *nc.reference(case, fam), case.kind):
                caught = True
                break
        if not caught:
            through.append(mut)
    assert not through, f"{case.id}: mutants pass the bars: {through}"


@pytest.mark.parametrize("case", nc.CASES, ids=CASE_IDS)
def test_emulated_kernel_is_inside_the_bars(case):
    for fam in case.families:
        nd = nc.build(case, fam)
        out, lse = _oracle(nd, p_round=nc.emulation_p_round(case),
                           q_round=nc.emulation_q_round(case))
        nc.compare(out, lse, *nc.reference(case, fam), case.kind)
        if case.kind == "fp8":
            # the fp8 kernels cast Q to e4m3: every query is exact there,
            # so the reference (which reads nd.q) sees what the kernel sees
            assert torch.equal(nc._e4m3(nd.q), nd.q.float()), (case.id, fam)


@pytest.mark.parametrize(
    "case", [c for c in nc.CASES if c.cuts],
    ids=[c.id for c in nc.CASES if c.cuts])
def test_oracle_sharded_equals_unsharded(case):
    """The property the emulated-rank GPU tests rely on, in fp64: per-shard
    partials (global q_offset, the shard's kv_offset) merged by
    combine_partials equal attention over the whole KV, with uneven cuts and
    a shard that is fully masked for some rows and partly for others."""
    from tree_attention_torch_amd.parallel.combine import combine_partials

    for fam in case.families:
        nd = nc.build(case, fam)
        outs, lses, kinds = [], [], set()
        for lo, hi in zip(case.cuts[:-1], case.cuts[1:]):
            o, l = nc.oracle(nd.ref_q, nd.ref_k[:, :, lo:hi],
                             nd.ref_v[:, :, lo:hi], causal=nd.causal,
                             q_offset=nd.q_offset, kv_offset=lo,
                             scale=nd.scale)
            outs.append(o)
            lses.append(l)
            if nd.causal:
                masked = torch.isinf(l)
                kinds.add("mixed" if masked.any() and not masked.all()
                          else "uniform")
        out, lse = combine_partials(torch.stack(outs), torch.stack(lses))
        whole_o, whole_l = _oracle(nd)
        torch.testing.assert_close(out, whole_o.float(), rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(lse, whole_l.float(), rtol=1e-5, atol=1e-5)
        if nd.causal and case.tq > 1:   # one position cannot be both
            assert "mixed" in kinds, "no shard masks some rows and not others"


def test_guarded_view_passes_for_contiguous():
    nd = nc.build(next(c for c in nc.CASES if c.guard and c.tkv == 65), "seam")
    gk, gv = nc.guard_rows(nd, nc.GUARD_PRE + nc.GUARD_POST)
    k = nc.guarded(nd.k, 65, nc.GUARD_PRE, nc.GUARD_POST, gk)
    v = nc.guarded(nd.v, 65, nc.GUARD_PRE, nc.GUARD_POST, gv)
    assert k.is_contiguous() and v.is_contiguous()
    assert torch.equal(k, nd.k) and torch.equal(v, nd.v)
    # the rows around the view: NaN V, decoy K scoring ~4x the needle
    base = v.as_strided((nc.GUARD_PRE + 65 + nc.GUARD_POST, 128), (128, 1),
                        v.storage_offset() - nc.GUARD_PRE * 128)
    assert torch.isnan(base[: nc.GUARD_PRE].float()).all()
    assert torch.isnan(base[nc.GUARD_PRE + 65:].float()).all()
    kb = k.as_strided((1, 128), (128, 1), k.storage_offset() + 65 * 128)
    s = (nd.q.float()[0, 0, 0] * kb.float()[0]).sum() * nd.scale
    assert s > 60
