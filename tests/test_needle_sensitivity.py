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
MANY = nc.many_split_cases()
MANY_IDS = [c.id for c in MANY]


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
    # the 40000-key rows (63 splits of 640) are the only ones above 8193
    assert {c.tkv for c in nc.CASES if c.tkv > 8193} == {40000}
    assert sum(c.tkv == 40000 for c in nc.CASES) == 2
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
    for fam in (f for f in case.families
                if f not in ("first_masked", "pair")):
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
        emu = dict(p_round=nc.emulation_p_round(case),
                   q_round=nc.emulation_q_round(case))
        # a many-split row rounds P per split, as the kernels do: a `pair`
        # row is one-hot inside each of its two splits
        out, lse = nc.split_oracle(nd, **emu) if case in MANY \
            else _oracle(nd, **emu)
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
        # one position cannot be both; nor can a frontier that crosses no cut
        # (the two 5-split shards: its frontier lies inside the second)
        crosses = any(case.qoff < c <= case.qoff + case.tq - 1
                      for c in case.cuts[1:-1])
        if nd.causal and case.tq > 1 and crosses:
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


# --------------------------------------------------------------------------
# many splits: the split plan, needles in every split, the pair family and
# the split / combine mutants
# --------------------------------------------------------------------------
# (S, chunk) read from pick_splits / plan_splits of ops/hip/bindings.cpp on
# 2026-10-21, by hand; it holds for (B, Hkv) = (1, 1), (2, 2) and (3, 3).
SPLIT_PLAN_TABLE = {
    1: (1, 128), 63: (1, 128), 64: (1, 128), 65: (1, 128), 127: (1, 128),
    128: (1, 128), 129: (1, 256), 511: (1, 512), 512: (1, 512),
    513: (2, 384), 576: (2, 384), 600: (2, 384), 1000: (2, 512),
    1023: (2, 512), 1024: (2, 512),
    1100: (3, 384), 1537: (4, 512), 2049: (5, 512), 2100: (5, 512),
    3000: (6, 512), 4097: (9, 512), 4608: (9, 512), 8193: (17, 512),
    40000: (63, 640),
}
SPLIT_TAILS = {1537: 1, 2049: 1, 4097: 1, 8193: 1, 40000: 320}


def test_split_plan_is_pinned():
    for tkv, want in SPLIT_PLAN_TABLE.items():
        for b, hkv in ((1, 1), (2, 2), (3, 3)):
            assert nc.split_plan(b, hkv, tkv) == want, (b, hkv, tkv)
        s, chunk = want
        assert chunk % 128 == 0 and (s - 1) * chunk < tkv <= s * chunk
        if tkv in SPLIT_TAILS:
            assert tkv - (s - 1) * chunk == SPLIT_TAILS[tkv]
    # a grid target that B*Hkv fills caps the split count below max_s:
    # 512 / 256 = 2 splits of 2048 keys, ceil(768 / 300) = 3 of 1408
    assert nc.split_plan(64, 4, 4097) == (2, 2176)
    assert nc.split_plan(100, 3, 4097) == (3, 1408)
    # every length the many-split rows use is in the table
    lengths = {c.capacity if c.route == "cache" else c.tkv for c in MANY}
    assert lengths <= set(SPLIT_PLAN_TABLE) | {2112, 2560, 4160}
    assert nc.split_plan(1, 2, 2112) == (5, 512)
    assert nc.split_plan(1, 2, 2560) == (5, 512)
    assert nc.split_plan(1, 2, 4160) == (9, 512)


def test_many_split_rows_cover_the_issue():
    """The (route, S) pairs the combine loop needs: S = NG + 1 and 2 NG + 1
    for both NG, a ragged and a full last split, 63 splits of 640, trailing
    splits emptied by a live length below and at or above NG."""
    got = {(c.route, c.plan[0], c.dtype) for c in MANY}
    for want in (("decode", 3, "bf16"), ("decode", 5, "bf16"),
                 ("decode", 9, "bf16"), ("decode", 5, "fp16"),
                 ("decode", 63, "bf16"), ("decode_fp8", 5, "fp8"),
                 ("decode_fp8", 9, "fp8"), ("decode_fp8", 63, "fp8"),
                 ("decode_d64", 9, "bf16"), ("decode_d64", 17, "bf16"),
                 ("decode_d64", 9, "fp16"), ("decode_narrow", 5, "bf16"),
                 ("decode_narrow", 9, "bf16"), ("mx_hw", 5, "mx"),
                 ("mx_hw", 9, "mx"), ("mx_dequant", 5, "mx"),
                 ("mx_dequant", 9, "mx"), ("spec", 5, "bf16"),
                 ("cache", 9, "bf16"), ("cache", 9, "fp8")):
        assert want in got, want
    assert {c.d for c in MANY if c.route == "decode_narrow"} == {80, 96, 112}
    assert {c.d for c in nc.CASES if c.route == "decode_narrow"} == \
        {32, 48, 80, 96, 112}
    for dt in ("bf16", "fp8"):
        live = {c.live_splits for c in MANY
                if c.route == "cache" and c.dtype == dt}
        ng = 4
        assert any(n < ng for n in live) and any(ng <= n < 9 for n in live) \
            and 9 in live
    assert any(c.cuts == (0, 2049, 4150) for c in nc.CASES)


@pytest.mark.parametrize("case", MANY, ids=MANY_IDS)
def test_every_split_and_seam_is_targeted(case):
    """Every split that holds live keys holds the target of a query row, and
    both sides of every split seam are targets. Only a row with fewer than
    2 S rows may leave seams out, and says so in its note."""
    chunk, s_live = case.plan[1], case.live_splits
    tg = set(nc.family_targets(case, "seam").flatten().tolist())
    assert {t // chunk for t in tg} == set(range(s_live)), case.id
    seams = range(chunk, case.tkv, chunk)
    open_seams = [s for s in seams if not {s - 1, s} <= tg]
    if case.b * case.hq * case.tq >= 2 * s_live:
        assert not open_seams, (case.id, open_seams)
    else:
        assert case.note and len(open_seams) <= len(seams) // 2, case.id


@pytest.mark.parametrize("case", MANY, ids=MANY_IDS)
def test_split_oracle_equals_reference(case):
    for fam in case.families:
        nd = nc.build(case, fam)
        out, lse = nc.split_oracle(nd)
        ref_out, ref_lse = nc.reference(case, fam)
        torch.testing.assert_close(out.float(), ref_out, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(lse.float(), ref_lse, rtol=1e-5, atol=1e-5)


_PAIR = [c for c in nc.CASES if "pair" in c.families]


@pytest.mark.parametrize("case", _PAIR, ids=[c.id for c in _PAIR])
def test_pair_rows_weigh_two_splits(case):
    """Every row of the pair family: two targets in different splits, the
    minor one at a weight of at least 0.15, both together at least 0.99;
    for the e4m3-Q kinds the query is exact in e4m3."""
    nd = nc.build(case, "pair")
    chunk = case.plan[1]
    assert (nd.targets // chunk != nd.targets2 // chunk).all()
    assert int(nd.targets2.max()) < case.tkv
    _, lse = nc.oracle(nd.ref_q, nd.ref_k, nd.ref_v, scale=nd.scale)
    w = []
    for tg in (nd.targets, nd.targets2):
        sc = (nd.ref_q.double() * nc.take_rows(nd.ref_k, case, tg).double()
              ).sum(-1) * nd.scale
        w.append(torch.exp(sc - lse))
    minor, total = torch.minimum(*w), w[0] + w[1]
    assert float(minor.min()) >= 0.15, (case.id, float(minor.min()))
    assert float(total.min()) >= 0.99, (case.id, float(total.min()))
    if case.kind != "half":
        assert torch.equal(nc._e4m3(nd.q), nd.q.float()), case.id
    # every live split is some row's first or second target
    hit = set((nd.targets // chunk).flatten().tolist()) | \
        set((nd.targets2 // chunk).flatten().tolist())
    assert hit == set(range(case.live_splits))


@pytest.mark.parametrize("case", MANY, ids=MANY_IDS)
def test_every_split_mutant_is_rejected(case):
    muts = nc.split_mutants(case)
    names = {m if isinstance(m, str) else m[0] for m in muts}
    assert {"split_drop", "seam_skipped"} <= names
    if case.live_splits > 1:
        assert {"split_oswap", "combine_mean", "lse_row_shift"} <= names
        # ln 2 of lse is inside the e4m3-P kinds' lse bars: see split_mutants
        assert "seam_twice" in names or (
            case.kind in ("fp8", "mx_hw") and "pair" not in case.families)
    if "pair" in case.families:
        assert "weight_base2" in names
    if case.live_splits > case.combine_groups:
        assert "combine_first_group" in names
    parts = {}
    through = []
    for mut in muts:
        caught = False
        for fam in case.families:
            nd = nc.build(case, fam)
            if fam not in parts:
                parts[fam] = nc.split_parts(nd)
            out, lse = nc.split_mutant(nd, parts[fam], mut)
            if nc.rejected(out, lse, *nc.reference(case, fam), case.kind):
                caught = True
                break
        if not caught:
            through.append(mut)
    assert not through, f"{case.id}: split mutants pass the bars: {through}"
