"""The shared-prefix inputs (tests/shared_cases.py) expose what the two passes
can get wrong. CPU only: the passes are the plain-torch model of the helper,
the bars are the suite's unchanged ones.

Two comparisons run on the GPU as well: the binding returns (out, lse), the
session returns `out` alone. Every mutant must be visible to at least one of
them; which one is stated in shared_cases.LSE_ONLY and asserted here."""

import math

import pytest
import torch

import shared_cases as sc

CASES = [(layout, page, dtype) for layout in sc.LAYOUTS for page in sc.PAGES
         for dtype in sc.DTYPES]


@pytest.mark.parametrize("layout,page,dtype", CASES)
@pytest.mark.parametrize("n", sc.CHECKPOINTS)
def test_model_passes(layout, page, dtype, n):
    cs = sc.at(layout, page, dtype, n)
    assert cs.plan == sc.EXPECT[page]
    sc.one_group_each(cs.plan, sc.B)
    out, lse = sc.model(cs)
    sc.compare(cs, out, lse, f"{layout} n={n}")


@pytest.mark.parametrize("page", sc.PAGES)
def test_needles_cover_the_edges(page):
    """Key 0, both sides of the split seam, both sides of the prefix boundary
    and the last key are all somebody's target, and no two members of a group
    share a target on a head."""
    for n in (1, sc.STEPS):
        cs = sc.at("fork", page, "bf16", n)
        want = {"key0", "seam-1", "seam", "P-1", "P", "last"}
        assert sc.coverage(cs) >= want, sc.coverage(cs)
        for rows, _ in cs.plan:
            for h in range(sc.HQ):
                tg = [int(cs.targets[b, h]) for b in rows
                      if cs.lengths[b] > 0]
                assert len(set(tg)) == len(tg), (rows, h, tg)


@pytest.mark.parametrize("page", sc.PAGES)
def test_empty_suffix_row(page):
    """Before its first append row 2 ends on the prefix boundary: its suffix
    partial is empty and its output is the prefix partial alone."""
    cs = sc.at("fork", page, "bf16", 0)
    _, _, _, start = cs.tables()
    assert cs.lengths[2] == 640
    if page == 128:
        assert int(start[2]) == cs.lengths[2]
    out, lse = sc.model(cs)
    sc.compare(cs, out, lse)


@pytest.mark.parametrize("page", sc.PAGES)
@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("mutant", sc.MUTANTS)
def test_mutant_rejected(page, dtype, mutant):
    """At (out, lse) level every mutant is rejected after the first step; with
    `out` alone, all but the ones that only count keys twice. Those move lse
    by ln 2 = 0.69: the bf16 / fp16 lse bar (1e-3 relative and absolute, 0.03
    at an lse of 25) sees that, the fp8 bar (5e-2, 1.3 there) does not."""
    cs = sc.at("fork", page, dtype, 1)
    out, lse = sc.model(cs, mutant)
    seen = sc.rejected(cs, out, lse)
    assert seen == (mutant not in sc.LSE_ONLY or cs.kind == "half"), \
        f"{mutant}: (out, lse) level {'sees' if seen else 'misses'} it"
    out_sees = sc.rejected(cs, out, None)
    assert out_sees == (mutant not in sc.LSE_ONLY), \
        f"{mutant}: the out-only comparison {'sees' if out_sees else 'misses'} it"


@pytest.mark.parametrize("page", sc.PAGES)
def test_double_count_is_ln2_on_lse(page):
    """Keys counted twice leave `out` alone and add ln 2 to the lse of a row
    whose needle is among them."""
    cs = sc.at("fork", page, "bf16", 1)
    ok_out, ok_lse = sc.model(cs)
    out, lse = sc.model(cs, "start-1page")
    # (the needle leads every other key by ~16 nats: doubling some of the
    # others moves `out` by their weight, e^-16 of O(1) values, at the most)
    torch.testing.assert_close(out, ok_out, rtol=1e-3, atol=1e-3)
    prefix = cs.plan[0][1]
    hit = 0
    for b in cs.plan[0][0]:
        for h in range(sc.HQ):
            if prefix - page <= int(cs.targets[b, h]) < prefix:
                d = float(lse[b, h, 0] - ok_lse[b, h, 0])
                assert abs(d - math.log(2.0)) < 1e-3, (b, h, d)
                hit += 1
    assert hit, "no needle in the doubled page"


def test_every_mutant_is_seen_on_the_gpu():
    """The GPU suite compares (out, lse) at the binding, for bf16, fp16 and
    fp8 pools, and `out` at the session: together they see every mutant, the
    double count through the bf16 / fp16 binding comparison alone."""
    half_binding_sees = set(sc.MUTANTS)
    fp8_binding_sees = session_sees = set(sc.MUTANTS) - set(sc.LSE_ONLY)
    assert half_binding_sees | fp8_binding_sees | session_sees \
        == set(sc.MUTANTS)
    for page in sc.PAGES:
        cs = sc.at("fork", page, "bf16", 1)
        for mutant in sc.LSE_ONLY:
            assert sc.rejected(cs, *sc.model(cs, mutant))
