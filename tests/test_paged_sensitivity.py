"""CPU proof that the paged needle inputs (tests/paged_cases.py) can see a
wrong page: the oracle reads the pool through the TRUE table and meets the
suite's bars; each paged-reader mutant, gathered on the CPU and compared
through the same `ragged_cases.compare` the GPU tests use
(tests/test_gpu_paged.py), is rejected."""

import pytest
import torch

import needle_cases as nc
import paged_cases as pc
import ragged_cases as rc

CASES = [pytest.param(n, "seam", id=str(n)) for n in pc.SETS] + \
    [pytest.param(n, "pair", id=f"{n}-pair") for n in rc.LENGTH_SETS_BIG]


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("page", pc.PAGES)
@pytest.mark.parametrize("lengths", pc.SETS, ids=str)
def test_paged_targets(lengths, page, dtype):
    """Head 0 targets L_b - 1; every row long enough targets the first key
    of a page that starts no split chunk; the needles are one-hot to the
    figure the needle suite holds its inputs to."""
    rg = pc.build(lengths, dtype, page)
    kvh = torch.arange(rc.HQ) // rc.G
    worst = 0.0
    for b, n in enumerate(lengths):
        tg = rg.targets[b].tolist()
        if n == 0:
            assert tg == [-1] * rc.HQ
            continue
        assert tg[0] == n - 1 and 0 <= min(tg) and max(tg) < n
        if rg.cap == rc.CAP:
            want = [s for s in pc.PAGE_STARTS[page] if s < n - 1]
        else:   # nine splits, 8 heads: at least 3 of the s * 512 + page
            want = []
            starts = {s + page for s in range(0, n, rc.CHUNK)
                      if s + page < n - 1}
            assert len(starts & set(tg)) >= min(3, len(starts)), (b, tg)
            assert all(t % rc.CHUNK for t in starts)
        assert set(want) <= set(tg), (b, tg)
        v_want = rg.v.float()[b, kvh, rg.targets[b]]
        worst = max(worst, float((rg.ref_out[b, :, 0] - v_want).abs().max()))
    assert worst <= 0.31 * nc.BARS[rg.kind][0], worst
    rc.compare(rg, rg.ref_out, rg.ref_lse)


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("page", pc.PAGES)
@pytest.mark.parametrize("lengths,family", CASES)
def test_pool_layout(lengths, family, page, dtype):
    """The pool is what the module docstring says: a permuted, interleaved
    table; poison everywhere a row owns nothing; guards kept on the last
    live page; and the true reader gives the contiguous cache back."""
    pl = pc.pool(lengths, dtype, page, family)
    rg = pl.rg
    assert pl.k_pool.shape == (pl.n_pages, rc.HKV, page, rc.D)
    assert pl.table.shape == (rc.B, rg.cap // page)
    assert pl.table.dtype == torch.int32
    owned = [p for row in pl.owned for p in row]
    assert len(set(owned)) == len(owned) == pl.n_pages - pc.SPARE
    steps = []
    for b, n in enumerate(lengths):
        live = pc.pages_of(n, page)
        assert pl.table[b, :live].tolist() == pl.owned[b]
        assert (pl.table[b, live:] == pl.poison).all()
        ids = pl.owned[b]
        steps += [y - x for x, y in zip(ids, ids[1:])]
    if len(steps) >= 3:   # consecutive pages: neither adjacent nor ordered
        assert sum(s != 1 for s in steps) > len(steps) // 2
        assert any(s < 0 for s in steps)
    free = sorted(set(range(pl.n_pages)) - set(owned))
    assert pl.poison in free
    assert torch.isnan(pl.v_pool[free].float()).all()
    kc, vc = pc.contiguous(pl)
    for b, n in enumerate(lengths):
        end = pc.pages_of(n, page) * page
        assert torch.equal(kc[b, :, :end].view(torch.uint8),
                           rg.k_cache[b, :, :end].view(torch.uint8))
        assert torch.isnan(vc[b, :, n:].float()).all()


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("page", pc.PAGES)
@pytest.mark.parametrize("lengths,family", CASES)
def test_true_table_meets_the_bars(lengths, family, page, dtype):
    pl = pc.pool(lengths, dtype, page, family)
    out, lse = pc.gather(pl)
    rc.compare(pl.rg, out, lse, f"true table, page {page}")
    torch.testing.assert_close(out, pl.rg.ref_out, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("page", pc.PAGES)
@pytest.mark.parametrize("lengths", pc.SETS, ids=str)
def test_every_paging_mutant_is_rejected(lengths, page, dtype):
    """The table ignored, another row's table, the entry index off by one
    either way, a page id one tile late, the chunk's first id kept, the
    pool indexed (Hkv, n_pages), KV heads swapped inside a page."""
    pl = pc.pool(lengths, dtype, page)
    assert len(pc.MUTANTS) == 8
    for name in pc.MUTANTS:
        out, lse = pc.gather(pl, name)
        assert rc.rejected(pl.rg, out, lse), \
            f"{lengths} {dtype} page {page}: mutant {name} passes the bars"


@pytest.mark.parametrize("lengths", rc.LENGTH_SETS, ids=str)
def test_ragged_targets_alone_miss_a_late_page_id(lengths):
    """Why the page-start targets exist: over ragged_cases' own targets no
    key lies in [256, 384), so a page id one 128-key tile late passes the
    fp8 bars at page 256."""
    pl = pc.scatter(rc.build(lengths, "fp8"), 256)
    rc.compare(pl.rg, *pc.gather(pl))
    assert not rc.rejected(pl.rg, *pc.gather(pl, "pid_lag"))
