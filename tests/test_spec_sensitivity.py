"""The speculative-verify inputs of tests/spec_cases.py expose every limit
error at the unchanged bars, on the CPU: a kernel that passes them has the
per-query-row visible lengths right. And n_local, the one formula append and
attention share, equals a brute-force count over _place."""

import pytest
import torch

import spec_cases as sc

from tree_attention_torch_amd.session import _n_local, _place

PARAMS = [pytest.param(c, id=sc.case_id(c)) for c in sc.CASES]


@pytest.mark.parametrize("dtype", sc.DTYPES)
@pytest.mark.parametrize("case", PARAMS)
def test_oracle_meets_itself_and_mutants_are_rejected(case, dtype):
    sp = sc.build(case, dtype)
    assert torch.isfinite(sp.ref_out).all(), "the oracle read a guard row"
    sc.compare(sp, sp.ref_out, sp.ref_lse, "oracle")
    muts = sc.mutant_limits(sp)
    assert set(muts) == {"vis+1", "vis-1", "no_causal", "row/G", "row_b^1",
                         "chunk_down", "chunk_up"}
    for name, lim in muts.items():   # no case is exempt from any mutant
        out, lse = sc.attend_limits(sp, lim)
        assert sc.rejected(sp, out, lse), \
            f"{sc.case_id(case)} {dtype}: mutant {name} passes the bars"


@pytest.mark.parametrize("case", PARAMS)
def test_cases_cover_the_seams(case):
    """Each case holds a row whose drafts straddle 511 | 512, a row with
    more than one draft, and limits that differ inside a row."""
    t, starts, counts = case
    assert any(s < 512 <= s + c - 1 for s, c in zip(starts, counts))
    assert max(counts) >= 2 and len(set(counts)) >= 1
    vis = sc.vis_of(t, starts, counts)
    assert any(len(set(row.tolist())) > 1 for row in vis)


def test_case_table_covers_the_issue():
    ts = {c[0] for c in sc.CASES}
    assert ts == {3, 4, 6}
    starts = {s for c in sc.CASES for s in c[1]}
    assert {510, 62, 126, 0} <= starts
    assert any(len(set(c[2])) > 1 for c in sc.CASES), "unequal counts"
    assert any(0 in c[2] for c in sc.CASES), "a row with count 0"


@pytest.mark.parametrize("world", [1, 2, 3, 4])
@pytest.mark.parametrize("block", [4, 64, 256])
def test_n_local_is_the_count_place_implies(world, block):
    t_max = 3 * world * block + 5
    owned = [0] * world
    for t in range(t_max + 1):
        for r in range(world):
            assert _n_local(t, block, r, world) == owned[r], (t, r)
        owner, pos = _place(t, block, world)
        # contiguous appends: the token lands at the end of its shard
        assert pos == owned[owner], (t, owner)
        owned[owner] += 1
