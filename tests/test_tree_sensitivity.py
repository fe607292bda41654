"""The draft-tree inputs of tests/tree_cases.py expose every ancestor-mask
error at the unchanged bars, on the CPU: a kernel that passes them has the
masks right. A mutant is exempt from a case only where it shows every query
exactly the keys the true mask shows, which this test computes; no mutant is
exempt everywhere, and every case rejects at least one."""

import itertools

import pytest
import torch

import tree_cases as tc

from tree_attention_torch_amd.session import _tree_masks

PARAMS = [pytest.param(c, id=tc.case_id(c)) for c in tc.CASES]
MUTANTS = ("chain", "self_only", "self+parent", "no_self", "row_b^1", "row/G",
           "no_group_offset", "base+1", "base-1", "global_slot")
SHARD = (1, 3, 4)      # rank, world, block of the host model of a shard


def _same(a, b, cap) -> bool:
    """Whether masks a and b = (base, bits) show every query the same keys."""
    return all(
        tc.canon(int(a[0][i]), int(a[1][i]), cap) ==
        tc.canon(int(b[0][i]), int(b[1][i]), cap)
        for i in itertools.product(*(range(n) for n in a[0].shape)))


def _verdicts(case, dtype) -> dict:
    """mutant -> None where it equals the true mask on this case, else
    whether the bars reject it."""
    tr = tc.build(case, dtype)
    assert torch.isfinite(tr.ref_out).all(), "the oracle read a guard row"
    tc.compare(tr, tr.ref_out, tr.ref_lse, "oracle")
    true = tc.true_masks(tr)
    like = (*true, tr.ref_out, tr.ref_lse)
    verdicts = {}
    for name, mut in tc.mutant_masks(tr).items():
        if _same(mut, true, tr.cap):
            verdicts[name] = None
            continue
        out, lse = tc.attend_masks(tr.q, tr.k_cache, tr.v_cache, *mut,
                                   like=like)
        verdicts[name] = tc.rejected(tr, out, lse)
    # one shard of a sharded sequence: the reference is that shard's partial
    # under its true local masks
    pos = torch.tensor(tc.shard_positions(*SHARD))
    k_l, v_l = tr.k_cache[:, :, pos], tr.v_cache[:, :, pos]
    base, bits = tc.shard_masks(tr, *SHARD)
    true = (tc.per_head(base[:, None].expand(tc.B, tr.t)), tc.per_head(bits))
    gbase, gbits = tc.global_slot_masks(tr, *SHARD)
    mut = (tc.per_head(gbase[:, None].expand(tc.B, tr.t)), tc.per_head(gbits))
    if _same(mut, true, k_l.shape[2]):
        verdicts["global_slot"] = None
    else:
        ref = tc.attend_masks(tr.q, k_l, v_l, *true)
        out, lse = tc.attend_masks(tr.q, k_l, v_l, *mut,
                                   like=(*true, *ref))
        verdicts["global_slot"] = tc.rejected(tr, out, lse, ref)
    assert tuple(verdicts) == MUTANTS
    return verdicts


@pytest.fixture(scope="module")
def verdicts():
    return {(tc.case_id(c), d): _verdicts(c, d)
            for c in tc.CASES for d in tc.DTYPES}


@pytest.mark.parametrize("dtype", tc.DTYPES)
@pytest.mark.parametrize("case", PARAMS)
def test_mutants_are_rejected(verdicts, case, dtype):
    v = verdicts[tc.case_id(case), dtype]
    passed = [name for name, r in v.items() if r is False]
    assert not passed, f"mutants {passed} differ from the tree and pass"
    assert any(r for r in v.values()), "the case rejects no mutant"


@pytest.mark.parametrize("mutant", MUTANTS)
def test_no_mutant_is_exempt_everywhere(verdicts, mutant):
    assert any(v[mutant] for v in verdicts.values())


def test_star_and_two_branch_reject_the_chain_mask(verdicts):
    """What makes the session tests on these cases fail under attend_many's
    mask."""
    for name in ("star", "two_branch"):
        for d in tc.DTYPES:
            assert verdicts[name, d]["chain"] is True


@pytest.mark.parametrize("case", PARAMS)
def test_shard_masks_are_the_session_formula(case):
    """The host model of a shard above is session._tree_masks, the twin of
    kv_append_tree_kernel."""
    tr = tc.build(case, "bf16")
    for rank, world, block in (SHARD, (0, 1, 64), (0, 2, 4), (2, 3, 1)):
        base, bits = tc.shard_masks(tr, rank, world, block)
        for b in range(tc.B):
            got = _tree_masks(tr.starts[b], tr.counts[b], tr.parents[b], tr.t,
                              block, rank, world)
            assert got == (int(base[b]), bits[b].tolist()), (rank, world, b)
    assert torch.equal(tc.shard_masks(tr, 0, 1, 64)[1], tr.bits)


def test_case_table_covers_the_issue():
    assert {c[0] for c in tc.CASES} == {4, 6, 16}
    assert {510, 62, 126, 0} <= {s for c in tc.CASES for s in c[1]}
    assert any(0 in c[2] for c in tc.CASES), "a row with count 0"
    assert any(s == 0 and n == 0 for c in tc.CASES
               for s, n in zip(c[1], c[2])), "an empty row"
    assert any(len(set(c[3])) == tc.B for c in tc.CASES), "a tree per row"
    assert any(c[0] == 16 and tc.depth(c[3][0]) >= 4 for c in tc.CASES)
    assert tc.TWO6 == (-1, 0, 0, 1, 2, 2) and tc.PER_CALL == 4
    # a branch crosses the launch-group boundary
    assert tc.TWO6[4] < tc.PER_CALL <= 4
