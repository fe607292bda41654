"""CPU proof that the ragged needle inputs (tests/ragged_cases.py) can see a
wrong per-row length. No GPU: the oracle is run with MUTATED lengths over the
guarded cache and compared with the true answer through the same `compare`
the GPU tests use (tests/test_gpu_ragged.py), at the suite's unchanged bars.
"""

import pytest
import torch

import needle_cases as nc
import ragged_cases as rc

ALL_LENGTHS = rc.LENGTH_SETS + rc.GRAPH_STEPS
MUTANTS = ("L+1", "L-1", "row0_for_all", "max_for_all", "capacity_for_all",
           "row_b^1")


def _mutant(rg, lengths):
    return rc.attend_lengths(
        rg, lengths, lambda q, k, v: nc.oracle(q, k, v))


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("lengths", ALL_LENGTHS, ids=str)
def test_ragged_needles_are_one_hot(lengths, dtype):
    """Every live row's oracle output is its target's V row to <= 0.31 of
    the out bar (the figure the needle suite holds its inputs to), an empty
    row's is 0 / -inf, and the oracle passes its own comparison."""
    rg = rc.build(lengths, dtype)
    assert rg.q.shape == (rc.B, rc.HQ, 1, rc.D)
    assert int(rg.targets[:, 0].max()) == max(lengths) - 1
    kvh = torch.arange(rc.HQ) // rc.G
    worst = 0.0
    for b, n in enumerate(lengths):
        if n == 0:
            assert (rg.targets[b] == -1).all()
            assert not rg.ref_out[b].any()
            assert (rg.ref_lse[b] == float("-inf")).all()
            continue
        assert int(rg.targets[b, 0]) == n - 1
        assert 0 <= int(rg.targets[b].min()) and int(rg.targets[b].max()) < n
        want = rg.v.float()[b, kvh, rg.targets[b]]             # (Hq, D)
        worst = max(worst, float((rg.ref_out[b, :, 0] - want).abs().max()))
        # the guard pattern really is in place
        assert torch.isnan(rg.v_cache[b, :, n:].float()).all()
        assert torch.equal(rg.k_cache[b, :, :n].float(),
                           rg.k[b, :, :n].float())
    assert worst <= 0.31 * nc.BARS[rg.kind][0], worst
    rc.compare(rg, rg.ref_out, rg.ref_lse)
    out64, lse64 = _mutant(rg, lengths)       # fp64 naive == fp32 reference
    torch.testing.assert_close(out64, rg.ref_out, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lse64, rg.ref_lse, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("lengths", rc.LENGTH_SETS, ids=str)
def test_every_length_mutant_is_rejected(lengths, dtype):
    """Every listed length error fails the bars, and so does every single
    batch row whose (clipped) length it changes."""
    rg = rc.build(lengths, dtype)
    muts = rc.mutant_lengths(lengths)
    assert tuple(muts) == MUTANTS
    for name, wrong in muts.items():
        clipped = [max(0, min(n, rc.CAP)) for n in wrong]
        assert clipped != list(lengths), (name, "changes nothing")
        out, lse = _mutant(rg, wrong)
        assert rc.rejected(rg, out, lse), \
            f"{lengths} {dtype}: mutant {name} passes the bars"
        for b in range(rc.B):
            if clipped[b] == lengths[b]:
                continue
            row_ok = not nc.rejected(out[b], lse[b].nan_to_num(neginf=-1e30),
                                     rg.ref_out[b],
                                     rg.ref_lse[b].nan_to_num(neginf=-1e30),
                                     rg.kind)
            assert not row_ok, \
                f"{lengths} {dtype}: mutant {name} passes on row {b}"


def test_stream_round_trips():
    """What a session is fed casts back to the stored bytes."""
    for dtype in rc.DTYPES:
        rg = rc.build(rc.LENGTH_SETS[0], dtype)
        ks, vs = rc.stream(rg)
        assert torch.equal(ks.to(rg.k.dtype).view(torch.uint8),
                           rg.k.view(torch.uint8))
        assert torch.equal(vs.to(rg.v.dtype).view(torch.uint8),
                           rg.v.view(torch.uint8))
