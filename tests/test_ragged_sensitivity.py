"""CPU proof that the ragged needle inputs (tests/ragged_cases.py) can see a
wrong per-row length. No GPU: the oracle is run with MUTATED lengths over the
guarded cache and compared with the true answer through the same `compare`
the GPU tests use (tests/test_gpu_ragged.py), at the suite's unchanged bars.
"""

import pytest
import torch

import needle_cases as nc
import ragged_cases as rc

SETS = rc.LENGTH_SETS + rc.LENGTH_SETS_BIG
ALL_LENGTHS = SETS + rc.GRAPH_STEPS
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
@pytest.mark.parametrize("lengths", SETS, ids=str)
def test_every_length_mutant_is_rejected(lengths, dtype):
    """Every listed length error fails the bars, and so does every single
    batch row whose (clipped) length it changes."""
    rg = rc.build(lengths, dtype)
    muts = rc.mutant_lengths(lengths)
    assert tuple(muts) == MUTANTS
    muts.update(rc.chunk_mutant_lengths(lengths))   # len_rounds_to_chunk
    assert len(muts) == len(MUTANTS) + 2
    for name, wrong in muts.items():
        clipped = [max(0, min(n, rg.cap)) for n in wrong]
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


def _row_partials(rg, b, **emu):
    """fp64 partials of batch row b over the splits of its cache's plan:
    (S, 1, Hq, 1, D), (S, 1, Hq, 1); a split past the row's length is
    empty."""
    s_all, chunk = nc.split_plan(rc.B, rc.HKV, rg.cap)
    assert chunk == rc.CHUNK
    n, outs, lses = rg.lengths[b], [], []
    for s in range(s_all):
        lo, hi = s * chunk, max(s * chunk, min((s + 1) * chunk, n))
        o, l = nc.oracle(rg.q[b:b + 1].float(),
                         rg.k_cache[b:b + 1, :, lo:hi].float(),
                         rg.v_cache[b:b + 1, :, lo:hi].float(), **emu)
        outs.append(o)
        lses.append(l)
    return torch.stack(outs), torch.stack(lses)


def _seam_mutants(rg, b, o, l):
    """seam_twice(s) / seam_skipped(s) of row b for every split s whose
    first key a head targets: the first 128 keys of split s also counted in
    split s - 1, or in neither."""
    n, muts = rg.lengths[b], {}
    for s in sorted({int(t) // rc.CHUNK for t in rg.targets[b]
                     if int(t) % rc.CHUNK == 0}):
        lo, hi = s * rc.CHUNK, min((s + 1) * rc.CHUNK, n)
        mid = min(lo + nc.SEAM_KEYS, hi)
        q, kc, vc = rg.q[b:b + 1].float(), rg.k_cache[b:b + 1].float(), \
            rg.v_cache[b:b + 1].float()
        head = nc.oracle(q, kc[:, :, lo:mid], vc[:, :, lo:mid])
        rest = nc.oracle(q, kc[:, :, mid:hi], vc[:, :, mid:hi])
        so, sl = o.clone(), l.clone()
        so[s], sl[s] = rest
        muts[f"seam_skipped({s})"] = nc.merge_partials(so, sl)
        if s:
            to, tl = o.clone(), l.clone()
            to[s - 1], tl[s - 1] = nc.merge_partials(
                torch.stack([o[s - 1], head[0]]),
                torch.stack([l[s - 1], head[1]]))
            muts[f"seam_twice({s})"] = nc.merge_partials(to, tl)
    return muts


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("lengths", rc.LENGTH_SETS_BIG, ids=str)
def test_ragged_split_mutants_are_rejected(lengths, dtype):
    """The nine-split capacity, row by row: the fp64 split oracle equals the
    reference to 1e-5; dropping any split that holds a target, exchanging
    its out partial with the next live split's, an unweighted mean and a
    combine that stops after its first group of 4 splits are rejected at
    the bars of the kind."""
    rg = rc.build(lengths, dtype)
    assert rg.cap == rc.CAP_BIG
    first_group_seen = False
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        ref = (rg.ref_out[b:b + 1], rg.ref_lse[b:b + 1])
        o, l = _row_partials(rg, b)
        out, lse = nc.merge_partials(o, l)
        torch.testing.assert_close(out.float(), ref[0], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(lse.float(), ref[1], rtol=1e-5, atol=1e-5)
        live = -(-n // rc.CHUNK)
        assert not torch.isfinite(l[live:]).any() and \
            torch.isfinite(l[:live]).all()
        hit = sorted({int(t) // rc.CHUNK for t in rg.targets[b]})
        assert len(hit) >= min(live, rc.HQ - 1)
        muts = {}
        for s in hit:
            keep = [i for i in range(o.shape[0]) if i != s]
            muts[f"split_drop({s})"] = nc.merge_partials(o[keep], l[keep])
            if live > 1:
                idx = list(range(o.shape[0]))
                t = (s + 1) % live
                idx[s], idx[t] = t, s
                muts[f"split_oswap({s},{t})"] = nc.merge_partials(o[idx], l)
        if live > 1:
            w = torch.isfinite(l).double()
            muts["combine_mean"] = ((o * w.unsqueeze(-1)).sum(0) / w.sum(0)
                                    .unsqueeze(-1), lse)
        if live > 4:
            muts["combine_first_group"] = nc.merge_partials(o[:4], l[:4])
            first_group_seen = True
        # a one-hot key counted twice adds ln 2 to lse and leaves out alone:
        # inside the fp8 lse bar, so fp8 sees seam_twice on its pair rows
        muts.update({k: m for k, m in _seam_mutants(rg, b, o, l).items()
                     if dtype == "bf16" or k.startswith("seam_skipped")})
        for name, (mo, ml) in muts.items():
            assert nc.rejected(mo, ml, *ref, rg.kind), \
                f"{lengths} {dtype} row {b}: {name} passes the bars"
    assert first_group_seen


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("lengths", rc.LENGTH_SETS_BIG, ids=str)
def test_ragged_pair_rows(lengths, dtype):
    """The pair family of the nine-split capacity: two targets in different
    splits, the minor weight >= 0.15, both together >= 0.99, an fp8 query
    exact in e4m3; the split oracle equals the reference, stays inside the
    bars with P rounded per split, and base-2 weights (final lse right) are
    rejected on every paired row."""
    rg = rc.build(lengths, dtype, "pair")
    seam = rc.build(lengths, dtype)
    paired = [b for b in range(rc.B) if (rg.targets2[b] >= 0).any()]
    assert paired == [b for b, n in enumerate(lengths) if n > 2 * rc.CHUNK]
    assert len(paired) >= 2
    kvh = torch.arange(rc.HQ) // rc.G
    if dtype == "fp8":
        assert torch.equal(nc._e4m3(rg.q), rg.q.float())
    for b, n in enumerate(lengths):
        if b not in paired:   # one-hot query, as in the seam family
            assert torch.equal(rg.q[b], seam.q[b])
            continue
        t1, t2 = rg.targets[b], rg.targets2[b]
        assert (t1 // rc.CHUNK != t2 // rc.CHUNK).all() and int(t2.max()) < n
        kb = rg.k[b].double()
        qb = rg.q[b, :, 0].double()
        w = [torch.exp((qb * kb[kvh, t]).sum(-1) / rc.D ** 0.5
                       - rg.ref_lse[b, :, 0].double()) for t in (t1, t2)]
        assert float(torch.minimum(*w).min()) >= 0.15
        assert float((w[0] + w[1]).min()) >= 0.99
        ref = (rg.ref_out[b:b + 1], rg.ref_lse[b:b + 1])
        o, l = _row_partials(rg, b)
        out, lse = nc.merge_partials(o, l)
        torch.testing.assert_close(out.float(), ref[0], rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(lse.float(), ref[1], rtol=1e-5, atol=1e-5)
        emu = _row_partials(rg, b, p_round="e4m3" if dtype == "fp8"
                            else "bf16",
                            q_round="e4m3" if dtype == "fp8" else None)
        nc.compare(*nc.merge_partials(*emu), *ref, rg.kind)
        m = l.amax(0)
        w2 = torch.exp2(l - m)
        base2 = (o * w2.unsqueeze(-1)).sum(0) / w2.sum(0).unsqueeze(-1)
        assert nc.rejected(base2, lse, *ref, rg.kind), \
            f"{lengths} {dtype} row {b}: weight_base2 passes the bars"
        twice = {k: m for k, m in _seam_mutants(rg, b, o, l).items()
                 if k.startswith("seam_twice")}
        assert len(twice) >= 4
        for name, (mo, ml) in twice.items():
            assert nc.rejected(mo, ml, *ref, rg.kind), \
                f"{lengths} {dtype} row {b}: {name} passes the bars"
        # ... and the seam family alone does not see base-2 weights
        so, sl = _row_partials(seam, b)
        sw = torch.exp2(sl - sl.amax(0))
        s2 = (so * sw.unsqueeze(-1)).sum(0) / sw.sum(0).unsqueeze(-1)
        assert not nc.rejected(s2, nc.merge_partials(so, sl)[1],
                               seam.ref_out[b:b + 1], seam.ref_lse[b:b + 1],
                               seam.kind)


def test_stream_round_trips():
    """What a session is fed casts back to the stored bytes."""
    for dtype in rc.DTYPES:
        rg = rc.build(rc.LENGTH_SETS[0], dtype)
        ks, vs = rc.stream(rg)
        assert torch.equal(ks.to(rg.k.dtype).view(torch.uint8),
                           rg.k.view(torch.uint8))
        assert torch.equal(vs.to(rg.v.dtype).view(torch.uint8),
                           rg.v.view(torch.uint8))
