"""What the fork tests can see, on the CPU: the scenario of
tests/fork_cases.py run through PoolModel (a paged pool that forks and copies
on write through fork_cases.copy_rows) and read back by paged_cases.gather,
at the bars tests/test_gpu_fork.py uses (ragged_cases.compare). The true
model passes every checkpoint; every mutant fails at least one needle row.

One exception, by construction: a copy of the WHOLE page instead of `rows`
rows only adds bytes past the live length of a page no other row holds, which
no correct reader ever reads. No needle can see it; the byte comparison of the
whole pool, which the kernel test makes, does."""

import pytest
import torch

import fork_cases as fc
import ragged_cases as rc

NEEDLE_COPY_MUTANTS = tuple(m for m in fc.COPY_MUTANTS if m != "whole_page")


def _caught(seen) -> list:
    return [what for what, rg, out, lse in seen if rc.rejected(rg, out, lse)]


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("page", fc.PAGES)
def test_true_model_passes(page, dtype):
    seen = fc.model_checkpoints(page, dtype)
    assert [s[0] for s in seen] == ["step 1", f"step {fc.STEPS}",
                                    "row 0 gone"]
    for what, rg, out, lse in seen:
        rc.compare(rg, out, lse, f"fork model, page {page}, {what}")


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("page", fc.PAGES)
@pytest.mark.parametrize("mutant", NEEDLE_COPY_MUTANTS)
def test_copy_mutant_is_caught(mutant, page, dtype):
    caught = _caught(fc.model_checkpoints(page, dtype, copy_mutant=mutant))
    print(f"{mutant} page {page} {dtype}: caught at {caught}")
    assert caught, f"copy_rows mutant {mutant} passes every checkpoint"


@pytest.mark.parametrize("dtype", rc.DTYPES)
@pytest.mark.parametrize("page", fc.PAGES)
@pytest.mark.parametrize("mutant", fc.SESSION_MUTANTS)
def test_session_mutant_is_caught(mutant, page, dtype):
    caught = _caught(fc.model_checkpoints(page, dtype, session_mutant=mutant))
    print(f"{mutant} page {page} {dtype}: caught at {caught}")
    assert caught, f"session mutant {mutant} passes every checkpoint"


def _pools(dtype, page=128, hkv=2, n_pages=7, d=16):
    g = torch.Generator().manual_seed(5)
    raw = torch.randint(0, 256, (2, n_pages, hkv, page,
                                 d * rc._TD[dtype].itemsize),
                        dtype=torch.uint8, generator=g)
    return raw[0].view(rc._TD[dtype]), raw[1].view(rc._TD[dtype])


@pytest.mark.parametrize("dtype", rc.DTYPES)
def test_copy_rows_model(dtype):
    """copy_rows against index arithmetic written out, and every mutant
    against the byte comparison of the whole pool."""
    triples = [(0, 3, 1), (0, 4, 127), (1, 5, 0), (2, 6, 64)]
    k, v = _pools(dtype)
    want_k, want_v = k.clone(), v.clone()
    for src, dst, rows in triples:
        want_k[dst, :, :rows] = want_k[src, :, :rows]
        want_v[dst, :, :rows] = want_v[src, :, :rows]
    fc.copy_rows(k, v, triples)
    u8 = torch.uint8
    assert torch.equal(k.view(u8), want_k.view(u8))
    assert torch.equal(v.view(u8), want_v.view(u8))
    assert not torch.equal(k.view(u8), _pools(dtype)[0].view(u8))
    for mutant in fc.COPY_MUTANTS:
        km, vm = _pools(dtype)
        fc.copy_rows(km, vm, triples, mutant)
        assert not (torch.equal(km.view(u8), want_k.view(u8))
                    and torch.equal(vm.view(u8), want_v.view(u8))), mutant


@pytest.mark.parametrize("page", fc.PAGES)
def test_whole_page_is_invisible_to_needles(page):
    """The exception of the module docstring, checked: the mutant's bytes
    differ from the true model's, its needle rows do not."""
    true = fc.model_checkpoints(page, "bf16")
    seen = fc.model_checkpoints(page, "bf16", copy_mutant="whole_page")
    assert not _caught(seen)
    for (_, _, out, lse), (_, _, out_t, lse_t) in zip(seen, true):
        assert torch.equal(out, out_t) and torch.equal(lse, lse_t)
