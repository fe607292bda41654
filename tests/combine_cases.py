"""Inputs for the combine kernels and their fp64 reference.

One set of partials (outs (S, rows, D), lses (S, rows), fp32) per content;
the reference is the combine formula evaluated in fp64 on the CPU and
rounded to fp32. The GPU tests (tests/test_gpu_combine.py) run the three HIP
combine kernels on them, the CPU tests (tests/test_combine.py) run
combine_partials and the eager twin of the all-reduce path.

This module is a plain helper (not a conftest).
"""

from __future__ import annotations

import math

import torch

import needle_cases as nc

SEED = 20261022
SPLITS = (1, 2, 4, 5, 8, 9, 17, 64)        # fa_combine_kernel: NG = 4 or 8
WORLDS = (2, 3, 8)
ROWS = (1, 3 * 5 * 7, 2 * 8 * 4)
# the existing bar of the combine tests, applied to the fp64 reference
# rounded to fp32
RTOL = ATOL = 1e-5
NEG_INF = float("-inf")


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(SEED + sum(
        int(k) * 1009 ** i for i, k in enumerate(key)))


def contents(s: int, rows: int, d: int, ng: int = 0):
    """(name, outs, lses, exact) for every content that exists at S = s.
    `exact`: the result is compared by equality, not at the bar. ng > 0 adds
    the two-live-splits content at positions (ng - 1, ng) when s > ng."""
    g = _gen(s, rows, d)
    r = torch.arange(rows)
    outs = torch.randn(s, rows, d, generator=g)

    def fresh():
        return torch.full((s, rows), NEG_INF)

    # (a) generic: randn lse times 4, a masked split that rotates over rows
    lses = torch.randn(s, rows, generator=g) * 4
    if s > 1:
        lses[r % s, r] = NEG_INF
    yield "generic", outs, lses, False
    # (b) hot-late: the last split at +300, the rest about -300. A max taken
    #     over the first splits only overflows exp(600)
    lses = torch.randn(s, rows, generator=g) - 300.0
    lses[s - 1] = 300.0
    yield "hot_late", outs, lses, False
    # (c) one-finite: only split p is finite, for every p in turn
    for p in range(s):
        lses = fresh()
        lses[p] = torch.randn(rows, generator=g) * 4
        yield f"one_finite_{p}", outs, lses, True
    # (d) all masked
    yield "all_masked", outs, fresh(), True
    # (e) two live splits at weights 0.7 / 0.3
    pairs = [(0, s - 1)] if s > 1 else []
    if ng and s > ng:
        pairs.append((ng - 1, ng))
    for a, b in pairs:
        c = torch.randn(rows, generator=g) * 4
        lses = fresh()
        lses[a], lses[b] = c + math.log(0.7), c + math.log(0.3)
        yield f"two_live_{a}_{b}", outs, lses, False
    # (f) very negative with a masked peer: every finite lse in [-250, -150]
    if s > 1:
        lses = -250.0 + 100.0 * torch.rand(s, rows, generator=g)
        lses[(r + 1) % s, r] = NEG_INF
        yield "very_negative_masked_peer", outs, lses, False


def reference(outs: torch.Tensor, lses: torch.Tensor):
    """The combine formula in fp64, rounded to fp32."""
    o, l = nc.merge_partials(outs.double(), lses.double())
    return o.float(), l.float()


def check(name, out, lse, outs, lses, exact: bool, what: str) -> dict:
    """Compare (out, lse) with the fp64 reference: by equality where the
    content says so, else at RTOL / ATOL. -> the worst errors, for a
    caller that wants to print them before it asserts."""
    out, lse = out.detach().float().cpu(), lse.detach().float().cpu()
    ref_o, ref_l = reference(outs, lses)
    fin = torch.isfinite(ref_l)
    err = {"out": float((out - ref_o).abs().max()),
           "lse": float((lse[fin] - ref_l[fin]).abs().max()) if fin.any()
           else 0.0}
    where = f"{what} [{name}] S={outs.shape[0]} rows={outs.shape[1]} " \
            f"D={outs.shape[2]}"
    if exact:
        assert torch.equal(out, ref_o), f"{where}: out not bit-equal"
        assert torch.equal(lse, ref_l), f"{where}: lse not bit-equal"
    else:
        torch.testing.assert_close(out, ref_o, rtol=RTOL, atol=ATOL,
                                   msg=lambda m: f"{where}: out\n{m}")
        torch.testing.assert_close(lse, ref_l, rtol=RTOL, atol=ATOL,
                                   msg=lambda m: f"{where}: lse\n{m}")
    return err


def one_finite_is_exact(outs, lses) -> None:
    """The reference of a one-finite content IS that partial, bit for bit
    (exp(0) = 1, log(1) = 0): what `exact` relies on."""
    p = int(torch.isfinite(lses[:, 0]).nonzero()[0])
    ref_o, ref_l = reference(outs, lses)
    assert torch.equal(ref_o, outs[p]) and torch.equal(ref_l, lses[p])
