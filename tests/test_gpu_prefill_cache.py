"""fa_prefill_cache_kernel through its two bindings against the fp64 masked
softmax of tests/prefill_cases.py, at the smallest shapes at which each of
its mechanisms can fail."""

import pytest
import torch

import prefill_cases as pc

pytestmark = pytest.mark.gpu

BF16, FP16 = torch.bfloat16, torch.float16
ALL = (0, 1, 64)   # (rank, world, block): one rank owns every token
# id: (t0, T, rwb, page or None = slab, dtype, aimed, forced splits)
CASES = {
    "a-causal-slab": (0, 33, ALL, None, BF16, False, (0,)),
    "b-slab": (300, 296, ALL, None, BF16, True, (0, 3)),
    "b-page128": (300, 296, ALL, 128, BF16, True, (0,)),
    "b-page128-fp16": (300, 296, ALL, 128, FP16, True, (0,)),
    "c-page256": (300, 296, ALL, 256, BF16, True, (0,)),
    "d-staircase-slab": (5, 70, (1, 3, 4), None, BF16, True, (0,)),
    "d-staircase-vis0-slab": (5, 70, (2, 3, 4), None, BF16, True, (0,)),
    "e-page128-splits": (300, 296, ALL, 128, BF16, True, (1, 3)),
}


@pytest.fixture(scope="module")
def ext():
    from tree_attention_torch_amd.ops import flash

    assert flash.hip_available(), "HIP extension must be built in-tree"
    return flash._load_extension()


def _nan_filled(shape, dtype):
    """0xFF bytes: a NaN in bf16 and in fp16."""
    return torch.full((*shape[:-1], shape[-1] * 2), 0xFF,
                      dtype=torch.uint8).view(dtype)


def _launch(ext, q, k, v, vis, page, splits):
    """Store k / v (HKV, n, D) as the layout asks, every row the sequence
    does not hold NaN-filled, and run the binding."""
    n, dt = k.shape[1], k.dtype
    qd, vis_d = q[None].cuda(), vis.cuda()
    llen = torch.tensor([n], dtype=torch.long, device="cuda")
    if page is None:
        cap = n + 37 + (1 if (n + 37) % 128 == 0 else 0)   # no tile multiple
        ks, vs = (_nan_filled((1, pc.HKV, cap, pc.D), dt) for _ in range(2))
        ks[0, :, :n], vs[0, :, :n] = k, v
        return ext.flash_attention_cache_prefill(
            qd, ks.cuda(), vs.cuda(), llen, vis_d, pc.SCALE, splits)
    live = -(-n // page)
    # a scrambled table over a pool with 3 pages of no row; 8 entries wide,
    # the ones past the live pages name no page at all and are never read
    ids = torch.randperm(live + 3, generator=torch.Generator().manual_seed(7))
    kp, vp = (_nan_filled((live + 3, pc.HKV, page, pc.D), dt)
              for _ in range(2))
    for j in range(live):
        m = min(page, n - j * page)
        kp[ids[j], :, :m] = k[:, j * page : j * page + m]
        vp[ids[j], :, :m] = v[:, j * page : j * page + m]
    table = torch.full((8,), 10 ** 6, dtype=torch.int32)
    table[:live] = ids[:live].int()
    return ext.flash_attention_paged_prefill(
        qd, kp.cuda(), vp.cuda(), table.cuda(), llen, vis_d, pc.SCALE, splits)


@pytest.mark.parametrize("g", [1, 4])
@pytest.mark.parametrize("case", CASES)
def test_prefill_cache_kernel(ext, case, g):
    """(a) pure causal, a partial wave; (b) two q-blocks, the second partial,
    a prefix over three pages, a partial last tile, by the plan (S = 2 here)
    and on the slab with S = 3; (c) page 256; (d) staircase limits under
    (1, 3, 4), and under (2, 3, 4) where the first rows see nothing (exactly
    out = 0, lse = -inf); (e) S = 1 and S = 3 over a table 8 pages wide
    (chunk 384: q-block 0 owns an empty chunk, rows of its chunk 1 see none
    of it, chunk 1 ends mid-page).

    The aimed cases fail on a limit off by one: checked on the CPU, the fp64
    reference passes these bars against itself with vis as it is and misses
    them (out off by > 1) with vis + 1 and with vis - 1."""
    t0, t, rwb, page, dtype, aimed, forced = CASES[case]
    q, k, v, vis = pc.make(t0, t, rwb, dtype, g, aimed)
    ref_o, ref_l = pc.reference(q, k, v, vis)
    first = None
    for splits in forced:
        out, lse = _launch(ext, q, k, v, vis, page, splits)
        out, lse = out[0].cpu().double(), lse[0].cpu().double()
        if first is not None:   # S = 1 and S = 3 agree
            torch.testing.assert_close(out, first, **pc.OUT_TOL)
        first = out
        print(case, g, splits, "out err", (out - ref_o).abs().max().item(),
              "lse err", (lse - ref_l)[:, vis > 0].abs().max().item())
        assert torch.isfinite(out).all()
        torch.testing.assert_close(out, ref_o, **pc.OUT_TOL)
        torch.testing.assert_close(lse, ref_l, **pc.LSE_TOL)
        blind = vis == 0
        assert (out[:, blind] == 0).all() and (lse[:, blind] == -torch.inf).all()
