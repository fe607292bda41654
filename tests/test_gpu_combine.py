"""GPU (MI355X) tests of the three HIP combine kernels against an fp64
evaluation of the combine formula on the CPU (tests/combine_cases.py):

* combine_packed (fa_combine_kernel over the all-gathered buffer; the same
  kernel merges the split-KV partials) at S in {1, 2, 4, 5, 8, 9, 17, 64}:
  S = NG + 1 and 2 NG + 1 for NG = 512 / D = 4 and 8 make its
  `for (s = g; s < S; s += NG)` loops take a second and a third step;
* combine_rescale_pack + combine_finish (the halves of the all-reduce
  combine) at world sizes {2, 3, 8} and D in {32, 64, 112, 128}, the
  collective emulated by an fp32 elementwise max of m and an fp32 sum of
  packed, the inputs prepared by combine.allreduce_local_max, the helper
  tree_combine_allreduce itself calls.

Contents (combine_cases.contents): generic with a rotating masked split;
the dominant partial in the LAST split at lse +300 against -300; only one
split finite, at every position in turn (bit-equal to that partial); all
masked (out == 0, lse == -inf); two live splits at 0.7 / 0.3, first / last
and across the NG boundary; every finite lse in [-250, -150] beside a masked
peer. The bars are the combine tests' rtol = atol = 1e-5, applied to the
fp64 reference rounded to fp32. combine_partials (fp32, CPU) is held to the
same reference alongside.
"""

import pytest
import torch

import combine_cases as cc
from tree_attention_torch_amd.parallel.combine import (allreduce_local_max,
                                                       combine_partials)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from tree_attention_torch_amd.ops import flash

    assert flash.hip_available(), "HIP extension must be built in-tree"
    return flash._load_extension()


def _partials_eager(outs, lses):
    s, rows, d = outs.shape
    out, lse = combine_partials(outs.reshape(s, 1, rows, 1, d),
                                lses.reshape(s, 1, rows, 1))
    return out.reshape(rows, d), lse.reshape(rows)


@pytest.mark.parametrize("d", (64, 128))
@pytest.mark.parametrize("s", cc.SPLITS)
def test_combine_packed(ext, s, d):
    worst = {"out": 0.0, "lse": 0.0}
    for rows in cc.ROWS:
        for name, outs, lses, exact in cc.contents(s, rows, d, ng=512 // d):
            packed = torch.cat([outs, lses.unsqueeze(-1)], -1).cuda()
            out, lse = ext.combine_packed(packed.view(-1), s, 1, rows, 1, d)
            e = cc.check(name, out.reshape(rows, d), lse.reshape(rows), outs,
                         lses, exact, "combine_packed")
            worst = {k: max(worst[k], e[k]) for k in worst}
            cc.check(name, *_partials_eager(outs, lses), outs, lses, exact,
                     "combine_partials")
    print(f"combine_packed S={s} D={d}: worst |dO| {worst['out']:.3g} "
          f"|dLSE| {worst['lse']:.3g}")


@pytest.mark.parametrize("d", (32, 64, 112, 128))
@pytest.mark.parametrize("world", cc.WORLDS)
def test_combine_rescale_pack_and_finish(ext, world, d):
    worst = {"out": 0.0, "lse": 0.0}
    for rows in cc.ROWS:
        for name, outs, lses, exact in cc.contents(world, rows, d):
            o = outs.reshape(world, 1, rows, 1, d).cuda()
            l = lses.reshape(world, 1, rows, 1).cuda()
            # MAX all-reduce of what every rank offers, SUM of the packs
            m = torch.stack([allreduce_local_max(l[r])
                             for r in range(world)]).amax(0).contiguous()
            packed = None
            for r in range(world):
                p = ext.combine_rescale_pack(o[r].contiguous(),
                                             l[r].contiguous(), m)
                packed = p if packed is None else packed + p
            out, lse = ext.combine_finish(packed.contiguous(), m)
            e = cc.check(name, out.reshape(rows, d), lse.reshape(rows), outs,
                         lses, exact, "combine_rescale_pack + combine_finish")
            worst = {k: max(worst[k], e[k]) for k in worst}
    print(f"rescale_pack + finish world={world} D={d}: worst |dO| "
          f"{worst['out']:.3g} |dLSE| {worst['lse']:.3g}")
