"""The fp64 reference under an ancestor mask and a session walk with a draft
tree for the MLA tree tests (GPU and CPU)."""

import math

import torch

import tree_attention_torch_amd as ta
from mla_fp8_cases import deq, spread
from mla_paged_cases import check, ref64


def ref64_tree(q, rows, bases, masks, scale=None):
    """fp64 masked softmax: key p is dead for query i iff p >= bases[b] and
    bit p - bases[b] of masks[b][i] is clear (slots >= 16 have no bit)."""
    scale = scale or 1.0 / math.sqrt(576)
    outs, lses = [], []
    for b, r in enumerate(rows):
        k = r.double().cpu()
        slot = torch.arange(len(k)) - bases[b]
        m = torch.as_tensor(masks[b], dtype=torch.long)[:, None] & 0xFFFF
        live = (slot < 0)[None] | (((m >> slot.clamp(0, 16)[None]) & 1) == 1)
        s = (torch.matmul(q[b].double().cpu(), k.T) * scale).masked_fill(
            ~live[None], -math.inf)
        lse = torch.logsumexp(s, -1)
        p = torch.exp(s - lse.clamp(min=-1e300)[..., None]).nan_to_num(0.0)
        outs.append(p @ k[:, :512])
        lses.append(lse)
    return torch.stack(outs), torch.stack(lses)


# row 0: the accepted path 0 - 1 - 3 - 4 lands on tokens 125..128, across the
# page seam; row 1 keeps one node of five, so tokens 128..130 and the page
# they alone held go back
PARENTS = [[-1, 0, 0, 1, 3, 2], [-1, -1, 0, 2, 3, -1]]
COUNTS, PATHS, KEEP = [6, 5], [[0, 1, 3, 4], [1]], [4, 1]


def tree_walk(device, dtype="bf16", group=None, block=256, hq=16):
    """prefill, append_tree, attend_tree, commit and attend against fp64 over
    a host mirror (the dequantized rows under "fp8_block")."""
    fp8 = dtype == "fp8_block"
    g = torch.Generator().manual_seed(11)
    new = lambda *s: torch.randn(*s, generator=g).bfloat16()
    held = deq if fp8 else (lambda r: r)
    sess = ta.PagedMlaSession(2, 600, page=128, n_pages=6, dtype=dtype,
                              block=block, group=group, device=device)
    rows = [new(n, 576) for n in (125, 127)]
    rows = [spread(r) for r in rows] if fp8 else rows
    for b, r in enumerate(rows):
        sess.prefill(b, r.to(device))
    mirror = [held(r) for r in rows]
    c = new(2, 1, 6, 576)
    c = spread(c, 5) if fp8 else c
    sess.append_tree(c.to(device), PARENTS, COUNTS)
    masks = []
    for par, cnt in zip(PARENTS, COUNTS):   # node i and its ancestors
        row = []
        for i in range(6):
            m, n = 0, i if i < cnt else -1
            while n >= 0:
                m, n = m | 1 << n, par[n]
            row.append(m)
        masks.append(row)
    q = new(2, hq, 6, 576)
    seen = [sess.attend_tree(q.to(device)).cpu()]
    with_drafts = [torch.cat([r, held(c[b, 0, :n])])
                   for b, (r, n) in enumerate(zip(mirror, COUNTS))]
    check(seen[0], None,
          ref64_tree(q, with_drafts, [125, 127], masks)[0], None)
    free = sess.free_pages
    sess.commit(PATHS, KEEP)
    if sess.world == 1:   # tokens 128..131 of row 1 had a page of their own
        assert sess.free_pages == free + 1
    mirror = [torch.cat([r, held(c[b, 0, p])])
              for b, (r, p) in enumerate(zip(mirror, PATHS))]
    assert sess.totals == [129, 128]
    q = new(2, hq, 1, 576)
    seen.append(sess.attend(q.to(device)).cpu())
    check(seen[1], None, ref64(q, mirror)[0], None)
    return torch.cat([o.flatten() for o in seen])
