"""Paged latent pools, the fp64 reference and a session walk for the MLA paged
tests (GPU and CPU)."""

import math

import torch

import tree_attention_torch_amd as ta
from needle_cases import BARS

OUT_BAR, LSE_BAR = BARS["half"]
NAN = float("nan")


def paged(lens, page, dtype=torch.bfloat16, seed=0, max_pages=None):
    """rows[b] (lens[b], 576) and a pool / permuted table holding them; the
    pool's first and last page are named by out-of-range ids (clamped); NaN
    (or an id far outside) wherever nothing may be read."""
    g = torch.Generator().manual_seed(seed)
    need = [-(-n // page) for n in lens]
    n_pages = sum(need) + 3
    mid = (torch.randperm(n_pages - 2, generator=g) + 1).tolist()
    ids = ([0, n_pages - 1] + mid)[: sum(need)]
    ids = [ids[i] for i in torch.randperm(len(ids), generator=g).tolist()]
    pool = torch.full((n_pages, 1, page, 576), NAN, dtype=dtype)
    table = torch.full((len(lens), max_pages or max(need) + 1), 1 << 30,
                       dtype=torch.int32)
    rows = []
    for b, n in enumerate(lens):
        r = torch.randn(n, 576, generator=g).to(dtype)
        rows.append(r)
        for j in range(need[b]):
            pid = ids.pop()
            pool[pid, 0, : min(page, n - j * page)] = r[j * page : (j + 1) * page]
            table[b, j] = {0: -3, n_pages - 1: n_pages + 5}.get(pid, pid)
    return rows, pool, table


def ref64(q, rows, vis=None, scale=None):
    """fp64 masked softmax: key p is masked for query t iff p >= vis[b][t]."""
    scale = scale or 1.0 / math.sqrt(576)
    outs, lses = [], []
    for b, r in enumerate(rows):
        k = r.double().cpu()
        s = torch.matmul(q[b].double().cpu(), k.T) * scale   # (Hq, Tq, n)
        if vis is not None:
            dead = torch.arange(len(k))[None, :] >= torch.as_tensor(vis[b])[:, None]
            s = s.masked_fill(dead[None], -math.inf)
        lse = torch.logsumexp(s, -1) if len(k) else s.new_full(s.shape[:2], -math.inf)
        p = torch.exp(s - lse.clamp(min=-1e300)[..., None]).nan_to_num(0.0)
        outs.append(p @ k[:, :512])
        lses.append(lse)
    return torch.stack(outs), torch.stack(lses)


def check(out, lse, ro, rl):
    print("max |out err|", (out.double().cpu() - ro).abs().max().item())
    torch.testing.assert_close(out.double().cpu(), ro, rtol=OUT_BAR, atol=OUT_BAR)
    if lse is not None:
        torch.testing.assert_close(lse.double().cpu(), rl, rtol=LSE_BAR, atol=LSE_BAR)


def chain(lens, tq):
    return [[max(n - (tq - 1 - i), 0) for i in range(tq)] for n in lens]


def session_walk(device, group=None, block=256, hq=16):
    """Every session step against the fp64 reference over a host mirror."""
    g = torch.Generator().manual_seed(5)
    new = lambda *s: torch.randn(*s, generator=g).bfloat16()
    sess = ta.PagedMlaSession(3, 600, page=128, n_pages=8, block=block,
                              group=group, device=device)
    mirror, seen = [new(n, 576) for n in (130, 5, 250)], []
    for b, r in enumerate(mirror):
        sess.prefill(b, r.to(device))

    def attend(tq, vis=None):
        q = new(3, hq, tq, 576)
        fn = sess.attend if tq == 1 else sess.attend_many
        out = fn(q.to(device))
        check(out, None, ref64(q, mirror, vis)[0], None)
        seen.append(out.cpu())

    attend(1)
    for active in (None, [True, False, True]):
        c = new(3, 1, 1, 576)
        sess.append(c.to(device), active)
        for b in range(3):
            if active is None or active[b]:
                mirror[b] = torch.cat([mirror[b], c[b, 0]])
        attend(1)
    c, counts = new(3, 1, 3, 576), [3, 0, 2]
    before = [len(r) for r in mirror]
    sess.append_many(c.to(device), counts)
    mirror = [torch.cat([r, c[b, 0, :n]]) for b, (r, n) in enumerate(zip(mirror, counts))]
    attend(3, [[t0 + (min(i, n - 1) + 1 if n else 0) for i in range(3)]
               for t0, n in zip(before, counts)])
    sess.truncate(0, before[0] + 1)     # one draft of row 0 accepted
    mirror[0] = mirror[0][: before[0] + 1]
    attend(1)
    free = sess.free_pages
    sess.reset(2)
    assert sess.free_pages > free
    mirror[2] = new(140, 576)
    sess.prefill(2, mirror[2].to(device))   # takes the pages row 2 gave back
    assert sess.totals == [len(r) for r in mirror]
    attend(1)
    return torch.cat([o.flatten() for o in seen])
