"""Measure actual fp8 kernel error vs the dequantized-KV fp32 oracle, to
set honest test tolerances.

    python tools/fp8_err.py            # decode sweep (25 cases)
    python tools/fp8_err.py --prefill  # prefill-kernel sweep (30 cases)
    python tools/fp8_err.py --tree     # the end-to-end fp8+GQA tree config

The test bars are the printed WORST x 2.5 (tests/test_gpu_kernels.py
_check_fp8_decode / test_fp8_prefill, tests/test_gpu_tree.py).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tree_attention_torch_amd.ops import flash  # noqa: E402
from tree_attention_torch_amd.ops.reference import flash_res_lse  # noqa: E402

DECODE = [(1, 8, 8, 4096, 1, False), (1, 32, 4, 8192, 1, False),
          (2, 8, 2, 1500, 1, False), (1, 8, 8, 1024, 256, True),
          (1, 16, 2, 2048, 512, True)]
# prefill kernel (fa_prefill2_fp8): the shapes the tests assert on first,
# then q_offset > 0, ragged rows/keys, non-causal, GQA 8:1, two q-blocks
PREFILL = [(1, 2, 2, 512, 512, True), (1, 4, 1, 300, 300, True),
           (1, 8, 8, 1024, 256, True), (1, 16, 2, 2048, 512, True),
           (2, 4, 4, 777, 333, False), (1, 8, 1, 4096, 1024, True)]


def sweep(shapes, seeds):
    ext = flash._load_extension()
    worst_o = worst_l = 0.0
    n = 0
    for seed in range(seeds):
        torch.manual_seed(seed)
        for (b, hq, hkv, t, tq, causal) in shapes:
            q = torch.randn(b, hq, tq, 128, device="cuda").bfloat16()
            k8 = torch.randn(b, hkv, t, 128, device="cuda").to(
                torch.float8_e4m3fn)
            v8 = torch.randn(b, hkv, t, 128, device="cuda").to(
                torch.float8_e4m3fn)
            scale = 128 ** -0.5
            o, l = ext.flash_attention(q, k8, v8, scale, causal, t - tq, 0)
            ro, rl = flash_res_lse(q.float().cpu(), k8.float().cpu(),
                                   v8.float().cpu(), scale, causal, t - tq, 0)
            eo = (o.cpu() - ro).abs().max().item()
            el = (l.cpu() - rl).abs().max().item()
            worst_o = max(worst_o, eo)
            worst_l = max(worst_l, el)
            n += 1
            print(f"seed{seed} b{b} hq{hq} hkv{hkv} t{t} tq{tq} "
                  f"c{int(causal)}: max|dO|={eo:.4f} max|dLSE|={el:.4f}",
                  flush=True)
    print(f"WORST over {n} cases: dO={worst_o:.4f} dLSE={worst_l:.4f} "
          f"(x2.5: {2.5 * worst_o:.4f} / {2.5 * worst_l:.4f})")


def tree(seeds):
    """tests/test_gpu_tree.py::test_fp8_gqa_tree_attention_gpu's config
    (fp8 KV + GQA 8:1 decode over 8192 keys through tree_attention)."""
    import tree_attention_torch_amd as ta

    worst = 0.0
    for seed in range(seeds):
        torch.manual_seed(seed)
        q, k, v = ta.make_data((1, 32, 8192, 128), rank=seed, device="cuda",
                               dtype="fp8", kv_heads=4)
        out = ta.tree_attention(q, k, v)
        ref = ta.attention_reference(q.cpu(), k.cpu().float(),
                                     v.cpu().float())
        e = (out.cpu() - ref).abs().max().item()
        worst = max(worst, e)
        print(f"tree rank-seed{seed}: max|dO|={e:.4f}", flush=True)
    print(f"WORST over {seeds} cases: dO={worst:.4f} (x2.5: {2.5 * worst:.4f})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--prefill", action="store_true")
    ap.add_argument("--tree", action="store_true")
    ap.add_argument("--seeds", type=int, default=5)
    a = ap.parse_args()
    if a.prefill:
        sweep(PREFILL, a.seeds)
    elif a.tree:
        tree(a.seeds)
    else:
        sweep(DECODE, a.seeds)
