"""Measurement tool (not a test): forward + backward of DeformCrossAttention2D at dim = 256 and 512 (the wide position-bias family,
csrc/deform_attn_wide.hip) for 8 x 50 x 50 and 8 x 100 x 100 tokens, and beside them dim = 128 on the per-pair kernels (functional.CPB_REGIONS
off, the switch SMML_CPB_REGIONS=0 sets) in the same process.

Per case: device events around forward + backward of the module (train mode, dropout 0.1), min and median over --steps calls after --warmup;
in a second pass functional.TIMER brackets the fused forward (dim 128: attention + bias in one kernel; wide: bias kernel + attention kernel)
and the position-bias backward kernel alone.  The expectation to check, not a gate: the MLP's time grows about (W / 32)^2 against the
dim-128 line's position-bias share (the width-32 kernels' layer 2 runs on the 16-bit matrix pipe as split products, the wide family's on
the exact-fp32 MFMA at the vector rate, so the constant differs too).

    python tests/tools/bench_cpb_wide.py [--steps 5] [--warmup 2] [--bags 8] [--grids 50 100] [--dims 128 256 512] [--out profiles/cpb_wide_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import smml          # noqa: E402

Fh = smml.functional


def case(dev, dim, bags, grid, steps, warmup):
    torch.manual_seed(7)
    mod = smml.DeformCrossAttention2D(dim=dim, heads=8, offset_groups=8, dropout=0.1).to(dev).train()
    n = grid * grid
    gen = torch.Generator().manual_seed(dim + grid)
    x1 = (torch.randn(bags, n, dim, generator=gen) * 0.5).to(dev).requires_grad_()
    x2 = (torch.randn(bags, n, dim, generator=gen) * 0.5).to(dev).requires_grad_()
    wo = torch.randn(bags, n, dim, generator=gen).to(dev)

    def step():
        mod.zero_grad(set_to_none=True)
        x1.grad = x2.grad = None
        (mod.forward_tokens(x1, x2) * wo).sum().backward()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    Fh.TIMER.enabled = True
    try:
        step()
        torch.cuda.synchronize()
        kern = {k: {"launches": v[0], "mean_ms": v[1], "pairs": v[2]} for k, v in Fh.TIMER.collect().items()}
    finally:
        Fh.TIMER.enabled = False
    keys = int(Fh.capi.lib().smml_offsets_out_len(grid, 6, 4)) ** 2
    return {"dim": dim, "width": dim // 4, "bags": bags, "grid": grid, "keys": keys, "fwd_bwd_ms": {"min": min(ms), "median": statistics.median(ms)},
            "kernels": kern}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bags", type=int, default=8)
    ap.add_argument("--grids", type=int, nargs="+", default=[50, 100])
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cpb_wide_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    Fh.CPB_REGIONS = False            # dim 128 on the per-pair kernels (the wide family has no region path to compare with)
    res = []
    for grid in a.grids:
        for dim in a.dims:
            r = case(dev, dim, a.bags, grid, a.steps, a.warmup)
            res.append(r)
            k = ", ".join(f"{n} {v['mean_ms']:.3f} ms" for n, v in r["kernels"].items())
            print(f"dim {dim} (width {r['width']}) {a.bags} x {grid} x {grid}, {r['keys']} keys: forward + backward min {r['fwd_bwd_ms']['min']:.3f} / "
                  f"median {r['fwd_bwd_ms']['median']:.3f} ms; {k}", flush=True)
    doc = {"tool": "tests/tools/bench_cpb_wide.py", "note": "one box, one run", "device": torch.cuda.get_device_name(dev), "steps": a.steps,
           "warmup": a.warmup, "cases": res}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
