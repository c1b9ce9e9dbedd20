"""Measurement tool (not a test): the 2-D position bias per linear region with two heads per offset group (csrc/cpb_regions.h, "_mh"
entry points) against the per-pair MLP kernels.

Times DeformCrossAttention2D(dim=128, heads=8, offset_groups=4) forward + backward at B = 8, C = 128, a 100 x 100 token grid (10 000
queries, 625 sampled keys), with cpb_regions_multi_head False and True, with device events after a warm-up and over windows of at least
--min-seconds.  Also prints the region count of the tables and the share of pairs without a region (they evaluate the MLP), as
tests/test_gpu_regions.py does.  Prints one line per case and a JSON summary.

    python tests/tools/bench_regions_multihead.py [--min-seconds 1.0] [--side 100] [--regions 0|1]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_regions1d import timed                    # noqa: E402
from helpers import params_for, smml, synth          # noqa: E402

Fh = smml.functional


def module(dev, regions):
    mod = smml.DeformCrossAttention2D(dim=128, heads=8, offset_groups=4, cpb_regions_multi_head=regions)
    mod.load_state_dict(params_for(mod, 42, "bench2d_g4"))
    return mod.to(dev)


def inputs(dev, n):
    B, C = 8, 128
    x1 = synth.normal((B, n, C), 42, "bench2d_g4:x1").to(dev).requires_grad_()
    x2 = synth.normal((B, n, C), 42, "bench2d_g4:x2").to(dev).requires_grad_()
    w = synth.normal((B, n, C), 42, "bench2d_g4:w").to(dev)
    return x1, x2, w


def region_stats(dev, n):
    """Region count, kink records and the share of pairs that evaluated the MLP, from one forward of the region path."""
    mod = module(dev, True)
    x1, x2, _ = inputs(dev, n)
    Fh.DECISION_TAP = tapped = []
    try:
        mod.forward_tokens(x1, x2)
    finally:
        Fh.DECISION_TAP = None
    torch.cuda.synchronize()
    a = [e for e in tapped if e["kind"] == "attn"][0]
    B, H, N, J = a["B"], a["heads"], a["N"], a["J"]
    rid = a["region_ids"].to(torch.int64) & 0xFFFF
    nst = rid.shape[2] * 32
    valid = rid.view(B, H, nst // 32, J, 32).permute(0, 1, 3, 2, 4).reshape(B, H, J, nst)[..., :N]
    view = Fh.region_tables_view(a["tables"])
    return {"regions": view["n_regions"], "kink_records": view["n_edge"], "refined_cells": view["n_sub"], "overflow": view["overflow"],
            "share_without_region": float((valid == 0xFFFF).float().mean()), "keys": J}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--side", type=int, default=100, help="token grid side (N = side^2)")
    ap.add_argument("--regions", type=int, choices=(0, 1), default=None, help="only this setting of the switch (e.g. under a profiler)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = a.side * a.side
    res = {}
    for regions in ((False, True) if a.regions is None else (bool(a.regions),)):
        mod = module(dev, regions)
        x1, x2, w = inputs(dev, n)

        def run():
            (mod.forward_tokens(x1, x2) * w).sum().backward()
        ms, reps = timed(run, a.min_seconds)
        res[f"module_n{n}_multihead{int(regions)}_ms"] = ms
        print(f"DeformCrossAttention2D(heads=8, offset_groups=4) fwd+bwd 8x128x{n} cpb_regions_multi_head={regions}: {ms:.3f} ms ({reps} reps)",
              flush=True)
    if a.regions in (None, 1):
        st = region_stats(dev, n)
        res["region_stats"] = st
        print(f"region path: {st['regions']} regions, {st['kink_records']} kink records, {st['refined_cells']} refined cells, {st['keys']} keys; "
              f"{st['share_without_region']:.2e} of the pairs evaluated the MLP", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
