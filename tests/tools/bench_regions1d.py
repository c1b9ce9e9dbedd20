"""Measurement tool (not a test): the 1-D position bias per linear piece (csrc/cpb_regions1d.h) against the per-pair MLP kernels.

Times, with device events after a warm-up of every shape and over windows of at least 1 s:
  * DeformCrossAttention1D forward + backward at B = 8, C = 128, N in {2 501, 10 001};
  * one DeformPathomicNet training step with attn_dim = 1 at 8 bags x 10 000 instances x 512 features;
each with cpb_regions (resp. args.deform1d_cpb_regions) False and True.  Prints one line per case and a JSON summary.

    python tests/tools/bench_regions1d.py [--min-seconds 1.0] [--only module|model] [--n 10001] [--regions 0|1]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import params_for, smml, synth          # noqa: E402
from test_oracle_golden import pathomic_args         # noqa: E402


def timed(fn, min_seconds):
    """ms per call: device events around batches of calls until the window is >= min_seconds."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    reps = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 1000.0 * min_seconds:
            return ms / reps, reps
        reps = max(reps * 2, int(reps * 1000.0 * min_seconds / max(ms, 1e-3) * 1.1) + 1)


def module_case(dev, n, regions, min_seconds):
    B, C = 8, 128
    mod = smml.DeformCrossAttention1D(dim=C, downsample_factor=4, offset_scale=2, offset_kernel_size=6, cpb_regions=regions)
    mod.load_state_dict(params_for(mod, 42, "bench1d"))
    mod = mod.to(dev)
    x1 = synth.normal((B, n, C), 42, "bench1d:x1").to(dev).requires_grad_()
    x2 = synth.normal((B, n, C), 42, "bench1d:x2").to(dev).requires_grad_()
    w = synth.normal((B, n, C), 42, "bench1d:w").to(dev)

    def run():
        (mod.forward_tokens(x1, x2) * w).sum().backward()
    return timed(run, min_seconds)


def model_case(dev, regions, min_seconds):
    B, n = 8, 10000
    args = pathomic_args(attn_dim=1, return_vgrid=False, input_path_dim=512, deform1d_cpb_regions=regions, batch_size=B)
    net = smml.DeformPathomicNet(args)
    net.load_state_dict(params_for(net, 42, "bench1d:model"))
    net = net.to(dev)
    x = synth.bag(B, n, 512, 42, "bench1d:bag").to(dev)
    xt, xi = synth.normal((B, 59), 42, "bench1d:t").to(dev), synth.normal((B, 361), 42, "bench1d:i").to(dev)
    label = torch.arange(B, device=dev) % 4

    def run():
        for p in net.parameters():
            p.grad = None
        feats, _, _, lg, _, _, _ = net(x_path=x, x_omic=None, x_omic_tumor=xt, x_omic_immune=xi)
        (torch.nn.functional.cross_entropy(lg[2], label) + feats.pow(2).mean()).backward()
    return timed(run, min_seconds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--only", choices=("module", "model"), default=None)
    ap.add_argument("--n", type=int, default=None, help="module case: only this token count")
    ap.add_argument("--regions", type=int, choices=(0, 1), default=None, help="only this setting of the switch (e.g. under a profiler)")
    a = ap.parse_args()
    flags = (False, True) if a.regions is None else (bool(a.regions),)
    dev = torch.device("cuda:0")
    res = {}
    if a.only in (None, "module"):
        for n in ((2501, 10001) if a.n is None else (a.n,)):
            for regions in flags:
                ms, reps = module_case(dev, n, regions, a.min_seconds)
                res[f"module_n{n}_regions{int(regions)}_ms"] = ms
                print(f"DeformCrossAttention1D fwd+bwd 8x128x{n} cpb_regions={regions}: {ms:.3f} ms ({reps} reps)", flush=True)
    if a.only in (None, "model"):
        for regions in flags:
            ms, reps = model_case(dev, regions, a.min_seconds)
            res[f"pathomic_step_regions{int(regions)}_ms"] = ms
            print(f"DeformPathomicNet step attn_dim=1 8x10000x512 deform1d_cpb_regions={regions}: {ms:.3f} ms ({reps} reps)", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
