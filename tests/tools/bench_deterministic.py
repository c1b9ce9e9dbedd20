"""Measurement tool (not a test): what the deterministic mode (functional.deterministic) costs.

At the headline shape - 8 bags of 10 000 x 512, a 100 x 100 token grid, 625 sampled keys - it times, default and deterministic
INTERLEAVED in one process (one timed call of each in turn, so that drift of the machine hits both alike):
  * the four kernel families the mode replaces, each at the shape the step launches it with
      gemm       weight gradient of a 512 -> 128 linear layer over 80 000 rows (split-K)
      layernorm  backward on [80 000, 128]
      colsum     bias gradient [1, 80 000, 512] and the Pooler mean [8, 10 000, 128]
      sampler    backward of the bilinear sampler, 8 x 100 x 100 x 128 map, 8 groups, 625 keys (default: zero fill + scatter)
  * the whole training step of bench.py (DeformCrossTransMIL + cross-entropy + BatchLoss + Adam, train mode).
Device events around every call; per case the min and the median over --steps calls (>= 10) after --warmup (3) of each mode.
Prints one line per case and a JSON summary.

    python tests/tools/bench_deterministic.py [--steps 12] [--warmup 3] [--grid 100] [--bags 8]
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
from helpers import smml, synth          # noqa: E402
import bench                             # noqa: E402

Fh = smml.functional
capi = smml._capi


def interleaved(run, steps, warmup):
    """run(det) timed with device events, default and deterministic in turn -> {mode: (min ms, median ms)}."""
    for _ in range(warmup):
        for det in (False, True):
            run(det)
    torch.cuda.synchronize()
    ms = {False: [], True: []}
    for _ in range(steps):
        for det in (False, True):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(det)
            b.record()
            b.synchronize()
            ms[det].append(a.elapsed_time(b))
    return {("deterministic" if k else "default"): (min(v), statistics.median(v)) for k, v in ms.items()}


def family_cases(dev, B, S):
    L = capi.lib()
    n = S * S
    R = B * n
    gen = torch.Generator().manual_seed(1)
    rn = lambda *s: torch.randn(*s, generator=gen).to(dev)
    cases = {}

    dy, x = rn(R, 512), rn(R, 128)
    sk = Fh._splitk_for(512, 128, R)

    def gemm(det):
        dw = torch.empty(512, 128, device=dev) if det else Fh._ZEROS.zeros((512, 128), dev)
        Fh._gemm(dy, x, dw, M=512, N=128, K=R, sam=1, sak=512, sbk=128, sbn=1, ldc=128, splitk=sk, det=det)
    cases[f"gemm dW [512 x 128] over {R} rows, splitk {sk}"] = gemm

    xl, dyl, g = rn(R, 128), rn(R, 128), rn(128)
    y, mean, rstd = torch.empty_like(xl), torch.empty(R, device=dev), torch.empty(R, device=dev)
    capi.check(L.smml_layernorm_fwd_f32(capi.fptr(xl), capi.fptr(g), capi.fptr(g), capi.fptr(y), capi.fptr(mean), capi.fptr(rstd), R, 128, 1e-5,
                                        capi.stream()))
    dxl = torch.empty_like(xl)
    wsb = L.smml_layernorm_bwd_det_workspace_bytes(R, 128)

    def layernorm(det):
        dg, db = Fh._ZEROS.zeros((128,), dev), Fh._ZEROS.zeros((128,), dev)
        args = (capi.fptr(xl), capi.fptr(dyl), capi.fptr(g), capi.fptr(mean), capi.fptr(rstd), capi.fptr(dxl), capi.fptr(dg), capi.fptr(db), R, 128,
                1, 1.0, 0)
        if det:
            ws = Fh._scratch(wsb, dev)
            capi.check(L.smml_layernorm_bwd_det_f32(*args, capi.fptr(ws), wsb, capi.stream()))
        else:
            capi.check(L.smml_layernorm_bwd_f32(*args, capi.stream()))
    cases[f"layernorm backward [{R}, 128]"] = layernorm

    xb = dy.view(1, R, 512)
    cases[f"colsum [1, {R}, 512]"] = lambda det: Fh.colsum(xb, det=det)
    xp = xl.view(B, n, 128)
    cases[f"colsum [{B}, {n}, 128]"] = lambda det: Fh.colsum(xp, 1.0 / n, det=det)

    G, cg = 8, 16
    J = L.smml_offsets_out_len(S, 6, 4) ** 2
    xm = rn(B, S, S, G * cg)
    vs = (torch.rand(B * G, J, 2, generator=gen) * 2.4 - 1.2).to(dev)
    dkv = rn(B, J, G * cg)
    dvs = torch.empty_like(vs)
    wss = L.smml_bilinear_sample_bwd_det_workspace_bytes(B, S, S, G, J)

    def sampler(det):
        dvs.zero_()
        if det:
            dx, ws = torch.empty_like(xm), Fh._scratch(wss, dev)
            capi.check(L.smml_bilinear_sample_bwd_det_f32(capi.fptr(xm), capi.fptr(vs), capi.fptr(dkv), capi.fptr(dx), capi.fptr(dvs), capi.fptr(ws),
                                                          wss, B, S, S, G, cg, J, 2, capi.stream()))
        else:
            dx = torch.zeros_like(xm)
            capi.check(L.smml_bilinear_sample_bwd_f32(capi.fptr(xm), capi.fptr(vs), capi.fptr(dkv), capi.fptr(dx), capi.fptr(dvs), B, S, S, G, cg,
                                                      J, 2, capi.stream()))
    cases[f"sampler backward {B} x {S} x {S} x {G * cg}, {J} keys"] = sampler
    return cases


def step_case(dev, B, S, in_dim):
    torch.manual_seed(42)
    mil = smml.DeformCrossTransMIL(bench.mil_args(in_dim))
    mil.load_state_dict(synth.fill_params({k: tuple(v.shape) for k, v in mil.state_dict().items()}, 42, "bench"))
    mil = mil.to(dev).train()
    opt = bench.make_adam(mil.parameters())
    bloss = smml.BatchLoss(B, 1)
    path = synth.bag(B, S * S, in_dim, 42, "bench:bag").to(dev)
    omic = torch.relu(synth.normal((B, 128), 42, "bench:omicvec")).to(dev)
    label = torch.randint(0, 4, (B,), generator=torch.Generator().manual_seed(0)).to(dev)

    def step(det):
        with smml.deterministic(det):
            enc, logits, _, omic_t, vgrid = mil(path, omic)
            loss = torch.nn.functional.cross_entropy(logits, label) + torch.sum(bloss(omic_t, vgrid))
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--grid", type=int, default=100, help="token grid side (N = grid^2)")
    ap.add_argument("--bags", type=int, default=8)
    ap.add_argument("--in-dim", type=int, default=512)
    a = ap.parse_args()
    if a.steps < 10:
        raise SystemExit("--steps must be at least 10")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    res = {}
    cases = family_cases(dev, a.bags, a.grid)
    cases[f"training step {a.bags} x {a.grid * a.grid} x {a.in_dim}"] = step_case(dev, a.bags, a.grid, a.in_dim)
    for name, run in cases.items():
        r = interleaved(run, a.steps, a.warmup)
        d, t = r["default"], r["deterministic"]
        res[name] = {"default_ms": {"min": d[0], "median": d[1]}, "deterministic_ms": {"min": t[0], "median": t[1]}, "ratio_of_medians": t[1] / d[1]}
        print(f"{name}: default min {d[0]:.4f} / median {d[1]:.4f} ms, deterministic min {t[0]:.4f} / median {t[1]:.4f} ms "
              f"(x {t[1] / d[1]:.2f})", flush=True)
    print(json.dumps({"steps": a.steps, "warmup": a.warmup, "cases": res}))


if __name__ == "__main__":
    main()
