"""Times the attention-maps pass (functional.deform_attention_maps without the dense output: smml_attn_maps_f32 + smml_attn_splat_f32) beside
the fused forward it follows, at the headline shape (8 bags x 8 heads x 10 000 queries x 625 keys, 2-D region path, inference): HIP events
around every call, `--warmup` untimed and `--steps` timed calls each (bench.py's defaults), medians.  Bytes are what the pass has to move,
from the shapes: the live score tiles and lse once, the partial rows written and read once, key_mass; the splat's traffic is the mass, the
sample positions and the map.  Writes one JSON line to stdout and to --out.  Needs the GPU: there is no CPU form of these kernels."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
smml = importlib.import_module("subspace-multimodal-learning_amd")
Fh = smml.functional


def timed(fn, warmup, steps):
    """Median / min / max GPU milliseconds of fn() from HIP events on the launch stream."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bags", type=int, default=8)
    ap.add_argument("--grid", type=int, default=100, help="token grid side (N = grid^2)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_maps_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_attn_maps needs the GPU (no CPU form of the kernels)")
    dev = torch.device("cuda", 0)
    B, S, H = a.bags, a.grid, 8
    T = smml.lib().smml_offsets_out_len(S, 6, 4)
    N, J = S * S, T * T
    gen = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=gen)
    shapes = {"mlp.0.0.weight": (32, 2), "mlp.0.0.bias": (32,), "mlp.1.0.weight": (32, 32), "mlp.1.0.bias": (32,), "mlp.2.weight": (1, 32), "mlp.2.bias": (1,)}
    p = smml.synth.fill_params({"layer3.attn2d.rel_pos_bias." + k: v for k, v in shapes.items()}, 42, "bench")
    w = [p["layer3.attn2d.rel_pos_bias." + k].to(dev) for k in shapes]
    ax = 2.0 * torch.arange(S, dtype=torch.float32) / (S - 1) - 1.0
    gq = torch.stack((ax.view(1, S).expand(S, S), ax.view(S, 1).expand(S, S)), dim=-1).reshape(N, 2).contiguous().to(dev)
    off = torch.tanh(rn(B * H, 2, T, T) * 0.7) * 4.0
    gx = torch.arange(T, dtype=torch.float32).view(1, T).expand(T, T)
    vs = (2.0 * (torch.stack((gx, gx.t()), 0)[None] + off) / max(T - 1, 1) - 1.0).permute(0, 2, 3, 1).reshape(B * H, J, 2).contiguous().to(dev)
    q, k, v = (rn(B, N, 512) * 0.4).to(dev), (rn(B, J, 512) * 0.4).to(dev), rn(B, J, 512).to(dev)
    pmax = Fh.table_pmax(1.0, float(vs.abs().max()))
    sink = Fh.AttnScores()

    def forward(**kw):
        with torch.no_grad():
            return Fh.deform_attention(q, k, v, vs, gq, *w, heads=H, groups=H, scale=0.125, cpb_regions=True, cpb_region_pmax=pmax, **kw)

    res = {"shape": {"bags": B, "heads": H, "queries": N, "keys": J, "grid": [S, S]}, "warmup": a.warmup, "steps": a.steps}
    res["forward_inference_ms"] = timed(forward, a.warmup, a.steps)
    res["forward_keeping_scores_ms"] = timed(lambda: forward(attn_scores=sink), a.warmup, a.steps)
    maps = lambda: Fh.deform_attention_maps(sink, vs, heads=H, groups=H, grid_hw=(S, S))
    res["maps_ms"] = timed(maps, a.warmup, a.steps)
    mass = maps()["key_mass"]
    L, capi = smml.lib(), Fh.capi
    pm = torch.empty(B, H, S, S, device=dev)
    res["splat_ms"] = timed(lambda: capi.check(L.smml_attn_splat_f32(capi.fptr(mass), capi.fptr(vs), capi.fptr(pm), B, H, H, J, S, S, capi.stream())),
                            a.warmup, a.steps)
    tiles = (N + 31) // 32
    slices = (tiles + 7) // 8
    wsb = L.smml_attn_maps_workspace_bytes(B, N, J, H)
    ws, km = torch.empty((wsb + 3) // 4, device=dev), torch.empty(B, H, J, device=dev)
    res["maps_stream_ms"] = timed(lambda: capi.check(L.smml_attn_maps_f32(capi.fptr(sink.logits), capi.fptr(sink.lse), capi.fptr(km), None,
                                                                          capi.fptr(ws), wsb, B, N, J, H, capi.stream())), a.warmup, a.steps)
    assert torch.equal(km, mass)
    nbytes = 4 * (B * H * tiles * 32 * J + B * H * N + 2 * B * H * slices * J + B * H * J)
    res["maps_stream_bytes"] = nbytes              # smml_attn_maps_f32 alone (both kernels), buffers allocated outside the timed call
    res["maps_stream_bytes_per_s"] = nbytes / (res["maps_stream_ms"]["median"] * 1e-3)
    res["maps_over_forward"] = res["maps_ms"]["median"] / res["forward_keeping_scores_ms"]["median"]
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
