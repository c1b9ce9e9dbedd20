"""Times the gated attention pooling (functional.attention_pool_gated, the gated kernels of csrc/attn_pool.hip) at 8 x 10 000 x 1024 and
at the reference's bag, 8 x 2 500 x 1024, D = 128: HIP events around every call, `--warmup` untimed and `--steps` timed calls each,
medians.

  gated_pool_fwd / _bwd   the two gated C entry points alone, buffers allocated outside the timed call; bytes per second over the bytes
                          that must move - x once plus h2 (2 D columns) once per kernel, B N (L + 2 D) 4; the backward also writes
                          dpre [B, N, 2 D]: its rate is given without and with that write
  plain_pool_fwd / _bwd   the plain pooling kernels in the same run, over B N (L + D) 4 bytes: the yardstick
  composed_*              the gated pooling, hidden layer included, from operations that need none of the gated code: two linear calls
                          without activation, ATen tanh / sigmoid / mul, linear with one output column, softmax_rows, matmul4 with M = 1
  fused_*                 the same from linear's tanh | sigmoid epilogue (one product over x for both gates) and attention_pool_gated
                          with hidden = (Wv, bv, Wu, bu); same leaves, same upstream gradient
  gated_abmil_step        the whole module (ABMIL with abmil_gated): forward, backward, one Adam step
The 8 x 2 500 bag (82 MB) fits the 256 MiB Infinity Cache, so back-to-back calls re-read it on die: its rates are not HBM rates.
Writes one JSON line to stdout and to --out.  Needs the GPU: there is no CPU form of these kernels."""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
smml = importlib.import_module("subspace-multimodal-learning_amd")
from bench_abmil import timed          # noqa: E402

Fh = smml.functional
NAMES = ("wv", "bv", "wu", "bu", "w", "b")


def composed(x, wv, bv, wu, bu, w, b):
    B, N, L = x.shape
    g = torch.tanh(Fh.linear(x, wv, bv)) * torch.sigmoid(Fh.linear(x, wu, bu))
    A = Fh.softmax_rows(Fh.linear(g, w, b).view(B, N))
    return Fh.matmul4(A.view(B, 1, 1, N), x.view(B, 1, N, L)).view(B, L)


def fused(x, wv, bv, wu, bu, w, b):
    with torch.no_grad():
        h2 = Fh.linear(x, torch.cat((wv, wu)), torch.cat((bv, bu)), act=Fh.ACT_TANH_SIGMOID)
    return Fh.attention_pool_gated(x, h2, w, b, hidden=(wv, bv, wu, bu))


def bench_shape(B, N, dev, warmup, steps):
    L, D = 1024, 128
    capi, lib = Fh.capi, smml.lib()
    x = smml.synth.bag(B, N, L, 42, "bench_gated_abmil:bag").to(dev)
    model = smml.ABMIL(argparse.Namespace(label_dim=4, path_dim=128, abmil_gated=True)).to(dev)
    model.load_state_dict({k: v.to(dev) for k, v in smml.synth.fill_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, 42,
                                                                           "bench_gated_abmil").items()})
    v, u, o = model.attention_V[0], model.attention_U[0], model.attention_out
    with torch.no_grad():
        h2 = Fh.linear(x, torch.cat((v.weight, u.weight)), torch.cat((v.bias, u.bias)), act=Fh.ACT_TANH_SIGMOID)
        h = h2[..., :D].contiguous()
    w, b = o.weight.detach().reshape(D).contiguous(), o.bias.detach().contiguous()
    dM = smml.synth.normal((B, L), 42, "bench_gated_abmil:dM").to(dev)
    res = {"shape": [B, N, L], "hidden": D, "x_bytes": 4 * B * N * L, "h2_bytes": 4 * B * N * 2 * D}

    # the entry points alone: gated, and the plain ones beside them
    s, M, lse = torch.empty(B, N, device=dev), torch.empty(B, L, device=dev), torch.empty(B, device=dev)
    fb, bb = lib.smml_attn_pool_fwd_workspace_bytes(B, N, L, 0), lib.smml_attn_pool_bwd_workspace_bytes(B, N, D, 0)
    ws = torch.empty((max(fb, bb) + 3) // 4, device=dev)
    dh2, dh, dw, db = torch.empty_like(h2), torch.empty_like(h), torch.empty(D, device=dev), torch.empty(1, device=dev)
    P = capi.fptr
    calls = {
        "gated_pool_fwd": lambda: capi.check(lib.smml_attn_pool_gated_fwd_f32(P(x), P(h2), P(w), P(b), P(s), P(M), P(lse), P(ws), fb, B, N, L, D, 0,
                                                                              capi.stream())),
        "gated_pool_bwd": lambda: capi.check(lib.smml_attn_pool_gated_bwd_f32(P(x), P(h2), P(w), P(s), P(lse), P(dM), P(dh2), P(dw), P(db), P(ws), bb,
                                                                              B, N, L, D, 0, 1, capi.stream())),
        "plain_pool_fwd": lambda: capi.check(lib.smml_attn_pool_fwd_f32(P(x), P(h), P(w), P(b), P(s), P(M), P(lse), P(ws), fb, B, N, L, D, 0,
                                                                        capi.stream())),
        "plain_pool_bwd": lambda: capi.check(lib.smml_attn_pool_bwd_f32(P(x), P(h), P(w), P(s), P(lse), P(dM), P(dh), P(dw), P(db), P(ws), bb, B, N, L,
                                                                        D, 0, 1, capi.stream())),
    }
    res["splits"] = fb // (B * (L + 4) * 4)
    for name in ("plain_pool_fwd", "plain_pool_bwd", "gated_pool_fwd", "gated_pool_bwd"):      # each backward after its own forward: s, lse match
        res[name + "_ms"] = timed(calls[name], warmup, steps)
        must = res["x_bytes"] + (res["h2_bytes"] if name.startswith("gated") else res["h2_bytes"] // 2)
        res[name + "_bytes_that_must_move"] = must
        res[name + "_bytes_per_s"] = must / (res[name + "_ms"]["median"] * 1e-3)
        if name.endswith("bwd"):
            res[name + "_bytes_per_s_with_write"] = (2 * must - res["x_bytes"]) / (res[name + "_ms"]["median"] * 1e-3)

    # fused against composed, through autograd, same leaves and the same upstream gradient
    leaves = [t.detach().clone().requires_grad_() for t in (v.weight, v.bias, u.weight, u.bias, o.weight, o.bias)]

    def fwd_bwd(pool):
        for t in leaves:
            t.grad = None
        pool(x, *leaves).backward(dM)

    with torch.no_grad():
        ref, got = composed(x, *leaves), fused(x, *leaves)
    res["fused_vs_composed_max_rel_diff"] = float((got - ref).abs().max() / ref.abs().max())
    grads = {}
    for name, pool in (("composed", composed), ("fused", fused)):
        with torch.no_grad():
            res[name + "_fwd_ms"] = timed(lambda: pool(x, *leaves), warmup, steps)
        res[name + "_fwd_bwd_ms"] = timed(lambda: fwd_bwd(pool), warmup, steps)
        grads[name] = [t.grad.clone() for t in leaves[:5]]          # without the score bias: its gradient is rounding noise around 0
    res["fused_vs_composed_grad_max_rel_diff"] = {n: float((a - c).abs().max() / c.abs().max())
                                                  for n, a, c in zip(NAMES, grads["fused"], grads["composed"])}
    res["composed_over_fused_fwd"] = res["composed_fwd_ms"]["median"] / res["fused_fwd_ms"]["median"]
    res["composed_over_fused_fwd_bwd"] = res["composed_fwd_bwd_ms"]["median"] / res["fused_fwd_bwd_ms"]["median"]

    # the whole module: forward, backward, Adam
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    label = torch.arange(B, device=dev) % 4

    def step():
        enc, logits, _ = model(x)
        loss = torch.nn.functional.cross_entropy(logits, label) + 1e-3 * enc.pow(2).mean()
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()

    res["gated_abmil_step_ms"] = timed(step, warmup, steps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bags", type=int, default=8)
    ap.add_argument("--instances", type=int, nargs="+", default=[10000, 2500])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gated_abmil_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gated_abmil needs the GPU (no CPU form of the kernels)")
    dev = torch.device("cuda", 0)
    res = {"warmup": a.warmup, "steps": a.steps, "shapes": [bench_shape(a.bags, n, dev, a.warmup, a.steps) for n in a.instances]}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
