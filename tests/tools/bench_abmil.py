"""Times ABMIL's attention pooling (functional.attention_pool, csrc/attn_pool.hip) at 8 x 10 000 x 1024 and at the reference's bag,
8 x 2 500 x 1024: HIP events around every call, `--warmup` untimed and `--steps` timed calls each, medians.

  pool_fwd / pool_bwd   the two C entry points alone, buffers allocated outside the timed call; bytes per second over the bytes that must
                        move - x once plus H once per kernel (the backward also writes dH: reported beside it, not counted)
  fused_*               attention_pool through autograd with h as an ordinary input (forward; forward + backward)
  composed_*            the same pooling from what the package offered before the kernels: linear with one output column for the scores,
                        softmax_rows, matmul4 with M = 1 for the weighted sum - the yardstick, same inputs, same gradients (dh, dw2, db2)
  abmil_step            the whole module: forward, backward, one Adam step
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


def composed_pool(x, h, w2, b2):
    B, N, L = x.shape
    s = Fh.linear(h, w2, b2)                                                 # [B, N, 1]: a product with one output column
    A = Fh.softmax_rows(s.view(B, N))
    return Fh.matmul4(A.view(B, 1, 1, N), x.view(B, 1, N, L)).view(B, L)     # M = 1 per bag


def bench_shape(B, N, dev, warmup, steps):
    L, D = 1024, 128
    capi, lib = Fh.capi, smml.lib()
    x = smml.synth.bag(B, N, L, 42, "bench_abmil:bag").to(dev)
    args = argparse.Namespace(label_dim=4, path_dim=128)
    model = smml.ABMIL(args).to(dev)
    model.load_state_dict({k: v.to(dev) for k, v in smml.synth.fill_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, 42,
                                                                           "bench_abmil").items()})
    a0, a2 = model.attention[0], model.attention[2]
    with torch.no_grad():
        h = Fh.linear(x, a0.weight, a0.bias, act=Fh.ACT_TANH)
    w2, b2 = a2.weight.detach().reshape(D).contiguous(), a2.bias.detach().contiguous()
    dM = smml.synth.normal((B, L), 42, "bench_abmil:dM").to(dev)
    res = {"shape": [B, N, L], "hidden": D, "x_bytes": 4 * B * N * L, "h_bytes": 4 * B * N * D}

    # the two entry points alone
    s, M, lse = torch.empty(B, N, device=dev), torch.empty(B, L, device=dev), torch.empty(B, device=dev)
    fb, bb = lib.smml_attn_pool_fwd_workspace_bytes(B, N, L, 0), lib.smml_attn_pool_bwd_workspace_bytes(B, N, D, 0)
    ws = torch.empty((max(fb, bb) + 3) // 4, device=dev)
    dh, dw2, db2 = torch.empty_like(h), torch.empty(D, device=dev), torch.empty(1, device=dev)
    fwd = lambda: capi.check(lib.smml_attn_pool_fwd_f32(capi.fptr(x), capi.fptr(h), capi.fptr(w2), capi.fptr(b2), capi.fptr(s), capi.fptr(M),
                                                        capi.fptr(lse), capi.fptr(ws), fb, B, N, L, D, 0, capi.stream()))
    bwd = lambda: capi.check(lib.smml_attn_pool_bwd_f32(capi.fptr(x), capi.fptr(h), capi.fptr(w2), capi.fptr(s), capi.fptr(lse),
                                                        capi.fptr(dM), capi.fptr(dh), capi.fptr(dw2), capi.fptr(db2), capi.fptr(ws), bb, B, N, L, D,
                                                        0, 1, capi.stream()))
    must = res["x_bytes"] + res["h_bytes"]
    res["splits"] = fb // (B * (L + 4) * 4)
    res["pool_fwd_ms"] = timed(fwd, warmup, steps)
    res["pool_bwd_ms"] = timed(bwd, warmup, steps)
    res["pool_bytes_that_must_move"] = must
    res["pool_fwd_bytes_per_s"] = must / (res["pool_fwd_ms"]["median"] * 1e-3)
    res["pool_bwd_bytes_per_s"] = must / (res["pool_bwd_ms"]["median"] * 1e-3)
    res["pool_bwd_bytes_per_s_with_dh_write"] = (must + res["h_bytes"]) / (res["pool_bwd_ms"]["median"] * 1e-3)

    # fused against composed, through autograd, same leaves and the same upstream gradient
    hl, w2l, b2l = h.clone().requires_grad_(), a2.weight.detach().clone().requires_grad_(), a2.bias.detach().clone().requires_grad_()

    def fwd_bwd(pool):
        for t in (hl, w2l, b2l):
            t.grad = None
        pool(x, hl, w2l, b2l).backward(dM)

    with torch.no_grad():
        ref, got = composed_pool(x, hl, w2l, b2l), Fh.attention_pool(x, hl, w2l, b2l)
    res["fused_vs_composed_max_rel_diff"] = float((got - ref).abs().max() / ref.abs().max())
    grads = {}
    for name, pool in (("composed", composed_pool), ("fused", Fh.attention_pool)):
        with torch.no_grad():
            res[name + "_fwd_ms"] = timed(lambda: pool(x, hl, w2l, b2l), warmup, steps)
        res[name + "_fwd_bwd_ms"] = timed(lambda: fwd_bwd(pool), warmup, steps)
        grads[name] = [t.grad.clone() for t in (hl, w2l)]
    res["fused_vs_composed_grad_max_rel_diff"] = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(grads["fused"], grads["composed"]))
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

    res["abmil_step_ms"] = timed(step, warmup, steps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bags", type=int, default=8)
    ap.add_argument("--instances", type=int, nargs="+", default=[10000, 2500])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "abmil_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_abmil needs the GPU (no CPU form of the kernels)")
    dev = torch.device("cuda", 0)
    res = {"warmup": a.warmup, "steps": a.steps, "shapes": [bench_shape(a.bags, n, dev, a.warmup, a.steps) for n in a.instances]}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
