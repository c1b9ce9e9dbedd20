"""Times the few-query co-attention (MultiheadAttention.fused_few_query, functional.few_query_attention, csrc/fewq_attn.hip) with L = 4
queries of width 256 over 8 x 10 000 keys and over the reference's bag, 8 x 2 500: HIP events around every call, `--warmup` untimed and
`--steps` timed calls each, medians.

  fewq_fwd / fewq_bwd   the two C entry points alone (x is y, gradient row written), buffers allocated outside the timed call; bytes per
                        second over the bytes that must move - forward: x once + raw; backward: x once + dx once + raw
  fused_*               the module with the flag on (forward under no_grad; forward + backward with gradients for the query, the bag and
                        the parameters)
  composed_*            the SAME module with the flag off - the path every call took before the kernels: two bag-sized projections,
                        matmul4, softmax_rows, matmul4 - the yardstick, same process, same inputs
  cmta_step             CMTA forward + backward + Adam step at the reference's 8 x 2 500 x 1024 with the extension key coattn_fused off / on
The 8 x 2 500 bag (20 MB) fits the 256 MiB Infinity Cache (the 8 x 10 000 one, 82 MB, does too, beside little else), so back-to-back calls
re-read it on die: the rates are not HBM rates.  Writes one JSON line to stdout and to --out.  Needs the GPU: there is no CPU form of these
kernels."""
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


def bench_shape(B, S, dev, warmup, steps):
    L, E = 4, 256
    capi, lib = Fh.capi, smml.lib()
    mod = smml.MultiheadAttention(E, 1)
    mod.load_state_dict(smml.synth.fill_params({k: tuple(v.shape) for k, v in mod.state_dict().items()}, 42, "bench_coattn"))
    mod = mod.to(dev).eval()
    q = smml.synth.normal((L, B, E), 42, "bench_coattn:q").to(dev)
    x = smml.synth.normal((B, S, E), 42, "bench_coattn:x").to(dev)          # the bag, batch first; the module sees its transpose, as in CMTA
    w_o = smml.synth.normal((L, B, E), 42, "bench_coattn:wo").to(dev)
    res = {"shape": [B, L, S, E], "x_bytes": 4 * B * S * E, "raw_bytes": 4 * B * L * S}

    # the two entry points alone
    with torch.no_grad():
        wq, wk, _ = mod.in_proj_weight.chunk(3, dim=0)
        bq, bk, _ = mod.in_proj_bias.chunk(3, dim=0)
        qh = Fh.linear(q.transpose(0, 1), wq, bq) * E ** -0.5
        u, c = Fh.linear(qh, wk.t()).contiguous(), Fh.linear(qh, bk.view(1, -1))[..., 0].contiguous()
    z, raw, lse = torch.empty(B, L, E, device=dev), torch.empty(B, L, S, device=dev), torch.empty(B, L, device=dev)
    fb, bb = lib.smml_fewq_attn_fwd_workspace_bytes(B, L, S, E, 0), lib.smml_fewq_attn_bwd_workspace_bytes(B, L, S, E, 0)
    ws = torch.empty((max(fb, bb) + 3) // 4, device=dev)
    dz, draw = smml.synth.normal((B, L, E), 42, "bench_coattn:dz").to(dev), smml.synth.normal((B, L, S), 42, "bench_coattn:draw").to(dev)
    du, dc, dx = torch.empty_like(u), torch.empty_like(c), torch.empty_like(x)
    fwd = lambda: capi.check(lib.smml_fewq_attn_fwd_f32(capi.fptr(u), capi.fptr(c), capi.fptr(x), capi.fptr(x), None, capi.fptr(z), capi.fptr(raw),  # noqa: E731
                                                        capi.fptr(lse), capi.fptr(ws), fb, B, L, S, E, E, S * E, E, S * E, E, 0, capi.stream()))
    bwd = lambda: capi.check(lib.smml_fewq_attn_bwd_f32(capi.fptr(u), capi.fptr(x), capi.fptr(x), capi.fptr(raw), capi.fptr(lse), capi.fptr(z),  # noqa: E731
                                                        capi.fptr(dz), capi.fptr(draw), None, capi.fptr(du), capi.fptr(dc), capi.fptr(dx), None,
                                                        capi.fptr(ws), bb, B, L, S, E, E, S * E, E, S * E, E, S * E, E, 0, 0, 0, capi.stream()))
    res["splits"] = fb // (B * L * (E + 4) * 4)
    res["fewq_fwd_ms"] = timed(fwd, warmup, steps)
    res["fewq_bwd_ms"] = timed(bwd, warmup, steps)
    res["fewq_fwd_bytes_that_must_move"] = res["x_bytes"] + res["raw_bytes"]
    res["fewq_bwd_bytes_that_must_move"] = 2 * res["x_bytes"] + res["raw_bytes"]
    res["fewq_fwd_bytes_per_s"] = res["fewq_fwd_bytes_that_must_move"] / (res["fewq_fwd_ms"]["median"] * 1e-3)
    res["fewq_bwd_bytes_per_s"] = res["fewq_bwd_bytes_that_must_move"] / (res["fewq_bwd_ms"]["median"] * 1e-3)

    # the module, flag on against flag off: same leaves, same upstream gradient
    ql, xl = q.clone().requires_grad_(), x.clone().requires_grad_()

    def call():
        kv = xl.transpose(0, 1)
        return mod(ql, kv, kv)[0]

    def fwd_bwd():
        for t in (ql, xl, *mod.parameters()):
            t.grad = None
        call().backward(w_o)

    outs, grads = {}, {}
    for name, flag in (("composed", False), ("fused", True)):
        mod.fused_few_query = flag
        with torch.no_grad():
            outs[name] = call().clone()
            res[name + "_fwd_ms"] = timed(call, warmup, steps)
        res[name + "_fwd_bwd_ms"] = timed(fwd_bwd, warmup, steps)
        grads[name] = [t.grad.clone() for t in (ql, xl, *mod.parameters())]
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())          # noqa: E731
    res["fused_vs_composed_max_rel_diff"] = rel(outs["fused"], outs["composed"])
    res["fused_vs_composed_grad_max_rel_diff"] = max(rel(a, b) for a, b in zip(grads["fused"], grads["composed"]))
    res["composed_over_fused_fwd"] = res["composed_fwd_ms"]["median"] / res["fused_fwd_ms"]["median"]
    res["composed_over_fused_fwd_bwd"] = res["composed_fwd_bwd_ms"]["median"] / res["fused_fwd_bwd_ms"]["median"]
    return res


def bench_cmta(B, N, dev, warmup, steps):
    xp = smml.synth.bag(B, N, 1024, 42, "bench_coattn:bag").to(dev)
    xo = smml.synth.normal((B, 431), 42, "bench_coattn:omic").to(dev)
    label = torch.arange(B, device=dev) % 4
    res = {"shape": [B, N, 1024]}
    for name, on in (("off", False), ("on", True)):
        torch.manual_seed(0)
        net = smml.CMTA(argparse.Namespace(label_dim=4, coattn_fused=on)).to(dev).eval()      # eval: the dropout layers would draw different masks
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)

        def step():
            out = net(x_path=xp, x_omic=xo)
            loss = torch.nn.functional.cross_entropy(out[0], label) + torch.nn.functional.l1_loss(out[3], out[4].detach()) \
                + torch.nn.functional.l1_loss(out[5], out[6].detach())
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

        res[f"cmta_step_coattn_fused_{name}_ms"] = timed(step, warmup, steps)
    res["off_over_on"] = res["cmta_step_coattn_fused_off_ms"]["median"] / res["cmta_step_coattn_fused_on_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bags", type=int, default=8)
    ap.add_argument("--keys", type=int, nargs="+", default=[10000, 2500])
    ap.add_argument("--cmta-instances", type=int, default=2500)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coattn_fewq_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_coattn needs the GPU (no CPU form of the kernels)")
    dev = torch.device("cuda", 0)
    res = {"warmup": a.warmup, "steps": a.steps, "shapes": [bench_shape(a.bags, s, dev, a.warmup, a.steps) for s in a.keys],
           "cmta": bench_cmta(a.bags, a.cmta_instances, dev, a.warmup, a.steps)}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
