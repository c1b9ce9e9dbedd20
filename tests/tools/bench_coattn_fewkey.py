"""Times the few-key co-attention (MultiheadAttention.fused_few_key, functional.few_key_attention, csrc/fewk_attn.hip): a bag of L queries of
width 256 over S = 4 keys, at 8 x 10 000 and at the reference's bag, 8 x 2 500.  HIP events around every call, `--warmup` untimed and
`--steps` timed calls each, medians; fused and composed take turns call by call inside one timed loop, so both see the same machine.

  fewk_fwd / fewk_bwd   the two C entry points alone (dx written, draw given), buffers allocated outside the timed call; bytes per second
                        over the bytes that must move - forward: x once + out once + raw; backward: x, dout and dx once + raw
  fused_*               the module with the flag on (forward under no_grad; forward + backward with gradients for the bag, the keys and
                        the parameters)
  composed_*            the SAME module with the flag off - two bag-sized projections, matmul4, softmax_rows, matmul4 - the yardstick,
                        same process, same inputs
  cmta_step             CMTA forward + backward + Adam step at the reference's 8 x 2 500 x 1024 with no extension key, with coattn_fused
                        alone and with coattn_fused and coattn_fused_few_key
The 8 x 10 000 bag is 82 MB and its output another 82 MB: back-to-back calls find part of them in the 256 MiB Infinity Cache, so the rates
are what a training step sees, not pure HBM rates.  Writes one JSON line to stdout and to --out.  Needs the GPU: there is no CPU form of
these kernels."""
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


def stats(ms):
    ms = sorted(ms)
    return {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}


def timed(fns, warmup, steps):
    """name -> median / min / max GPU milliseconds of each fns[name]() from HIP events on the launch stream; the functions take turns."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(steps):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {name: stats(v) for name, v in ms.items()}


def bench_shape(B, L, dev, warmup, steps):
    S, E = 4, 256
    capi = Fh.capi
    tag = "bench_coattn_fewkey"
    mods = {}
    for name, flag in (("composed", False), ("fused", True)):
        mod = smml.MultiheadAttention(E, 1)
        mod.load_state_dict(smml.synth.fill_params({k: tuple(v.shape) for k, v in mod.state_dict().items()}, 42, tag))
        mod.fused_few_key = flag
        mods[name] = mod.to(dev).eval()
    x = smml.synth.normal((B, L, E), 42, tag + ":x").to(dev)              # the bag, batch first; the module sees its transpose, as in CMTA
    kv = smml.synth.normal((S, B, E), 42, tag + ":kv").to(dev)
    w_o = smml.synth.normal((L, B, E), 42, tag + ":wo").to(dev)
    res = {"shape": [B, L, S, E], "x_bytes": 4 * B * L * E, "out_bytes": 4 * B * L * E, "raw_bytes": 4 * B * L * S}

    # the two entry points alone
    u, w = (smml.synth.normal((B, S, E), 42, tag + t).to(dev) * 0.1 for t in (":u", ":w"))
    c = smml.synth.normal((B, S), 42, tag + ":c").to(dev)
    out, raw = torch.empty(B, L, E, device=dev), torch.empty(B, L, S, device=dev)
    dout, draw = smml.synth.normal((B, L, E), 42, tag + ":dout").to(dev), smml.synth.normal((B, L, S), 42, tag + ":draw").to(dev)
    dx, du, dc, dw = torch.empty_like(x), torch.empty_like(u), torch.empty_like(c), torch.empty_like(w)
    dims = dict(B=B, L=L, S=S, Eq=E, Eo=E, splits=0)
    wsb = capi.call("smml_fewk_attn_bwd_workspace_bytes", dims)
    ws = torch.empty((wsb + 3) // 4, device=dev)
    base = dict(dims, x=x, u=u, w=w, x_batch_stride=L * E, x_row_stride=E, stream=capi.stream())
    fwd_ns = dict(base, c=c, key_padding_mask=None, out=out, raw=raw, workspace=None, workspace_bytes=0)
    bwd_ns = dict(base, raw=raw, dout=dout, draw=draw, dx=dx, du=du, dc=dc, dw=dw, workspace=ws, workspace_bytes=wsb, dout_batch_stride=L * E,
                  dout_row_stride=E, dx_batch_stride=L * E, dx_row_stride=E)
    core = timed({"fewk_fwd": lambda: capi.check(capi.call("smml_fewk_attn_fwd_f32", fwd_ns, Fh.FEWK_FWD_KEYS)),
                  "fewk_bwd": lambda: capi.check(capi.call("smml_fewk_attn_bwd_f32", bwd_ns, Fh.FEWK_BWD_KEYS))}, warmup, steps)
    res["splits"] = wsb // (B * S * (2 * E + 4) * 4)
    res["fewk_fwd_ms"], res["fewk_bwd_ms"] = core["fewk_fwd"], core["fewk_bwd"]
    res["fewk_fwd_bytes_that_must_move"] = res["x_bytes"] + res["out_bytes"] + res["raw_bytes"]
    res["fewk_bwd_bytes_that_must_move"] = 3 * res["x_bytes"] + res["raw_bytes"]
    res["fewk_fwd_bytes_per_s"] = res["fewk_fwd_bytes_that_must_move"] / (res["fewk_fwd_ms"]["median"] * 1e-3)
    res["fewk_bwd_bytes_per_s"] = res["fewk_bwd_bytes_that_must_move"] / (res["fewk_bwd_ms"]["median"] * 1e-3)

    # the module, flag on against flag off: same leaves, same upstream gradient, call by call in turn
    xl, kl = x.clone().requires_grad_(), kv.clone().requires_grad_()

    def call(name):
        return mods[name](xl.transpose(0, 1), kl, kl)[0]

    def fwd_bwd(name):
        for t in (xl, kl, *mods[name].parameters()):
            t.grad = None
        call(name).backward(w_o)

    outs, grads = {}, {}
    with torch.no_grad():
        for name in mods:
            outs[name] = call(name).clone()
        t_fwd = timed({name: (lambda n=name: call(n)) for name in mods}, warmup, steps)
    t_fb = timed({name: (lambda n=name: fwd_bwd(n)) for name in mods}, warmup, steps)
    for name in mods:
        fwd_bwd(name)
        grads[name] = [t.grad.clone() for t in (xl, kl, *mods[name].parameters())]
        res[name + "_fwd_ms"], res[name + "_fwd_bwd_ms"] = t_fwd[name], t_fb[name]
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
    fns = {}
    for name, keys in (("composed", {}), ("few_query", dict(coattn_fused=True)), ("both", dict(coattn_fused=True, coattn_fused_few_key=True))):
        torch.manual_seed(0)
        net = smml.CMTA(argparse.Namespace(label_dim=4, **keys)).to(dev).eval()      # eval: the dropout layers would draw different masks
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)

        def step(net=net, opt=opt):
            out = net(x_path=xp, x_omic=xo)
            loss = torch.nn.functional.cross_entropy(out[0], label) + torch.nn.functional.l1_loss(out[3], out[4].detach()) \
                + torch.nn.functional.l1_loss(out[5], out[6].detach())
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()

        fns[name] = step
    for name, t in timed(fns, warmup, steps).items():
        res[f"cmta_step_{name}_ms"] = t
    res["composed_over_both"] = res["cmta_step_composed_ms"]["median"] / res["cmta_step_both_ms"]["median"]
    res["few_query_over_both"] = res["cmta_step_few_query_ms"]["median"] / res["cmta_step_both_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bags", type=int, default=8)
    ap.add_argument("--rows", type=int, nargs="+", default=[10000, 2500])
    ap.add_argument("--cmta-instances", type=int, default=2500)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coattn_fewkey_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_coattn_fewkey needs the GPU (no CPU form of the kernels)")
    dev = torch.device("cuda", 0)
    res = {"warmup": a.warmup, "steps": a.steps, "shapes": [bench_shape(a.bags, n, dev, a.warmup, a.steps) for n in a.rows],
           "cmta": bench_cmta(a.bags, a.cmta_instances, dev, a.warmup, a.steps) if a.cmta_instances else None}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
