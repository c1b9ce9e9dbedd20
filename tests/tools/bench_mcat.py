"""Times MCAT_Surv (mcat.py) at the reference's bag, 8 x 2 500 x 1024, and at 8 x 10 000 x 1024, with the extension key `mcat_fused` true
(few-query co-attention + the token-set kernels of csrc/token_set.hip) and false (the composed forms, which run only kernels the package
had before) in the same process and in alternation: HIP events around every call, `--warmup` untimed calls, then `--rounds` rounds of
`--steps` timed calls of each form, the order reversing from round to round; medians over all of a form's calls.

  eval_fwd_ms        the forward in eval() under no_grad
  train_step_ms      forward + backward + one Adam step in train() (every dropout of the model active)
  launches_per_step  GPU kernels of ONE training step, counted by torch.profiler in a step of its own after the timed ones
  token_attn_*       8-head self-attention over the 4 tokens alone, from the token rows [4, B, 256]: fused = the packed projection (one
                     linear) + functional.token_self_attention + the out-projection, composed = coattention.MultiheadAttention(256, 8)
  token_pool_*       the gated head + softmax + weighted sum alone: fused = Attn_Net_Gated.gates + functional.token_pool_gated, composed =
                     Attn_Net_Gated.forward + softmax_rows + matmul4
After the co-attention the model works on 4 tokens per bag: the host's launches, not the kernels, bound these numbers.
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


def _ms(fn, steps):
    """GPU milliseconds of `steps` calls of fn(), each from a pair of HIP events on the launch stream"""
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def timed_alternating(fns, warmup, steps, rounds):
    """{name: median / min / max ms} of the callables `fns`, measured in the same process in alternation: every round times `steps` calls
    of each, the order of the names reverses from round to round, and a name's statistics are over all its rounds - so that whatever drifts
    on the host or the device during the run meets every variant alike."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for r in range(rounds):
        for name in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            ms[name] += _ms(fns[name], steps)
    out = {}
    for name, v in ms.items():
        v.sort()
        out[name] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "calls": len(v)}
    return out


def count_launches(fn):
    """GPU kernels one call of fn() launches, from torch.profiler's device events; None where the profiler reports no device activity."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = 0
    for ev in prof.events():
        if str(getattr(ev, "device_type", "")).endswith("CUDA") and "memcpy" not in ev.name.lower() and "memset" not in ev.name.lower():
            n += 1
    return n or None


def token_parts(model, B, dev, fused):
    """fn() pairs (forward + backward) of the two token-set operations alone at the model's shape"""
    layer, head = model.path_transformer.layers[0], model.path_attention_head
    att = layer.self_attn
    tok = smml.synth.normal((4, B, 256), 42, "bench_mcat:tok").to(dev).requires_grad_()
    g_tok = smml.synth.normal((4, B, 256), 42, "bench_mcat:gtok").to(dev)
    g_m = smml.synth.normal((B, 256), 42, "bench_mcat:gm").to(dev)

    def attn():
        if fused:
            qkv = Fh.linear(tok, att.in_proj_weight, att.in_proj_bias)
            o = Fh.token_self_attention(qkv.transpose(0, 1), heads=att.num_heads).transpose(0, 1)
            return Fh.linear(o, att.out_proj.weight, att.out_proj.bias)
        return att(tok, tok, tok, need_weights=False)[0]

    def pool():
        if fused:
            xb = tok.transpose(0, 1).contiguous()
            return Fh.token_pool_gated(xb, head.gates(xb), head.attention_c.weight, head.attention_c.bias)
        A, h = head(tok)
        return Fh.matmul4(Fh.softmax_rows(A.permute(1, 2, 0)).unsqueeze(1), h.transpose(0, 1).unsqueeze(1)).reshape(B, 256)

    def fwd_bwd(f, g):
        def run():
            tok.grad = None
            model.zero_grad(set_to_none=True)
            f().backward(g)
        return run

    return attn, fwd_bwd(attn, g_tok), pool, fwd_bwd(pool, g_m)


VARIANTS = ("fused", "composed")


def bench_shape(B, N, dev, warmup, steps, rounds):
    x_path = smml.synth.bag(B, N, 1024, 42, "bench_mcat:bag").to(dev)
    x_omic = smml.synth.normal((B, 431), 42, "bench_mcat:omic").to(dev)
    w = smml.synth.normal((B, 4), 42, "bench_mcat:w").to(dev)
    res = {"shape": [B, N, 1024], "fused": {}, "composed": {}}
    models, fns, params = {}, {}, None
    for name in VARIANTS:
        model = smml.MCAT_Surv(argparse.Namespace(label_dim=4, mcat_fused=name == "fused")).to(dev)
        if params is None:
            params = {k: v.to(dev) for k, v in smml.synth.fill_params({k: tuple(v.shape) for k, v in model.state_dict().items()}, 42,
                                                                      "bench_mcat").items()}
        model.load_state_dict(params)
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)

        def fwd(model=model):
            with torch.no_grad():
                return model(x_path=x_path, x_omic=x_omic)[0]

        def step(model=model, opt=opt):
            logits = model(x_path=x_path, x_omic=x_omic)[0]
            opt.zero_grad(set_to_none=True)
            (logits * w).sum().backward()
            opt.step()

        attn, attn_fb, pool, pool_fb = token_parts(model, B, dev, name == "fused")

        def no_grad(f):
            def run():
                with torch.no_grad():
                    return f()
            return run

        models[name] = model.eval()
        fns[name] = {"eval_fwd_ms": fwd, "token_attn_fwd_ms": no_grad(attn), "token_pool_fwd_ms": no_grad(pool), "token_attn_fwd_bwd_ms": attn_fb,
                     "token_pool_fwd_bwd_ms": pool_fb, "train_step_ms": step}

    def measure(key):
        for name, t in timed_alternating({name: fns[name][key] for name in VARIANTS}, warmup, steps, rounds).items():
            res[name][key] = t

    for key in ("eval_fwd_ms", "token_attn_fwd_ms", "token_pool_fwd_ms", "token_attn_fwd_bwd_ms", "token_pool_fwd_bwd_ms"):
        measure(key)
    for name in VARIANTS:
        res[name]["eval_logits"] = fns[name]["eval_fwd_ms"]().flatten().tolist()[:4]
        models[name].train()
    torch.manual_seed(0)
    measure("train_step_ms")
    for name in VARIANTS:          # the profiled calls come after every timed one: tracing slows the host
        res[name]["launches_per_step"] = count_launches(fns[name]["train_step_ms"])
        models[name].eval()
        res[name]["launches_per_eval_fwd"] = count_launches(fns[name]["eval_fwd_ms"])
        res[name]["launches_token_attn_fwd_bwd"] = count_launches(fns[name]["token_attn_fwd_bwd_ms"])
        res[name]["launches_token_pool_fwd_bwd"] = count_launches(fns[name]["token_pool_fwd_bwd_ms"])
    res["composed_over_fused_eval_fwd"] = res["composed"]["eval_fwd_ms"]["median"] / res["fused"]["eval_fwd_ms"]["median"]
    res["composed_over_fused_train_step"] = res["composed"]["train_step_ms"]["median"] / res["fused"]["train_step_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bags", type=int, default=8)
    ap.add_argument("--instances", type=int, nargs="+", default=[2500, 10000])
    ap.add_argument("--steps", type=int, default=20, help="timed calls per variant and round")
    ap.add_argument("--rounds", type=int, default=6, help="alternations of the two variants")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mcat_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mcat needs the GPU (no CPU form of the kernels)")
    dev = torch.device("cuda", 0)
    res = {"warmup": a.warmup, "steps": a.steps, "rounds": a.rounds,
           "shapes": [bench_shape(a.bags, n, dev, a.warmup, a.steps, a.rounds) for n in a.instances]}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
