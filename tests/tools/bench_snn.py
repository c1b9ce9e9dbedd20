"""Times the self-normalising (SNN) omic encoders with the extension key `snn_fused` on (functional.snn_stack, csrc/snn_stack.hip: every
encoder of a model in one forward launch and two backward launches) and off (a linear, an ELU and an AlphaDropout per layer - what the
package ran before the key existed) in the same process and in alternation, as tests/tools/bench_mcat.py does (its timed_alternating and
count_launches are used as they are): `--warmup` untimed calls, then `--rounds` rounds of `--steps` timed calls of each form, the order
reversing from round to round; medians over all of a form's calls.

  parts    the SNN part ALONE at B = 8, in train mode (AlphaDropout active): `mcat` = the 4 sig_networks [100|100|100|131 -> 256 -> 256] on the
           column views of x_omic, stacked to [4, B, 256]; `maxnet_pair` = DeformPathomicNet's two MaxNet encoders [59|361 -> 64 -> 48 -> 32 -> 128]
           with the ReLU.  launches_fwd_bwd: GPU kernels of one forward + torch.autograd.grad over all weights and biases (torch.profiler);
           launches_eval_fwd: of one forward in eval(); fwd_ms / fwd_bwd_ms: the eval forward under no_grad and the train-mode forward +
           gradients, i.e. the two entry points with their host side (HIP events: at this size the host's enqueue, not the device, sets
           them); kernel_us: the device time of each of the three kernels in one train-mode call, from torch.profiler's device events
  shapes   a whole MCAT_Surv (everything else at its defaults) at 8 x 2 500 x 1024 and 8 x 10 000 x 1024: eval forward and training step
           (forward + backward + Adam, every dropout active), median times and GPU kernels per call
Writes one JSON line to stdout and to --out.  Needs the GPU: there is no CPU form of these kernels."""
import argparse
import importlib
import json
import os
import re
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_mcat import ROOT, count_launches, smml, timed_alternating  # noqa: E402

cmta = importlib.import_module(smml.__name__ + ".cmta")
VARIANTS = ("snn_fused", "composed")


def _fill(mod, dev, tag):
    mod.load_state_dict(smml.synth.fill_params({k: tuple(v.shape) for k, v in mod.state_dict().items()}, 42, tag))
    return mod.to(dev)


def snn_part(kind, B, dev):
    """{variant: (forward(), the modules, the parameters)} of the SNN part alone"""
    if kind == "mcat":
        model = _fill(smml.MCAT_Surv(argparse.Namespace(label_dim=4)), dev, "bench_snn:mcat")
        nets = model.sig_networks
        x_all = smml.synth.normal((B, 431), 42, "bench_snn:omic").to(dev)
        cuts = [0, 100, 200, 300, 431]
        xs = [x_all[:, a:b] for a, b in zip(cuts, cuts[1:])]
        forward = {name: (lambda fused=name == "snn_fused": (cmta._sig_tokens(nets, xs, nets.training, fused),)) for name in VARIANTS}
    else:
        nets = torch.nn.ModuleList([_fill(smml.MaxNet(input_dim=k, omic_dim=128, dropout_rate=0.25, label_dim=4), dev, f"bench_snn:maxnet{k}")
                                    for k in (59, 361)])
        xs = [smml.synth.normal((B, k), 42, f"bench_snn:x{k}").to(dev) for k in (59, 361)]
        forward = {"snn_fused": lambda: cmta._snn_fused([n.encoder for n in nets], xs, nets.training, final_relu=True),
                   "composed": lambda: tuple(n.encode(x) for n, x in zip(nets, xs))}
    params = [p for n in nets for p in (n.parameters() if kind == "mcat" else n.encoder.parameters())]
    return forward, nets, params


def kernel_times(fn):
    """{kernel: device microseconds} of the SNN kernels one call of fn() launches (torch.profiler's device events)"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.events():
        m = re.search(r"snn_\w+_kernel", ev.name)
        if m and str(getattr(ev, "device_type", "")).endswith("CUDA"):
            out[m.group(0)] = out.get(m.group(0), 0.0) + ev.time_range.elapsed_us()
    return out


def bench_part(kind, B, dev, warmup, steps, rounds):
    forward, nets, params = snn_part(kind, B, dev)
    nets.train()
    gs = [torch.ones_like(o) for o in forward["composed"]()]

    def fwd_bwd(name):
        def run():
            return torch.autograd.grad(forward[name](), params, gs)
        return run

    def fwd(name):
        def run():
            with torch.no_grad():
                return forward[name]()
        return run

    res = {"B": B, **{name: {} for name in VARIANTS}}
    for name, t in timed_alternating({name: fwd_bwd(name) for name in VARIANTS}, warmup, steps, rounds).items():
        res[name]["fwd_bwd_ms"] = t
    nets.eval()
    for name, t in timed_alternating({name: fwd(name) for name in VARIANTS}, warmup, steps, rounds).items():
        res[name]["fwd_ms"] = t
    for name in VARIANTS:          # the profiled calls come after every timed one: tracing slows the host
        res[name]["launches_eval_fwd"] = count_launches(fwd(name))
        nets.train()
        res[name]["launches_fwd_bwd"] = count_launches(fwd_bwd(name))
        nets.eval()
    nets.train()
    res["snn_fused"]["kernel_us"] = kernel_times(fwd_bwd("snn_fused"))
    nets.eval()
    # what the design fixes: one draw of the multipliers, one forward launch and two backward launches
    n_train, n_eval = res["snn_fused"]["launches_fwd_bwd"], res["snn_fused"]["launches_eval_fwd"]
    if n_train is not None and n_train > 4 or n_eval is not None and n_eval > 3:
        raise SystemExit(f"bench_snn: the fused SNN part `{kind}` launched {n_train} kernels in train mode (at most 4) and {n_eval} in eval (at most 3)")
    return res


def bench_model(B, N, dev, warmup, steps, rounds):
    x_path = smml.synth.bag(B, N, 1024, 42, "bench_mcat:bag").to(dev)
    x_omic = smml.synth.normal((B, 431), 42, "bench_mcat:omic").to(dev)
    w = smml.synth.normal((B, 4), 42, "bench_mcat:w").to(dev)
    res = {"shape": [B, N, 1024], **{name: {} for name in VARIANTS}}
    models, fns = {}, {}
    for name in VARIANTS:
        model = _fill(smml.MCAT_Surv(argparse.Namespace(label_dim=4, snn_fused=name == "snn_fused")), dev, "bench_mcat")
        opt = torch.optim.Adam(model.parameters(), lr=1e-4)

        def fwd(model=model):
            with torch.no_grad():
                return model(x_path=x_path, x_omic=x_omic)[0]

        def step(model=model, opt=opt):
            logits = model(x_path=x_path, x_omic=x_omic)[0]
            opt.zero_grad(set_to_none=True)
            (logits * w).sum().backward()
            opt.step()

        models[name], fns[name] = model.eval(), {"eval_fwd_ms": fwd, "train_step_ms": step}
    for name, t in timed_alternating({name: fns[name]["eval_fwd_ms"] for name in VARIANTS}, warmup, steps, rounds).items():
        res[name]["eval_fwd_ms"] = t
    for name in VARIANTS:
        res[name]["eval_logits"] = fns[name]["eval_fwd_ms"]().flatten().tolist()[:4]
        models[name].train()
    torch.manual_seed(0)
    for name, t in timed_alternating({name: fns[name]["train_step_ms"] for name in VARIANTS}, warmup, steps, rounds).items():
        res[name]["train_step_ms"] = t
    for name in VARIANTS:
        res[name]["launches_per_step"] = count_launches(fns[name]["train_step_ms"])
        models[name].eval()
        res[name]["launches_per_eval_fwd"] = count_launches(fns[name]["eval_fwd_ms"])
    res["composed_over_fused_eval_fwd"] = res["composed"]["eval_fwd_ms"]["median"] / res["snn_fused"]["eval_fwd_ms"]["median"]
    res["composed_over_fused_train_step"] = res["composed"]["train_step_ms"]["median"] / res["snn_fused"]["train_step_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bags", type=int, default=8)
    ap.add_argument("--instances", type=int, nargs="+", default=[2500, 10000])
    ap.add_argument("--steps", type=int, default=20, help="timed calls per variant and round")
    ap.add_argument("--rounds", type=int, default=6, help="alternations of the two variants")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snn_encoder_bench.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_snn needs the GPU (no CPU form of the kernels)")
    dev = torch.device("cuda", 0)
    res = {"warmup": a.warmup, "steps": a.steps, "rounds": a.rounds,
           "parts": {kind: bench_part(kind, a.bags, dev, a.warmup, a.steps, a.rounds) for kind in ("mcat", "maxnet_pair")},
           "shapes": [bench_model(a.bags, n, dev, a.warmup, a.steps, a.rounds) for n in a.instances]}
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
