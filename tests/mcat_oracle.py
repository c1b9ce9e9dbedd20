"""fp32 / fp64 oracle of the reference's MCAT_Surv.forward (models/model.py:612-666) in plain torch on the CPU: a functional restatement in
eval mode over a {parameter name: tensor} table, in whatever dtype the table and the inputs have (the reference itself cannot run in
fp64: it casts `.float()` at :639 and :650).  Shared by tests/golden/make_golden_mcat.py, the host tests and the GPU parity tests
(tests/test_mcat_host.py, tests/test_gpu_mcat.py)."""
import torch

from helpers import synth

OMIC_SIZES = (100, 100, 100, 131)
HEADS, EMBED = 8, 256


def _layer_params(prefix):
    return {prefix + "self_attn.in_proj_weight": (768, 256), prefix + "self_attn.in_proj_bias": (768,),
            prefix + "self_attn.out_proj.weight": (256, 256), prefix + "self_attn.out_proj.bias": (256,),
            prefix + "linear1.weight": (512, 256), prefix + "linear1.bias": (512,), prefix + "linear2.weight": (256, 512),
            prefix + "linear2.bias": (256,), prefix + "norm1.weight": (256,), prefix + "norm1.bias": (256,),
            prefix + "norm2.weight": (256,), prefix + "norm2.bias": (256,)}


def _branch_params(name):
    p = {}
    for i in range(2):
        p.update(_layer_params(f"{name}_transformer.layers.{i}."))
    p.update({f"{name}_attention_head.attention_a.0.weight": (256, 256), f"{name}_attention_head.attention_a.0.bias": (256,),
              f"{name}_attention_head.attention_b.0.weight": (256, 256), f"{name}_attention_head.attention_b.0.bias": (256,),
              f"{name}_attention_head.attention_c.weight": (1, 256), f"{name}_attention_head.attention_c.bias": (1,),
              f"{name}_rho.0.weight": (256, 256), f"{name}_rho.0.bias": (256,)})
    return p


def param_shapes(label_dim=4):
    """The reference's MCAT_Surv(args, fusion='concat'), small sizes, in the order of its state_dict (92 tensors)."""
    p = {"wsi_net.0.weight": (256, 1024), "wsi_net.0.bias": (256,)}
    for i, n in enumerate(OMIC_SIZES):
        p.update({f"sig_networks.{i}.0.0.weight": (256, n), f"sig_networks.{i}.0.0.bias": (256,),
                  f"sig_networks.{i}.1.0.weight": (256, 256), f"sig_networks.{i}.1.0.bias": (256,)})
    p.update({"coattn.in_proj_weight": (768, 256), "coattn.in_proj_bias": (768,), "coattn.out_proj.weight": (256, 256),
              "coattn.out_proj.bias": (256,)})
    p.update(_branch_params("path"))
    p.update(_branch_params("omic"))
    p.update({"mm.0.weight": (256, 512), "mm.0.bias": (256,), "mm.2.weight": (256, 256), "mm.2.bias": (256,),
              "classifier.weight": (label_dim, 256), "classifier.bias": (label_dim,)})
    return p


PARAMS = param_shapes()
ZERO_GRADS = ("path_attention_head.attention_c.bias", "omic_attention_head.attention_c.bias")      # softmax is shift invariant: exactly 0


def lin(x, p, name):
    return x @ p[name + ".weight"].T + p[name + ".bias"]


def attention(q, k, v, p, prefix, heads):
    """models/MultiheadAttention.py / torch.nn.MultiheadAttention, sequence first: q [L, B, E], k and v [S, B, E] ->
    (out [L, B, E], raw scaled scores [B, heads, L, S])"""
    L, B, E = q.shape
    S, hd = k.shape[0], E // heads
    w, b = p[prefix + "in_proj_weight"], p[prefix + "in_proj_bias"]
    qp = (q @ w[:E].T + b[:E]) * float(hd) ** -0.5
    kp, vp = k @ w[E:2 * E].T + b[E:2 * E], v @ w[2 * E:].T + b[2 * E:]
    split = lambda t, n: t.reshape(n, B, heads, hd).permute(1, 2, 0, 3)          # noqa: E731  [B, heads, n, hd]
    raw = split(qp, L) @ split(kp, S).transpose(-1, -2)
    o = (torch.softmax(raw, dim=-1) @ split(vp, S)).permute(2, 0, 1, 3).reshape(L, B, E)
    return lin(o, p, prefix + "out_proj"), raw


def encoder_layer(x, p, prefix, heads=HEADS):
    """torch.nn.TransformerEncoderLayer in eval mode: post-norm, relu.  x [T, B, E]"""
    ln = lambda t, n: torch.nn.functional.layer_norm(t, (t.shape[-1],), p[prefix + n + ".weight"], p[prefix + n + ".bias"], 1e-5)      # noqa: E731
    x = ln(x + attention(x, x, x, p, prefix + "self_attn.", heads)[0], "norm1")
    return ln(x + lin(torch.relu(lin(x, p, prefix + "linear1")), p, prefix + "linear2"), "norm2")


def gated_scores(x, p, head):
    a = torch.tanh(lin(x, p, head + ".attention_a.0"))
    b = torch.sigmoid(lin(x, p, head + ".attention_b.0"))
    return lin(a * b, p, head + ".attention_c")


def branch(tokens, p, name, natural=None):
    """tokens [4, B, 256] -> (h [B, 256], raw head scores A [B, 1, 4]): two encoder layers, the gated head, softmax over the tokens, bmm, rho"""
    h = tokens
    for i in range(2):
        h = encoder_layer(h, p, f"{name}_transformer.layers.{i}.")
    A = gated_scores(h, p, name + "_attention_head")                               # [4, B, 1]
    if natural is not None and A.requires_grad:
        A.register_hook(lambda g: natural.__setitem__(name, float(g.abs().sum())))
    A = A.permute(1, 2, 0)                                                         # [B, 1, 4]
    pooled = torch.bmm(torch.softmax(A, dim=2), h.transpose(0, 1))                 # [B, 1, 256]
    return torch.relu(lin(pooled, p, name + "_rho.0")).reshape(tokens.shape[1], -1), A


def mcat(x_path, x_omic, p, natural=None):
    """-> {'logits', 'hazards', 'S' [B, label_dim], 'A_coattn' [B, 1, 4, N] raw, 'A_path', 'A_omic' [B, 1, 4] raw}"""
    edges = [sum(OMIC_SIZES[:i]) for i in range(len(OMIC_SIZES) + 1)]
    bag = torch.relu(lin(x_path, p, "wsi_net.0")).transpose(0, 1)                  # [N, B, 256]
    toks = []
    for i in range(len(OMIC_SIZES)):
        h = x_omic[:, edges[i]:edges[i + 1]]
        for j in range(2):
            h = torch.nn.functional.elu(lin(h, p, f"sig_networks.{i}.{j}.0"))
        toks.append(h)
    omic = torch.stack(toks)                                                       # [4, B, 256]
    co, A_coattn = attention(omic, bag, bag, p, "coattn.", 1)
    h_path, A_path = branch(co, p, "path", natural)
    h_omic, A_omic = branch(omic, p, "omic", natural)
    h = torch.relu(lin(torch.relu(lin(torch.cat((h_path, h_omic), dim=1), p, "mm.0")), p, "mm.2"))
    logits = lin(h, p, "classifier")
    hazards = torch.sigmoid(logits)
    return {"logits": logits, "hazards": hazards, "S": torch.cumprod(1 - hazards, dim=1), "A_coattn": A_coattn, "A_path": A_path,
            "A_omic": A_omic}


OUTPUTS = ("logits", "hazards", "S", "A_coattn", "A_path", "A_omic")


def problem(B=2, N=150, seed=42, tag="mcat", label_dim=4):
    """Bag, omic vector, synthetic parameters and loss weights: (2, 150, 42, 'mcat') is the golden fixture's."""
    x_path = synth.bag(B, N, 1024, seed, tag + ":bag")
    x_omic = synth.normal((B, sum(OMIC_SIZES)), seed, tag + ":omic")
    params = synth.fill_params(param_shapes(label_dim), seed=seed, tag=tag)
    w = synth.normal((B, label_dim), seed, tag + ":w")
    return x_path, x_omic, params, w


def run(x_path, x_omic, params, w, dtype):
    """Outputs and gradients for loss = sum logits w in `dtype`: the OUTPUTS, 'loss', 'dx_path', 'dx_omic', 'grad:<name>' and
    'natural:<name>' = sum |d scores| of the two gated heads (the natural scale of their score bias's vanishing gradient)."""
    p = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in params.items()}
    xp, xo = x_path.detach().to(dtype).requires_grad_(), x_omic.detach().to(dtype).requires_grad_()
    natural = {}
    out = mcat(xp, xo, p, natural)
    loss = (out["logits"] * w.to(dtype)).sum()
    loss.backward()
    res = {k: v.detach() for k, v in out.items()}
    res.update(loss=float(loss.detach()), dx_path=xp.grad, dx_omic=xo.grad)
    res.update({"grad:" + k: v.grad for k, v in p.items()})
    res.update({f"natural:{name}_attention_head.attention_c.bias": natural[name] for name in ("path", "omic")})
    return res
