"""fp32 / fp64 oracle of the reference's GatedABMIL (models/mil.py:129-152) in plain torch on the CPU: a functional restatement over a
{parameter name: tensor} table, in whatever dtype the table and the bag have.  Two forms share the gated pooling: the reference's own
forward and loss (one bag, B = 1), and the batched (encoded, logits) form of ABMIL with the extension key `abmil_gated`.  Shared by
tests/golden/make_golden_gated_abmil.py, the host tests and the GPU parity tests (tests/test_gated_abmil_host.py,
tests/test_gpu_gated_abmil.py)."""
import torch

from helpers import synth

PARAMS = {"attention_V.0.weight": (128, 1024), "attention_V.0.bias": (128,), "attention_U.0.weight": (128, 1024), "attention_U.0.bias": (128,),
          "attention_weights.weight": (1, 128), "attention_weights.bias": (1,), "classifier.0.weight": (2, 1024),
          "classifier.0.bias": (2,)}          # the reference's GatedABMIL, in the order of its state_dict
ZERO_GRAD = "attention_weights.bias"      # softmax is shift invariant: this gradient is exactly 0 in exact arithmetic

# ABMIL(args) with abmil_gated: label_dim = 3, path_dim = 128, the configuration of tests/abmil_oracle.py
NET_PARAMS = {"attention_V.0.weight": (128, 1024), "attention_V.0.bias": (128,), "attention_U.0.weight": (128, 1024),
              "attention_U.0.bias": (128,), "attention_out.weight": (1, 128), "attention_out.bias": (1,), "classifier.0.weight": (3, 1024),
              "classifier.0.bias": (3,), "multimodal_projection.weight": (128, 1024), "multimodal_projection.bias": (128,)}
NET_ZERO_GRAD = "attention_out.bias"


def gated_pool(x, p, out="attention_weights", natural=None):
    """x [B, N, L] -> (M [B, L], A [B, 1, N]).  natural: a list that receives sum |d s| once the scores' gradient is known - the natural
    scale of the score bias's gradient sum d s."""
    hv = torch.tanh(x @ p["attention_V.0.weight"].T + p["attention_V.0.bias"])
    hu = torch.sigmoid(x @ p["attention_U.0.weight"].T + p["attention_U.0.bias"])
    s = (hv * hu) @ p[out + ".weight"].T + p[out + ".bias"]                    # [B, N, 1]
    if natural is not None and s.requires_grad:
        s.register_hook(lambda g: natural.append(float(g.abs().sum())))
    A = torch.softmax(s.transpose(2, 1), dim=2)                                # [B, 1, N]
    return torch.bmm(A, x).reshape(x.shape[0], -1), A


def gated_abmil(x, p, labels, natural=None):
    """The reference's forward and loss for ONE bag x [1, N, L]: -> (prob [1, 2], loss, A [1, 1, N]); the loss is CrossEntropyLoss on the
    sigmoid probabilities, as models/mil.py:142-150 has it."""
    assert x.shape[0] == 1
    M, A = gated_pool(x, p, "attention_weights", natural)
    prob = torch.sigmoid(M @ p["classifier.0.weight"].T + p["classifier.0.bias"])
    return prob, torch.nn.functional.cross_entropy(prob, labels), A


def gated_net(x, p, natural=None):
    """ABMIL with abmil_gated, batched: -> (encoded [B, path_dim], logits [B, label_dim], A [B, 1, N])"""
    M, A = gated_pool(x, p, "attention_out", natural)
    logits = M @ p["classifier.0.weight"].T + p["classifier.0.bias"]
    encoded = M @ p["multimodal_projection.weight"].T + p["multimodal_projection.bias"]
    return encoded, logits, A


def problem(B, N, seed=42, tag="gated_abmil"):
    """Bag, synthetic parameters of the module form and loss weights of a test problem.  The bag of (1, 300, 42, 'gated_abmil') is the
    golden fixture's; `reference_problem` is the fixture's whole problem."""
    x = synth.bag(B, N, 1024, seed, tag + ":bag")
    params = synth.fill_params(NET_PARAMS, seed=seed, tag=tag)
    w_e = synth.normal((B, 128), seed, tag + ":we")
    w_l = synth.normal((B, 3), seed, tag + ":wl")
    return x, params, w_e, w_l


def reference_problem(N=300, seed=42, tag="gated_abmil"):
    """One bag, the synthetic parameters of the reference's class and its label: (300, 42, 'gated_abmil') is the golden fixture's."""
    return synth.bag(1, N, 1024, seed, tag + ":bag"), synth.fill_params(PARAMS, seed=seed, tag=tag), torch.tensor([1])


def _grads(out, p, natural):
    out["natural"] = natural[0]
    out.update({"grad:" + k: v.grad for k, v in p.items()})
    return out


def run(x, params, w_e, w_l, dtype):
    """The module form's outputs and gradients for loss = sum enc w_e + sum logits w_l in `dtype`:
    {'encoded', 'logits', 'softmax', 'loss', 'natural' = sum |d s|, 'grad:<name>'}."""
    p = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in params.items()}
    natural = []
    enc, logits, A = gated_net(x.detach().to(dtype), p, natural)
    loss = (enc * w_e.to(dtype)).sum() + (logits * w_l.to(dtype)).sum()
    loss.backward()
    return _grads({"encoded": enc.detach(), "logits": logits.detach(), "softmax": A.detach(), "loss": float(loss.detach())}, p, natural)


def run_reference(x, params, labels, dtype):
    """The reference form's outputs and gradients in `dtype`: {'prob', 'softmax', 'loss', 'natural' = sum |d s|, 'grad:<name>'}."""
    p = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in params.items()}
    natural = []
    prob, loss, A = gated_abmil(x.detach().to(dtype), p, labels, natural)
    loss.backward()
    return _grads({"prob": prob.detach(), "softmax": A.detach(), "loss": float(loss.detach())}, p, natural)
