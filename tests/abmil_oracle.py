"""fp32 / fp64 oracle of the reference's ABMIL (models/mil.py:63-82) in plain torch on the CPU: a functional restatement over a
{parameter name: tensor} table, in whatever dtype the table and the bag have.  Shared by tests/golden/make_golden_abmil.py, the host
tests and the GPU parity tests (tests/test_abmil_host.py, tests/test_gpu_abmil.py)."""
import torch

from helpers import synth

PARAMS = {"attention.0.weight": (128, 1024), "attention.0.bias": (128,), "attention.2.weight": (1, 128), "attention.2.bias": (1,),
          "classifier.0.weight": (3, 1024), "classifier.0.bias": (3,), "multimodal_projection.weight": (128, 1024),
          "multimodal_projection.bias": (128,)}          # label_dim = 3, path_dim = 128: the fixture's and the tests' configuration
ZERO_GRAD = "attention.2.bias"      # softmax is shift invariant: this gradient is exactly 0 in exact arithmetic


def abmil(x, p, natural=None):
    """-> (encoded [B, path_dim], logits [B, label_dim], A [B, 1, N]).  natural: a list that receives sum |d s| once the scores' gradient
    is known - the natural scale of d attention.2.bias = sum d s."""
    h = torch.tanh(x @ p["attention.0.weight"].T + p["attention.0.bias"])
    s = h @ p["attention.2.weight"].T + p["attention.2.bias"]                  # [B, N, 1]
    if natural is not None and s.requires_grad:
        s.register_hook(lambda g: natural.append(float(g.abs().sum())))
    A = torch.softmax(s.transpose(2, 1), dim=2)                                # [B, 1, N]
    M = torch.bmm(A, x).reshape(x.shape[0], -1)
    logits = M @ p["classifier.0.weight"].T + p["classifier.0.bias"]
    encoded = M @ p["multimodal_projection.weight"].T + p["multimodal_projection.bias"]
    return encoded, logits, A


def problem(B, N, seed=42, tag="abmil"):
    """Bag, synthetic parameters and loss weights of a test problem; (2, 300, 42, 'abmil') is the golden fixture's."""
    x = synth.bag(B, N, 1024, seed, tag + ":bag")
    params = synth.fill_params(PARAMS, seed=seed, tag=tag)
    w_e = synth.normal((B, 128), seed, tag + ":we")
    w_l = synth.normal((B, 3), seed, tag + ":wl")
    return x, params, w_e, w_l


def run(x, params, w_e, w_l, dtype):
    """The oracle's outputs and gradients for loss = sum enc w_e + sum logits w_l in `dtype`:
    {'encoded', 'logits', 'softmax', 'loss', 'natural', 'grad:<name>'}."""
    p = {k: v.detach().to(dtype).clone().requires_grad_() for k, v in params.items()}
    natural = []
    enc, logits, A = abmil(x.detach().to(dtype), p, natural)
    loss = (enc * w_e.to(dtype)).sum() + (logits * w_l.to(dtype)).sum()
    loss.backward()
    out = {"encoded": enc.detach(), "logits": logits.detach(), "softmax": A.detach(), "loss": float(loss.detach()), "natural": natural[0]}
    out.update({"grad:" + k: v.grad for k, v in p.items()})
    return out
