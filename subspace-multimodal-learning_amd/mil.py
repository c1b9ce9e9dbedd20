"""Host-side mirror of the reference's attention-pooling MIL baselines:

  ABMIL        models/mil.py:34-82     attention network without gating (Linear 1024 -> 128, tanh, Linear 128 -> 1), softmax over the bag,
                                       weighted sum of the raw features, classifier and multimodal projection; mode 'path' of define_net
  GatedABMIL   models/mil.py:102-152   the gated attention of Ilse et al.: scores from tanh(x V^T) (.) sigmoid(x U^T), a two-class sigmoid
                                       classifier and its own cross-entropy loss

Same constructor arguments (ABMIL: an `args` namespace with label_dim, path_dim; GatedABMIL: none), forward signatures, return tuples and
parameter names - a reference state_dict loads with strict=True.  The hidden layer runs on the f32 matrix cores (functional.linear with a
tanh epilogue, or ONE product over the bag for both gates with the tanh | sigmoid epilogue); scores, softmax and the weighted sum are one
streaming pass over the bag (functional.attention_pool / attention_pool_gated, csrc/attn_pool.hip).  The bag is a tensor of features: it
receives no gradient (x.requires_grad makes the backward raise)."""
from __future__ import annotations

import torch
from torch import nn

from . import functional as Fh


def _gated_pool(x, v, u, out, splits, scores_out=None):
    """The gated pooling over x [B, N, L] with the gates v, u (nn.Linear L -> D) and the score layer out (nn.Linear D -> 1): x is read once
    for both gates (one GEMM with 2 D output columns), the four gate gradients come out of attention_pool_gated's backward."""
    x = x.float()
    with torch.no_grad():
        h2 = Fh.linear(x, torch.cat((v.weight, u.weight)), torch.cat((v.bias, u.bias)), act=Fh.ACT_TANH_SIGMOID)       # [B, N, 2 D]
    return Fh.attention_pool_gated(x, h2, out.weight, out.bias, hidden=(v.weight, v.bias, u.weight, u.bias), splits=splits,
                                   scores_out=scores_out)      # [B, L]


def _softmax_of(sink):
    s, lse = sink
    return torch.exp(s - lse[:, None])[:, None, :]


class ABMIL(nn.Module):
    """args.abmil_gated (an extension key, absent or false by default): the attention network becomes the gated one - `attention` is
    replaced by attention_V, attention_U (Linear L -> D with tanh / sigmoid) and attention_out (Linear D -> K); forward and
    attention_weights keep their contracts."""

    def __init__(self, args):
        super().__init__()
        self.L = 1024
        self.D = 128
        self.K = 1
        self.args = args
        self.n_classes = args.label_dim
        self.gated = bool(getattr(args, "abmil_gated", False))
        if self.gated:
            self.attention_V = nn.Sequential(nn.Linear(self.L, self.D), nn.Tanh())
            self.attention_U = nn.Sequential(nn.Linear(self.L, self.D), nn.Sigmoid())
            self.attention_out = nn.Linear(self.D, self.K)
        else:
            self.attention = nn.Sequential(nn.Linear(self.L, self.D), nn.Tanh(), nn.Linear(self.D, self.K))
        self.classifier = nn.Sequential(nn.Linear(self.L * self.K, self.n_classes))
        self.multimodal_projection = nn.Linear(self.L * self.K, self.args.path_dim)
        self.pool_splits = None          # pieces the pooling kernels cut a bag into; None: chosen by the library (tests force ragged splits)

    def _pool(self, x, scores_out=None):
        if self.gated:
            return _gated_pool(x, self.attention_V[0], self.attention_U[0], self.attention_out, self.pool_splits, scores_out)
        x = x.float()
        a0, a2 = self.attention[0], self.attention[2]
        with torch.no_grad():       # the hidden layer's gradients are formed by attention_pool's backward, from the one pass that yields d scores
            h = Fh.linear(x, a0.weight, a0.bias, act=Fh.ACT_TANH)                     # [B, N, 128]
        return Fh.attention_pool(x, h, a2.weight, a2.bias, hidden=(a0.weight, a0.bias), splits=self.pool_splits,
                                 scores_out=scores_out)    # [B, 1024]

    def forward(self, x):
        M = self._pool(x)
        logits = Fh.linear(M, self.classifier[0].weight, self.classifier[0].bias)
        encoded = Fh.linear(M, self.multimodal_projection.weight, self.multimodal_projection.bias)
        return encoded, logits, None

    def attention_weights(self, x):
        """[B, 1, N]: the softmax over the bag that forward(x) pools with (A of models/mil.py:73) - exp(s - lse) of the raw scores and the
        log-sum-exp the pooling kernel itself wrote, from one forward pass under no_grad."""
        sink = []
        with torch.no_grad():
            self._pool(x, scores_out=sink)
            return _softmax_of(sink)


class GatedABMIL(nn.Module):
    """models/mil.py:102-152.  forward takes ONE bag, as the reference does; pool and attention_map take [B, N, 1024]."""

    def __init__(self):
        super().__init__()
        self.L = 1024
        self.D = 128
        self.K = 1
        self.attention_V = nn.Sequential(nn.Linear(self.L, self.D), nn.Tanh())
        self.attention_U = nn.Sequential(nn.Linear(self.L, self.D), nn.Sigmoid())
        self.attention_weights = nn.Linear(self.D, self.K)
        self.classifier = nn.Sequential(nn.Linear(self.L * self.K, 2), nn.Sigmoid())
        self.criterion = nn.CrossEntropyLoss()
        self.pool_splits = None          # as on ABMIL

    def pool(self, x, scores_out=None):
        """x [B, N, 1024] -> M [B, 1024]"""
        return _gated_pool(x, self.attention_V[0], self.attention_U[0], self.attention_weights, self.pool_splits, scores_out)

    def forward(self, x, subtype_labels, adj, mask):
        if x.dim() == 2:
            x = x[None]
        if x.dim() != 3 or x.shape[0] != 1:
            raise ValueError(f"GatedABMIL.forward takes one bag [1, N, {self.L}] (models/mil.py:130 squeezes it), got {tuple(x.shape)}; "
                             "pool(x) is the batched form")
        M = self.pool(x)                                                                                    # [1, 1024]
        prob = Fh.linear(M, self.classifier[0].weight, self.classifier[0].bias, act=Fh.ACT_SIGMOID)       # [1, 2]
        _, pred = torch.max(prob, 1)
        loss = self.criterion(prob, subtype_labels)      # on the probabilities, as the reference has it
        return prob.data, pred, subtype_labels, loss

    def attention_map(self, x):
        """[B, 1, N]: the softmax over the bag that pool(x) weighs the instances with (A of models/mil.py:138), from one forward pass
        under no_grad.  (`attention_weights` is the reference's name of the score layer.)"""
        sink = []
        with torch.no_grad():
            self.pool(x, scores_out=sink)
            return _softmax_of(sink)
