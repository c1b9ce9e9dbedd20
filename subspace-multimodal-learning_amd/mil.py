"""Host-side mirror of the reference's attention-pooling MIL baseline:

  ABMIL   models/mil.py:34-82   attention network without gating (Linear 1024 -> 128, tanh, Linear 128 -> 1), softmax over the bag,
                                weighted sum of the raw features, classifier and multimodal projection; mode 'path' of define_net

Same constructor argument (an `args` namespace: label_dim, path_dim), forward signature, return tuple and parameter names - a reference
state_dict loads with strict=True.  The hidden layer runs on the f32 matrix cores (functional.linear, tanh epilogue); scores, softmax and
the weighted sum are one streaming pass over the bag (functional.attention_pool, csrc/attn_pool.hip).  The bag is a tensor of features:
it receives no gradient (x.requires_grad makes the backward raise)."""
from __future__ import annotations

import torch
from torch import nn

from . import functional as Fh


class ABMIL(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.L = 1024
        self.D = 128
        self.K = 1
        self.args = args
        self.n_classes = args.label_dim
        self.attention = nn.Sequential(nn.Linear(self.L, self.D), nn.Tanh(), nn.Linear(self.D, self.K))
        self.classifier = nn.Sequential(nn.Linear(self.L * self.K, self.n_classes))
        self.multimodal_projection = nn.Linear(self.L * self.K, self.args.path_dim)
        self.pool_splits = None          # pieces the pooling kernels cut a bag into; None: chosen by the library (tests force ragged splits)

    def _pool(self, x, scores_out=None):
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
            s, lse = sink
            return torch.exp(s - lse[:, None])[:, None, :]
