"""Host-side mirror of the reference's co-attention survival baseline (`mode: mcat`) on the HIP kernels:

  TransformerEncoderLayer / TransformerEncoder   torch.nn's, as models/model.py:590-597 constructs them: post-norm, relu, sequence first
  Attn_Net_Gated                                 models/mcat_utils.py:115-145
  MCAT_Surv                                      models/model.py:559-666

Same constructors, forward signatures, return values and parameter names (checkpoint format; the encoder carries torch.nn's names, so
strict=True loads work in both directions).  After the co-attention has reduced the bag to 4 tokens everything runs on token sets of a
few KB, where launches, not bandwidth, set the time: the 8-head self-attention is ONE launch per direction on the packed projection
(functional.token_self_attention), and each branch's softmax + bmm + gated head is ONE (functional.token_pool_gated), both in
csrc/token_set.hip.  The bag-sized work - the wsi Linear + ReLU and the 4 genomic queries over the bag - is functional.linear and the
few-query co-attention (csrc/fewq_attn.hip), which reads the bag once (key is value).

What stays in ATen: ELU / AlphaDropout of the sig_networks (unless `snn_fused`), Dropout on [B, <= 512]- and [4, B, <= 512]-sized activations, the draw of the attention-dropout
multipliers, stack / cat, sigmoid, cumprod.  `captum` is not mirrored.

Extension key `mcat_fused` (default true): false sends the co-attention and both token-set operations through their composed forms
(coattention.MultiheadAttention with permutes, matmul4 and softmax_rows) - the cross-check of the tests and the yardstick of
tests/tools/bench_mcat.py.  Extension key `snn_fused` (default false): the four sig_networks run as one fused call
(functional.snn_stack, csrc/snn_stack.hip) instead of a linear, an ELU and an AlphaDropout per layer.  smml.define_net does not build this class: it is delivered as an import swap."""
from __future__ import annotations

import copy

import torch
import torch.nn.functional as F
from torch import nn

from . import functional as Fh
from .cmta import SNN_Block, _sig_tokens
from .coattention import MultiheadAttention
from .fusion import BilinearFusion


class TransformerEncoderLayer(nn.Module):
    """torch.nn.TransformerEncoderLayer(d_model, nhead, dim_feedforward, dropout, activation='relu'): post-norm, sequence first
    (src [T, B, E]).  `fused` (a plain attribute, default True): sets of at most 8 tokens at a head dim of 32 or 64 without masks take
    functional.token_self_attention on the packed projection (functional.token_path names the choice); anything else, or fused = False,
    runs self_attn - coattention.MultiheadAttention - as it stands."""

    def __init__(self, d_model, nhead, dim_feedforward=2048, dropout=0.1, activation="relu"):
        super().__init__()
        if activation != "relu" and activation is not F.relu:
            raise NotImplementedError(f"TransformerEncoderLayer: activation {activation!r} (MCAT constructs 'relu')")
        self.self_attn = MultiheadAttention(d_model, nhead, dropout=dropout)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)
        self.fused = True

    def _dropping(self, mod: nn.Dropout) -> bool:
        return self.training and mod.p > 0

    def _self_attention(self, src, src_mask, src_key_padding_mask):
        """x + dropout1(self_attn(x)), ready for norm1"""
        T, B, E = src.shape
        att = self.self_attn
        if Fh.token_path(T=T, E=E, heads=att.num_heads, attn_mask=src_mask is not None, key_padding_mask=src_key_padding_mask is not None,
                         fused=self.fused and att._qkv_same_embed_dim and att.bias_k is None and not att.add_zero_attn) == "composed":
            sa = att(src, src, src, key_padding_mask=src_key_padding_mask, need_weights=False, attn_mask=src_mask)[0]
            return src + self.dropout1(sa)
        qkv = Fh.linear(src, att.in_proj_weight, att.in_proj_bias)                        # [T, B, 3 E], read in place below
        keep = None
        if self.training and att.dropout > 0:
            keep = F.dropout(torch.ones(B, att.num_heads, T, T, device=src.device), p=att.dropout, training=True)
        o = Fh.token_self_attention(qkv.transpose(0, 1), heads=att.num_heads, keep=keep).transpose(0, 1)      # [T, B, E], dense
        if self._dropping(self.dropout1):
            return src + self.dropout1(Fh.linear(o, att.out_proj.weight, att.out_proj.bias))
        return Fh.linear(o, att.out_proj.weight, att.out_proj.bias, residual=src)

    def forward(self, src, src_mask=None, src_key_padding_mask=None):
        x = self._self_attention(src.float(), src_mask, src_key_padding_mask)
        x = Fh.layer_norm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
        ff = Fh.linear(x, self.linear1.weight, self.linear1.bias, act=Fh.ACT_RELU)
        if self._dropping(self.dropout) or self._dropping(self.dropout2):
            y = x + self.dropout2(Fh.linear(self.dropout(ff), self.linear2.weight, self.linear2.bias))
        else:
            y = Fh.linear(ff, self.linear2.weight, self.linear2.bias, residual=x)
        return Fh.layer_norm(y, self.norm2.weight, self.norm2.bias, self.norm2.eps)


class TransformerEncoder(nn.Module):
    """torch.nn.TransformerEncoder(encoder_layer, num_layers, norm=None): num_layers deep copies of the layer, parameter names
    layers.<i>.<...>"""

    def __init__(self, encoder_layer, num_layers, norm=None):
        super().__init__()
        self.layers = nn.ModuleList([copy.deepcopy(encoder_layer) for _ in range(num_layers)])
        self.num_layers = num_layers
        self.norm = norm

    def forward(self, src, mask=None, src_key_padding_mask=None):
        x = src
        for layer in self.layers:
            x = layer(x, src_mask=mask, src_key_padding_mask=src_key_padding_mask)
        if self.norm is not None:
            x = Fh.layer_norm(x, self.norm.weight, self.norm.bias, self.norm.eps)
        return x


class Attn_Net_Gated(nn.Module):
    """Attention network with sigmoid gating (models/mcat_utils.py:115-145): A = attention_c(tanh(a(x)) * sigmoid(b(x))), returned with x.
    The two gates are ONE product with the stacked weight (`gates`: [.., 2 D], the tanh half, then the sigmoid half - the layout of the
    gated pooling kernels); the reference's Dropout(0.25) on each gate is one ATen dropout on the pair."""

    def __init__(self, L=1024, D=256, dropout=False, n_classes=1):
        super().__init__()
        a, b = [nn.Linear(L, D), nn.Tanh()], [nn.Linear(L, D), nn.Sigmoid()]
        if dropout:
            a.append(nn.Dropout(0.25))
            b.append(nn.Dropout(0.25))
        self.attention_a = nn.Sequential(*a)
        self.attention_b = nn.Sequential(*b)
        self.attention_c = nn.Linear(D, n_classes)

    def gates(self, x):
        h2 = Fh.linear(x, torch.cat((self.attention_a[0].weight, self.attention_b[0].weight)),
                       torch.cat((self.attention_a[0].bias, self.attention_b[0].bias)), act=Fh.ACT_TANH_SIGMOID)
        if len(self.attention_a) > 2 and self.training:
            h2 = F.dropout(h2, p=self.attention_a[2].p, training=True)
        return h2

    def forward(self, x):
        h2 = self.gates(x)
        D = h2.shape[-1] // 2
        A = Fh.linear(h2[..., :D] * h2[..., D:], self.attention_c.weight, self.attention_c.bias)
        return A, x


class MCAT_Surv(nn.Module):
    def __init__(self, args, fusion='concat', omic_sizes=[100, 100, 100, 131], n_classes=4, model_size_wsi: str = 'small',
                 model_size_omic: str = 'small', dropout=0.25):
        super().__init__()
        self.args = args
        self.fusion = fusion
        self.omic_sizes = omic_sizes
        self.n_classes = args.label_dim
        self.size_dict_WSI = {"small": [1024, 256, 256], "big": [1024, 512, 384]}
        self.size_dict_omic = {'small': [256, 256], 'big': [1024, 1024, 1024, 256]}
        size = self.size_dict_WSI[model_size_wsi]
        self.wsi_net = nn.Sequential(nn.Linear(size[0], size[1]), nn.ReLU(), nn.Dropout(0.25))
        hidden = self.size_dict_omic[model_size_omic]
        sig_networks = []
        for input_dim in omic_sizes:
            fc_omic = [SNN_Block(dim1=input_dim, dim2=hidden[0])]
            for i, _ in enumerate(hidden[1:]):
                fc_omic.append(SNN_Block(dim1=hidden[i], dim2=hidden[i + 1], dropout=0.25))
            sig_networks.append(nn.Sequential(*fc_omic))
        self.sig_networks = nn.ModuleList(sig_networks)
        self.coattn = MultiheadAttention(embed_dim=256, num_heads=1)
        path_encoder_layer = TransformerEncoderLayer(d_model=256, nhead=8, dim_feedforward=512, dropout=dropout, activation='relu')
        self.path_transformer = TransformerEncoder(path_encoder_layer, num_layers=2)
        self.path_attention_head = Attn_Net_Gated(L=size[2], D=size[2], dropout=dropout, n_classes=1)
        self.path_rho = nn.Sequential(nn.Linear(size[2], size[2]), nn.ReLU(), nn.Dropout(dropout))
        omic_encoder_layer = TransformerEncoderLayer(d_model=256, nhead=8, dim_feedforward=512, dropout=dropout, activation='relu')
        self.omic_transformer = TransformerEncoder(omic_encoder_layer, num_layers=2)
        self.omic_attention_head = Attn_Net_Gated(L=size[2], D=size[2], dropout=dropout, n_classes=1)
        self.omic_rho = nn.Sequential(nn.Linear(size[2], size[2]), nn.ReLU(), nn.Dropout(dropout))
        if self.fusion == 'concat':
            self.mm = nn.Sequential(nn.Linear(256 * 2, size[2]), nn.ReLU(), nn.Linear(size[2], size[2]), nn.ReLU())
        elif self.fusion == 'bilinear':
            self.mm = BilinearFusion(dim1=256, dim2=256, scale_dim1=8, scale_dim2=8, mmhid=256)
        else:
            self.mm = None
        self.classifier = nn.Linear(size[2], self.n_classes)
        # extension key: mcat_fused (absent / true: the few-query co-attention and the token-set kernels; false: the composed forms)
        self.mcat_fused = bool(getattr(args, "mcat_fused", True))
        self.coattn.fused_few_query = self.mcat_fused
        for layer in list(self.path_transformer.layers) + list(self.omic_transformer.layers):
            layer.fused = self.mcat_fused
        # extension key: snn_fused (absent / false: linear, ELU and AlphaDropout per layer; independent of mcat_fused) - the four sig_networks
        # in ONE functional.snn_stack call on the column views of x_omic, whose [4, B, 256] output is the stacked tensor itself.  In train
        # mode the dropout multipliers of all eight layers come from one draw: reproducible under torch.manual_seed, but a random stream of
        # its own (the composed form draws once per layer)
        self.snn_fused = bool(getattr(args, "snn_fused", False))

    def _pool(self, head: Attn_Net_Gated, rho: nn.Sequential, h_trans, sink=None):
        """models/model.py:633-640 / :645-651: the gated head's scores, softmax over the 4 tokens, bmm with the tokens, rho -> [B, 256]"""
        T, B, E = h_trans.shape
        D = head.attention_c.weight.shape[1]
        if Fh.token_path(T=T, E=E, D=D, fused=self.mcat_fused and head.attention_c.weight.shape[0] == 1) == "token":
            xb = h_trans.transpose(0, 1).contiguous()                                     # [B, T, E]: the gates and the pooling read the same rows
            scores = [] if sink is not None else None
            M = Fh.token_pool_gated(xb, head.gates(xb), head.attention_c.weight, head.attention_c.bias, scores_out=scores)
            if sink is not None:
                sink.append(scores[0].view(B, 1, T))
        else:
            A, h = head(h_trans)                                                          # [T, B, 1], [T, B, E]
            A = A.permute(1, 2, 0)                                                        # [B, 1, T]
            M = Fh.matmul4(Fh.softmax_rows(A).unsqueeze(1), h.transpose(0, 1).unsqueeze(1)).reshape(B, E)
            if sink is not None:
                sink.append(A)
        return rho[2](Fh.linear(M, rho[0].weight, rho[0].bias, act=Fh.ACT_RELU)).reshape(B, -1)     # the reference's bare .squeeze() breaks B = 1

    def _forward(self, x_path, x_omic_all, sink=None):
        sizes = self.omic_sizes
        x_omic = [x_omic_all[:, sum(sizes[:i]):sum(sizes[:i + 1])] for i in range(len(sizes))]
        # wsi fc: Linear + ReLU fused in the GEMM epilogue, Dropout(0.25) in ATen (train mode only); the bag stays [B, N, 256] in memory and
        # the co-attention reads its sequence-first view in place
        h_path_bag = self.wsi_net[2](Fh.linear(x_path.float(), self.wsi_net[0].weight, self.wsi_net[0].bias, act=Fh.ACT_RELU)).transpose(0, 1)
        h_omic_bag = _sig_tokens(self.sig_networks, x_omic, self.training, self.snn_fused)       # [4, B, 256]
        h_path_coattn, A_coattn = self.coattn(h_omic_bag, h_path_bag, h_path_bag)          # [4, B, 256], raw scores [B, 1, 4, N]
        if sink is not None:
            sink.append(A_coattn)
        h_path = self._pool(self.path_attention_head, self.path_rho, self.path_transformer(h_path_coattn), sink)
        h_omic = self._pool(self.omic_attention_head, self.omic_rho, self.omic_transformer(h_omic_bag), sink)
        if self.fusion == 'bilinear':
            h = self.mm(h_path, h_omic)
        elif self.fusion == 'concat':
            h = Fh.linear(torch.cat((h_path, h_omic), dim=1), self.mm[0].weight, self.mm[0].bias, act=Fh.ACT_RELU)
            h = Fh.linear(h, self.mm[2].weight, self.mm[2].bias, act=Fh.ACT_RELU)
        else:
            raise NotImplementedError("Fusion [{}] is not implemented".format(self.fusion))
        logits = Fh.linear(h, self.classifier.weight, self.classifier.bias)
        hazards = torch.sigmoid(logits)
        S = torch.cumprod(1 - hazards, dim=1)
        return logits, hazards, S

    def forward(self, **kwargs):
        return self._forward(kwargs['x_path'], kwargs['x_omic'])

    @torch.no_grad()
    def attention_scores(self, **kwargs):
        """The dict the reference builds at models/model.py:665 and drops - the RAW scores of one forward:
        {'coattn': [B, 1, 4, N], 'path': [B, 1, 4], 'omic': [B, 1, 4]}.  Runs the model as it stands (train or eval) without a graph."""
        sink = []
        self._forward(kwargs['x_path'], kwargs['x_omic'], sink)
        return dict(zip(('coattn', 'path', 'omic'), sink))

    def attention_maps(self, **kwargs):
        """The three attention maps of one forward - the softmax of attention_scores over the bag and over the tokens:
        {'coattn': [B, 4, N], 'path': [B, 1, 4], 'omic': [B, 1, 4]}, every row sums to one."""
        raw = self.attention_scores(**kwargs)
        with torch.no_grad():
            return {'coattn': Fh.softmax_rows(raw['coattn'][:, 0]), 'path': Fh.softmax_rows(raw['path']), 'omic': Fh.softmax_rows(raw['omic'])}
