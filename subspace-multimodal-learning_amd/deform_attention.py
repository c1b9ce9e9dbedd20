"""Host-side mirror of the reference's deformable cross-attention modules on the HIP kernels.

Same constructor keywords / defaults, forward signatures, tensor layouts and parameter names
(= checkpoint format) as
  models/DeformableAttention2D.py:161-325  DeformCrossAttention2D (+ CPB :120-157, Scale :110-116)
  models/DeformableAttention1D.py:106-240  DeformCrossAttention1D (+ CPB :60-102)
so `state_dict`s are interchangeable.  The nn.Conv / nn.Linear sub-modules only hold the parameters
(identical default initialisation); the arithmetic runs in the kernels behind `functional`.

Additive knobs (reference defaults kept): `grid_hw` - the reference hard-wires a 50 x 50 token grid
(DeformableAttention2D.py:239-240,318); here the grid defaults to the square root of the token count.
`compute_dtype` (None | 'bf16' | 'fp16', default None): the 16-bit compute mode of the fused attention core
(csrc/deform_attn16.hip; BASELINE config 4 names bf16) - parameters, inputs, outputs and gradients stay fp32.
Corrected-semantics switches, OFF by default (bit-parity with the reference needs them off):
  * DeformCrossAttention2D(consistent_grid_norm=True): the reference normalises sample positions with the
    align_corners=True formula 2 v / (t - 1) - 1 (:100-108,265; x divided by rows - 1, y by cols - 1) but samples with
    F.grid_sample(align_corners=False) (:268) - ~21 % of the corner fetches fall outside the map at initialisation.  With
    the switch both the sample positions and the query grid use the pixel-centre convention (2 p + 1) / size - 1, x scaled
    by the number of columns and y by the number of rows.
  * DeformCrossAttention1D(true_1d_sampling=True): the reference's grid_sample_1d (:36-43) lays the features out
    [H = n, W = 1] while the grid carries (x = vs, y = 0), so every "sampled" key is the centre token scaled; with the switch
    the map is [H = 1, W = n] and vs interpolates along the tokens.
Attention maps (additive; default off): `forward_tokens(..., return_attn_maps=True)` / `forward(..., return_attn_maps=True)` append a dict
{"key_mass" [B, heads, J], "patch_map" [B, groups, rows, cols] (2-D module only), "vs", "vgrid"} to the return value - the pre-dropout
softmax of the SAME fused forward launch, reduced by functional.deform_attention_maps; "dense" adds "attn" [B, heads, N, J].  The fp32-grade
cores only (compute_dtype / cpb_table raise ValueError).
"""
from __future__ import annotations

import functools
import math
from typing import Optional, Tuple

import torch
from torch import nn

from . import functional as Fh


def _default(v, d):
    return d if v is None else v


class Scale(nn.Module):
    def __init__(self, scale):
        super().__init__()
        self.scale = scale

    def forward(self, x):
        return x * self.scale


class CPB(nn.Module):
    """Parameter holder of the continuous position bias MLP (in -> dim -> dim -> heads // offset_groups)."""

    def __init__(self, dim, *, heads, offset_groups, depth, in_dim=2, log_distance=True):
        super().__init__()
        self.heads, self.offset_groups, self.log_distance = heads, offset_groups, log_distance
        self.mlp = nn.ModuleList([nn.Sequential(nn.Linear(in_dim, dim), nn.ReLU())])
        for _ in range(depth - 1):
            self.mlp.append(nn.Sequential(nn.Linear(dim, dim), nn.ReLU()))
        self.mlp.append(nn.Linear(dim, heads // offset_groups))
        if depth != 2 or dim not in (32, 64, 128):
            raise NotImplementedError("the position-bias kernels are built for depth 2 and width 32, 64 or 128 (dim = 128, 256 or 512)")

    def tensors(self):
        m = self.mlp
        return (m[0][0].weight, m[0][0].bias, m[1][0].weight, m[1][0].bias, m[2].weight, m[2].bias)


def _dropout_args(mod, device=None):
    """nn.Dropout semantics on the attention probabilities: active in train() with p > 0; the 64-bit seed of the
    in-kernel counter-based mask is drawn from torch's default (CPU) generator, so torch.manual_seed reproduces it.
    While the step is being captured in a hipGraph the host seed would be the same in every replay: the call then also gets a
    device-resident offset that a captured counter bumps per call and per replay (functional.graph_seed_offset)."""
    p = float(mod.dropout.p)
    if not mod.training or p <= 0.0:
        return {"dropout_p": 0.0, "dropout_seed": 0}
    seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
    mod.last_dropout_seed = seed
    off = Fh.graph_seed_offset(device) if device is not None and torch.device(device).type == "cuda" else None
    return {"dropout_p": p, "dropout_seed": seed, "dropout_seed_offset": off}


_GRID_CACHE = {}
_GRAD_FORK = __import__("os").environ.get("SMML_GRAD_FORK", "1") != "0"       # measurement switch (functional.GradFork)


def _maps_arg(mod, return_attn_maps):
    """return_attn_maps of a module's forward -> (an AttnScores sink or None, dense); the modes without maps are refused before any launch"""
    if return_attn_maps not in (False, True, None, "dense"):
        raise ValueError("return_attn_maps must be False, True or 'dense'")
    if not return_attn_maps:
        return None, False
    if mod.cpb_table:
        raise ValueError(f"cpb_table={mod.cpb_table!r}: attention maps are built for the fp32-grade cores, not for the table modes")
    if mod.compute_dtype is not None:
        raise ValueError(f"compute_dtype={mod.compute_dtype!r}: attention maps are built for the fp32-grade cores, not for the 16-bit compute modes")
    return Fh.AttnScores(), return_attn_maps == "dense"


def _with_attn_maps(forward):
    """The channels-first forward of the reference plus the additive keyword-only return_attn_maps.  The reference's forward is kept as
    written and stays what inspect.signature reports (functools.wraps): (x1, x2, return_vgrid=False)."""
    @functools.wraps(forward)
    def with_maps(self, x1, x2, return_vgrid=False, *, return_attn_maps=False):
        if not return_attn_maps:
            return forward(self, x1, x2, return_vgrid)
        r = self.forward_tokens(x1.transpose(1, 2), x2.transpose(1, 2), return_vgrid, return_attn_maps=return_attn_maps)
        return (r[0].transpose(1, 2),) + tuple(r[1:])
    return with_maps


def _grid_queries_2d(Hh: int, Ww: int, device) -> torch.Tensor:
    """Cached per (rows, cols, device): a constant of the token grid (eight small kernels per forward otherwise)."""
    key = (Hh, Ww, str(device))
    g = _GRID_CACHE.get(key)
    if g is None:
        g = _GRID_CACHE[key] = _build_grid_queries_2d(Hh, Ww, device)
    return g


def _build_grid_queries_2d(Hh: int, Ww: int, device) -> torch.Tensor:
    """Normalised query grid [N, 2] = (x, y) per token, restating create_grid_like + normalize_grid(dim=0)
    (DeformableAttention2D.py:88-108,296-297): x is divided by (rows - 1), y by (cols - 1)."""
    qx = 2.0 * torch.arange(Ww, dtype=torch.float32, device=device) / max(Hh - 1, 1) - 1.0
    qy = 2.0 * torch.arange(Hh, dtype=torch.float32, device=device) / max(Ww - 1, 1) - 1.0
    return torch.stack((qx.view(1, Ww).expand(Hh, Ww), qy.view(Hh, 1).expand(Hh, Ww)), dim=-1).reshape(Hh * Ww, 2).contiguous()


def _pos_pmax_2d(Hh: int, Ww: int, th: int, tw: int, offset_scale: float) -> float:
    """Half-width (functional.table_pmax) of the square of signed-log offsets the 2-D position bias can be asked for on an Hh x Ww token
    grid with a th x tw key grid: |gq| and |vs| are bounded by the grids' shapes and tanh . offset_scale (normalize_grid divides x by
    rows - 1, y by cols - 1).  No host sync."""
    lo_q, lo_k = max(min(Hh, Ww) - 1, 1), max(min(th, tw) - 1, 1)
    gqb = max(1.0, abs(2.0 * (max(Hh, Ww) - 1) / lo_q - 1.0))
    vsb = max(abs(2.0 * (max(th, tw) - 1 + offset_scale) / lo_k - 1.0), 1.0 + 2.0 * offset_scale / lo_k)
    return Fh.table_pmax(gqb, vsb)


def _pos_pmax_1d(t: int, offset_scale: float) -> float:
    """The same for the 1-D module with t keys: |seq| <= 1, |vs| <= 1 + 2 offset_scale / (t - 1)."""
    return Fh.table_pmax(1.0, 1.0 + 2.0 * offset_scale / max(t - 1, 1))


class _DeformCrossAttention(nn.Module):
    """What the 2-D and the 1-D module share: the reference's options and sub-modules (registered in its order: the checkpoint format) and
    the token-major forward around two hooks - _keys (offsets network + sampler) and _bias_args (query positions, the options of
    functional.deform_attention)."""

    def _build(self, conv, posdim: int, offset_placeholders, *, dim, dim_head, heads, dropout, downsample_factor, offset_scale, offset_groups,
               offset_kernel_size, group_queries, group_key_values, compute_dtype, cpb_table, cpb_log_distance=True):
        Fh._dtype16(compute_dtype)             # validates: None | 'bf16' | 'fp16'
        self.compute_dtype = compute_dtype     # additive: None = the fp32-grade path, else the 16-bit compute mode of the fused core
        if cpb_table and compute_dtype is None:
            raise ValueError("cpb_table belongs to the 16-bit compute modes: pass compute_dtype='bf16' or 'fp16'")
        self.cpb_table = cpb_table             # additive: False | True ('full') | 'forward' - position bias from a table of the MLP (functional.deform_attention)
        offset_scale = _default(offset_scale, downsample_factor)
        assert offset_kernel_size >= downsample_factor, \
            'offset kernel size must be greater than or equal to the downsample factor'
        assert (offset_kernel_size - downsample_factor) % 2 == 0
        offset_groups = _default(offset_groups, heads)
        assert heads % offset_groups == 0
        if not cpb_log_distance and cpb_table:
            raise NotImplementedError("the table modes are built for the log-distance form of the position bias only")
        inner_dim = dim_head * heads
        self.scale = dim_head ** -0.5
        self.heads, self.offset_groups = heads, offset_groups
        self.dim, self.dim_head = dim, dim_head
        offset_dims = inner_dim // offset_groups
        self.downsample_factor = downsample_factor
        self.offset_kernel_size, self.offset_scale = offset_kernel_size, float(offset_scale)
        self.group_queries, self.group_key_values = group_queries, group_key_values
        self.to_offsets = nn.Sequential(
            conv(offset_dims, offset_dims, offset_kernel_size, groups=offset_dims, stride=downsample_factor,
                 padding=(offset_kernel_size - downsample_factor) // 2),
            nn.GELU(),
            conv(offset_dims, posdim, 1, bias=False),
            *offset_placeholders,
            nn.Tanh(),
            Scale(offset_scale))
        self.rel_pos_bias = CPB(dim // 4, offset_groups=offset_groups, heads=heads, depth=2, in_dim=posdim, log_distance=cpb_log_distance)
        self.dropout = nn.Dropout(dropout)
        self.to_q = conv(dim, inner_dim, 1, groups=offset_groups if group_queries else 1, bias=False)
        self.to_k = conv(dim, inner_dim, 1, groups=offset_groups if group_key_values else 1, bias=False)
        self.to_v = conv(dim, inner_dim, 1, groups=offset_groups if group_key_values else 1, bias=False)
        self.to_out = conv(inner_dim, dim, 1)

    def forward_tokens(self, x1t, x2t, return_vgrid=False, residual=None, return_attn_maps=False):
        """Token-major entry: x1t (queries) / x2t (keys, values) [B, N, C] -> [B, N, C] (+ residual).  return_attn_maps (True | 'dense'): the
        attention maps of this call (module docstring) are appended to the return value.  2-D: patch_map lies on the grid and at the sample
        positions the module sampled with, whichever normalisation is on.  1-D: no patch map - the default sampler reads the centre token
        for every key (the bug-compatible degenerate axis), so a splat says nothing there."""
        sink, dense = _maps_arg(self, return_attn_maps)
        G, H = self.offset_groups, self.heads
        q = Fh.grouped_pointwise(x1t, self.to_q.weight, G if self.group_queries else 1)            # [B, N, inner]
        vgrid, vs, kv, fork, state = self._keys(x1t, x2t, q)                                        # kv [B, J, C]
        gk = G if self.group_key_values else 1
        k = Fh.grouped_pointwise(kv, self.to_k.weight, gk)
        v = Fh.grouped_pointwise(kv, self.to_v.weight, gk)
        gq, opts, maps_args = self._bias_args(state, vgrid, vs)
        o = Fh.deform_attention(q, k, v, vs, gq, *self.rel_pos_bias.tensors(), heads=H, groups=G, scale=self.scale,
                                compute_dtype=self.compute_dtype, fork=fork, **opts, **_dropout_args(self, q.device),
                                **({} if sink is None else {"attn_scores": sink}))
        # the output projection follows the core's compute mode (single-term 16-bit operands, fp32 accumulation and storage)
        out = Fh.linear(o, self.to_out.weight.reshape(self.dim, -1), self.to_out.bias, residual=residual, prec=Fh.prec16(self.compute_dtype))
        ret = (out, vgrid) if return_vgrid else (out,)
        if sink is not None:
            maps = Fh.deform_attention_maps(sink, heads=H, groups=G, dense=dense, **maps_args)
            ret += ({**maps, "vs": vs.detach(), "vgrid": vgrid.detach()},)
        return ret if len(ret) > 1 else out

    @_with_attn_maps
    def forward(self, x1, x2, return_vgrid=False):
        """x1, x2 [B, C, N] channels-first as in the reference -> [B, C, N] (and vgrid [(B g), 2, th, tw]; 1-D: [(B g), t]).  Keyword-only
        return_attn_maps (True | 'dense'): the attention maps of the call are appended (module docstring)."""
        r = self.forward_tokens(x1.transpose(1, 2), x2.transpose(1, 2), return_vgrid)
        if return_vgrid:
            return r[0].transpose(1, 2), r[1]
        return r.transpose(1, 2)


class DeformCrossAttention2D(_DeformCrossAttention):
    def __init__(self, *, dim, dim_head=64, heads=8, dropout=0., downsample_factor=4, offset_scale=4,
                 offset_groups=8, offset_kernel_size=6, group_queries=True, group_key_values=True,
                 grid_hw: Optional[Tuple[int, int]] = None, consistent_grid_norm: bool = False, compute_dtype=None,
                 cpb_table: bool = False, cpb_regions_multi_head: bool = False):
        super().__init__()
        self.consistent_grid_norm = bool(consistent_grid_norm)
        # cpb_regions_multi_head (off by default): the position bias per linear region of its MLP also with two heads per offset group
        # (functional.deform_attention; one head per group takes that path anyway).  No table mode; other limits are checked at the call
        if cpb_regions_multi_head and cpb_table:
            raise ValueError("cpb_regions_multi_head (the region path) and cpb_table exclude each other")
        self.cpb_regions_multi_head = bool(cpb_regions_multi_head)
        self.grid_hw = grid_hw
        self._build(nn.Conv2d, 2, (), dim=dim, dim_head=dim_head, heads=heads, dropout=dropout, downsample_factor=downsample_factor,
                    offset_scale=offset_scale, offset_groups=offset_groups, offset_kernel_size=offset_kernel_size, group_queries=group_queries,
                    group_key_values=group_key_values, compute_dtype=compute_dtype, cpb_table=cpb_table)

    def _grid(self, n: int) -> Tuple[int, int]:
        if self.grid_hw is not None:
            return self.grid_hw
        s = int(round(math.sqrt(n)))
        if s * s != n:
            raise ValueError(f"token count {n} is not a square; pass grid_hw=(rows, cols)")
        return s, s

    def _key_grid(self, Hh: int, Ww: int) -> Tuple[int, int]:
        """The offsets network's output grid (= vgrid's), known before it runs."""
        L = Fh.capi.lib()
        return (L.smml_offsets_out_len(Hh, self.offset_kernel_size, self.downsample_factor),
                L.smml_offsets_out_len(Ww, self.offset_kernel_size, self.downsample_factor))

    def _region_pmax(self, Hh: int, Ww: int) -> float:
        """_pos_pmax_2d of a bag on an Hh x Ww grid, before its vgrid exists (prefetch_regions)."""
        return _pos_pmax_2d(Hh, Ww, *self._key_grid(Hh, Ww), self.offset_scale)

    def _regions_apply(self, n_tokens: int) -> bool:
        """Whether forward_tokens on a bag of n_tokens takes the region path with the pmax of _region_pmax (functional.deform_path)."""
        if self.consistent_grid_norm or not self.rel_pos_bias.mlp[0][0].weight.is_cuda:
            return False
        if tuple(self.rel_pos_bias.mlp[1][0].weight.shape) != (32, 32):      # widths 64 / 128 (dim = 256 / 512): no region path
            return False
        th, tw = self._key_grid(*self._grid(n_tokens))
        w = self.rel_pos_bias.tensors()
        return Fh.deform_path(posdim=2, heads=self.heads, groups=self.offset_groups, keys=th * tw, w2_shape=w[2].shape, w3_shape=w[4].shape,
                              compute_dtype=self.compute_dtype, cpb_table=self.cpb_table, region_pmax_given=True,
                              regions_multi_head=self.cpb_regions_multi_head) == "region"

    def prefetch_regions(self, n_tokens: int) -> None:
        """Starts the build of the position bias's region tables on a side stream (functional.RegionPrefetch); the next forward_tokens on
        a bag of n_tokens joins it.  Optional: without it the tables are built in front of the attention launch."""
        self._prefetch = None
        if not (Fh.REGION_PREFETCH and self._regions_apply(n_tokens)):
            return
        Hh, Ww = self._grid(n_tokens)
        self._prefetch = Fh.RegionPrefetch(*self.rel_pos_bias.tensors(), self._region_pmax(Hh, Ww))

    def _keys(self, x1t, x2t, q):
        B, N, C = x1t.shape
        Hh, Ww = self._grid(N)
        G = self.offset_groups
        fork = Fh.GradFork() if (q.requires_grad and not self.consistent_grid_norm and _GRAD_FORK) else None       # q's two gradients meet in one buffer
        vgrid, vs = Fh.offsets(q.view(B, Hh, Ww, -1), self.to_offsets[0].weight, self.to_offsets[0].bias,
                               self.to_offsets[2].weight.reshape(2, -1), groups=G, ks=self.offset_kernel_size,
                               r=self.downsample_factor, posdim=2, offset_scale=self.offset_scale, fork=fork)
        gq = _grid_queries_2d(Hh, Ww, x1t.device)
        if self.consistent_grid_norm:          # corrected semantics (off by default): pixel-centre convention on both sides
            th, tw = vgrid.shape[-2:]
            vs = torch.stack(((2.0 * vgrid[:, 0] + 1.0) / tw - 1.0, (2.0 * vgrid[:, 1] + 1.0) / th - 1.0), dim=-1)
            vs = vs.reshape(B * G, th * tw, 2).contiguous()
            ar = lambda n: (2.0 * torch.arange(n, dtype=torch.float32, device=x1t.device) + 1.0) / n - 1.0
            gq = torch.stack((ar(Ww).view(1, Ww).expand(Hh, Ww), ar(Hh).view(Hh, 1).expand(Hh, Ww)), dim=-1).reshape(Hh * Ww, 2).contiguous()
        kv = Fh.bilinear_sample(x2t.reshape(B, Hh, Ww, C), vs, groups=G, posdim=2)
        return vgrid, vs, kv, fork, (Hh, Ww, gq)

    def _bias_args(self, state, vgrid, vs):
        Hh, Ww, gq = state
        pmax = _pos_pmax_2d(Hh, Ww, *vgrid.shape[-2:], self.offset_scale)
        if self.cpb_table:
            opts = {"cpb_table": self.cpb_table, "cpb_table_pmax": None if self.consistent_grid_norm else pmax,      # None: from the data
                    "cpb_table_grid": (Hh, Ww)}                # gq is a regular grid in both normalisations
        elif not self.consistent_grid_norm:
            # the square the region tables of the position bias cover (no host sync), and the build started by prefetch_regions, if any
            opts = {"cpb_region_pmax": pmax, "cpb_region_prefetch": getattr(self, "_prefetch", None)}
            self._prefetch = None
        else:
            opts = {}
        if self.cpb_regions_multi_head:
            opts["cpb_regions_multi_head"] = True
        return gq, opts, {"vs": vs, "grid_hw": (Hh, Ww)}


class DeformCrossAttention1D(_DeformCrossAttention):
    def __init__(self, *, dim, dim_head=64, heads=8, dropout=0., downsample_factor=4, offset_scale=None,
                 offset_groups=4, offset_kernel_size=6, cpb_log_distance=True, group_queries=False,
                 group_key_values=False, true_1d_sampling: bool = False, compute_dtype=None, cpb_table: bool = False,
                 cpb_regions: bool = False):
        super().__init__()
        self.true_1d_sampling = bool(true_1d_sampling)
        # cpb_regions (off by default): the position bias per linear piece of its MLP (functional.deform_attention, csrc/cpb_regions1d.h) -
        # signed-log offsets and the fp32-grade core only; heads // offset_groups must be 1 or 2 (checked at the call)
        if cpb_regions and (compute_dtype is not None or cpb_table or not cpb_log_distance):
            raise ValueError("cpb_regions (the 1-D piece path) takes signed-log offsets in the fp32-grade core: no compute_dtype, no cpb_table, "
                             "cpb_log_distance=True")
        self.cpb_regions = bool(cpb_regions)
        self.cpb_log_distance = bool(cpb_log_distance)
        # nn.Identity: placeholder for the reference's Rearrange('b 1 n -> b n') (no parameters)
        self._build(nn.Conv1d, 1, (nn.Identity(),), dim=dim, dim_head=dim_head, heads=heads, dropout=dropout, downsample_factor=downsample_factor,
                    offset_scale=offset_scale, offset_groups=offset_groups, offset_kernel_size=offset_kernel_size, group_queries=group_queries,
                    group_key_values=group_key_values, compute_dtype=compute_dtype, cpb_table=cpb_table, cpb_log_distance=cpb_log_distance)

    def _keys(self, x1t, x2t, q):
        B, n, C = x1t.shape
        G = self.offset_groups
        vgrid, vs = Fh.offsets(q.view(B, 1, n, -1), self.to_offsets[0].weight, self.to_offsets[0].bias,
                               self.to_offsets[2].weight.reshape(1, -1), groups=G, ks=self.offset_kernel_size,
                               r=self.downsample_factor, posdim=1, offset_scale=self.offset_scale)
        # bug-compatible degenerate sampling (DeformableAttention1D.py:36-43): map laid out [H = n, W = 1]; the corrected
        # switch lays it out [H = 1, W = n] so that vs interpolates along the tokens
        kv = Fh.bilinear_sample(x2t.reshape(B, 1, n, C) if self.true_1d_sampling else x2t.reshape(B, n, 1, C), vs, groups=G, posdim=1)
        return vgrid, vs, kv, None, n

    def _bias_args(self, n, vgrid, vs):
        seq = (2.0 * torch.arange(n, dtype=torch.float32, device=vs.device) / max(n - 1, 1) - 1.0).view(n, 1)
        opts = {"log_distance": self.cpb_log_distance}
        if self.cpb_table:
            opts.update(cpb_table=self.cpb_table, cpb_table_pmax=_pos_pmax_1d(vgrid.shape[-1], self.offset_scale))
        if self.cpb_regions:
            opts.update(cpb_regions=True, cpb_region_pmax=_pos_pmax_1d(vgrid.shape[-1], self.offset_scale))
        return seq.contiguous(), opts, {}
