"""Autograd bindings of the HIP kernels (C-ABI in include/smml.h, loaded by _capi.py).

Each op is a torch.autograd.Function whose forward and backward launch hand-written gfx950 kernels on
the current HIP stream; PyTorch only provides device memory, the stream and the autograd graph.  All
tensors are fp32 and token-major (channel-last).  There is no CPU / eager fallback."""
from __future__ import annotations

import math
import os
from typing import Optional

import ctypes as C_

import torch

from . import _capi as capi

ACT_NONE, ACT_RELU, ACT_TANH = 0, 1, 2
ACT_SIGMOID = 3
ACT_TANH_SIGMOID = 4         # tanh on output columns [0, N / 2), sigmoid on [N / 2, N): the two gates of a gated attention head in one product


# ------------------------------------------------------------------------------------------------
# Deterministic mode: with the switch on, every sum the package's kernels form runs in a fixed order - partial results
# to a workspace, one owner per output element - so a value or gradient is a function of the inputs alone, run after run.  Off (the
# default) nothing changes: the same kernels, launches and bits as without the switch.  SMML_DETERMINISTIC=1 presets it.
# ------------------------------------------------------------------------------------------------
DETERMINISTIC = os.environ.get("SMML_DETERMINISTIC", "0") not in ("", "0")


def set_deterministic(on: bool) -> None:
    """Switches the deterministic mode on or off for the calls that follow (see `deterministic`)."""
    global DETERMINISTIC
    DETERMINISTIC = bool(on)


def is_deterministic() -> bool:
    return bool(DETERMINISTIC)


class deterministic:
    """with deterministic(): ... - the deterministic mode for the forward calls issued inside the block; nests, and restores the previous
    value on exit, also when the block raises.  Every autograd Function reads the switch in its FORWARD and keeps the choice: its backward
    is deterministic as well, even when it runs after the block has ended.

    Covered: the fp32-grade and 16-bit deform paths (DeformPathomicNet, both attn_dim values), BatchLoss, the co-attention
    MultiheadAttention and ABMIL (the attention-pooling kernels have a single form that is deterministic by construction - per-split
    partials merged in a fixed order - and the switch only selects the fixed-order reductions of the hidden layer's gradients; the
    few-query co-attention kernels are of the same kind, the switch selects the fixed-order forms of the weight gradients around them; the token-set kernels of MCAT_Surv have one form, fixed-order by
    construction).  An operation whose kernel still adds floats with atomics - the table modes of the position bias, the
    bf16-storage GEMM with a split reduction, the depthwise-convolution weight gradients of the Nystrom block and of PPEG - raises
    RuntimeError under the switch; there is no silent fall-back.

    The switch is NOT tied to torch.use_deterministic_algorithms: that flag makes unrelated ATen operations raise, and this package's
    kernels do not read it.  Set both if the ATen side of a program has to be pinned down too."""

    def __init__(self, on: bool = True):
        self.on = bool(on)
        self.prev = []

    def __enter__(self):
        global DETERMINISTIC
        self.prev.append(DETERMINISTIC)
        DETERMINISTIC = self.on
        return self

    def __exit__(self, *exc):
        global DETERMINISTIC
        DETERMINISTIC = self.prev.pop()
        return False


def _no_det(op: str, why: str):
    raise RuntimeError(f"{op} has no deterministic form yet: {why} (functional.deterministic / SMML_DETERMINISTIC is on; "
                       "there is no silent fall-back)")


def _scratch(nbytes: int, device) -> torch.Tensor:
    """Workspace of a deterministic launch: a plain torch.empty tensor (16-byte aligned, no host synchronisation, graph-capturable)."""
    return torch.empty(max((int(nbytes) + 3) // 4, 1), device=device, dtype=torch.float32)


class KernelTimer:
    """Optional HIP-event timing of the two dominant kernels (fused attention forward, position-bias
    backward) on the stream they are launched on; used by bench.py's roofline leg.  Off by default."""

    def __init__(self):
        self.enabled = False
        self.pairs = {"deform_attn_fwd": [], "cpb_bwd": []}
        self.work = {"deform_attn_fwd": [], "cpb_bwd": []}     # (query, key) pairs per launch

    def events(self, name, pairs_count):
        if not self.enabled:
            return None, None
        L = capi.lib()
        a, b = L.smml_event_create(), L.smml_event_create()
        self.pairs.setdefault(name, []).append((a, b))
        self.work.setdefault(name, []).append(pairs_count)
        return a, b

    def collect(self):
        """-> {name: (launches, mean ms, mean pairs per launch)}; destroys the events."""
        import ctypes
        L = capi.lib()
        out = {}
        for name, evs in self.pairs.items():
            tot = 0.0
            for a, b in evs:
                ms = ctypes.c_float(0)
                capi.check(L.smml_event_elapsed_ms(a, b, ctypes.byref(ms)), "event_elapsed")
                tot += ms.value
                L.smml_event_destroy(a); L.smml_event_destroy(b)
            if evs:
                out[name] = (len(evs), tot / len(evs), sum(self.work[name]) / len(evs))
            self.pairs[name] = []
            self.work[name] = []
        return out


TIMER = KernelTimer()

# Decision tap (parity tests only; None in production).  When a test sets this to a list, every bilinear-sampling launch and every
# fused-attention forward appends what is needed to recover the piecewise-linear decisions the kernels took - the sampler's
# cells, the layer-1 and layer-2 ReLU masks of the position-bias MLP - so that tests can impose the SAME decisions on the fp64
# oracle (tests/helpers.py Decisions).  Nothing here changes what the kernels compute.
DECISION_TAP = None


def relu_masks_rows(masks):
    """The saved layer-2 ReLU masks [B, H, nst / 32, J, 2, 32] (per-tile storage of the kernels) as [B, H, J, 2, nst] rows - the layout
    smml_deform_attn_relu1_masks writes and the tests decode.  Tests only."""
    B, H, NT, J, _, _ = masks.shape
    return masks.permute(0, 1, 3, 4, 2, 5).reshape(B, H, J, 2, NT * 32)


def relu1_masks(vs, gq, w1, b1, *, B: int, N: int, J: int, groups: int, log_distance: bool = True):
    """Layer-1 ReLU decisions of the position-bias MLP as the kernels evaluate them: int16 [(B G), J, 2, nst] in the bit order of the
    saved layer-2 masks (include/smml.h smml_deform_attn_relu1_masks).  Tests only."""
    out = torch.empty(B * groups, J, 2, capi.lib().smml_deform_attn_nst(N), device=vs.device, dtype=torch.int16)
    ns = dict(vs=_c(vs), gq=_c(gq), w1=_c(w1), b1=_c(b1), masks=out, B=B, N=N, J=J, G=groups, posdim=vs.shape[-1], stream=capi.stream(),
              opts=capi.deform_opts(log_distance=bool(log_distance)))
    capi.check(capi.call("smml_deform_attn_relu1_masks", ns, RELU1_KEYS), "relu1_masks")
    return out


class _ZeroPool:
    """Small zero-initialised fp32 tensors (weight / bias gradients that kernels accumulate into with atomics) carved out
    of one pre-zeroed slab per device: one fill kernel per slab instead of one per tensor (a training step asked for ~40
    of them, each a launch-bound 2-5 us).  Slices are never reused - a slab is dropped when it runs out and lives on
    only as long as its slices do - so a tensor handed out here is as private as torch.zeros(...) would be."""
    SLAB = 1 << 20            # floats (4 MiB)
    LIMIT = 1 << 16           # larger requests go to torch.zeros directly

    def __init__(self):
        self.slabs = {}
        self.enabled = os.environ.get("SMML_ZERO_POOL", "1") != "0"   # measurement switch

    def zeros(self, shape, device) -> torch.Tensor:
        shape = tuple(int(d) for d in shape)
        n = 1
        for d in shape:
            n *= d
        # Under hipGraph capture a pooled slice would be zero only in the capture run: the slab's fill is not part of the graph, so a
        # replay would accumulate onto the previous replay's sums.  torch.zeros inside a capture allocates from the graph's private pool
        # and its fill IS a node of the graph - re-zeroed by every replay.
        if (n == 0 or n > self.LIMIT or torch.device(device).type != "cuda" or not self.enabled
                or torch.cuda.is_current_stream_capturing()):
            return torch.zeros(shape, device=device, dtype=torch.float32)
        key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
        buf, used = self.slabs.get(key, (None, self.SLAB))
        n4 = (n + 3) & ~3                                    # keep every slice 16-byte aligned
        if used + n4 > self.SLAB:
            buf, used = torch.zeros(self.SLAB, device=device, dtype=torch.float32), 0
        self.slabs[key] = (buf, used + n4)
        return buf[used:used + n].view(shape)


_ZEROS = _ZeroPool()


def _zeros_like(t: torch.Tensor) -> torch.Tensor:
    return _ZEROS.zeros(t.shape, t.device)


def _c(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def _al16(*tensors) -> bool:
    """every tensor starts on a 16-byte boundary (float4 loads)"""
    return all(t.data_ptr() % 16 == 0 for t in tensors)


def _gemm(A, B, C, *, M, N, K, sam, sak, sbk, sbn, ldc, bias=None, bias_mode=0, rows_per_bias=1, bias_ld=0,
          residual=None, ldr=0, act=ACT_NONE, splitk=1, alpha=1.0, nb0=1, nb1=1, sa0=0, sa1=0, sb0=0, sb1=0,
          sc0=0, sc1=0, sbias0=0, sbias1=0, beta=1.0, accumulate=0, det=False):
    """det (the caller's deterministic choice, taken in its forward): products whose slices or batch items add up in one C (splitk > 1 or
    accumulate) go through smml_gemm_f32_det, which OVERWRITES C with the fixed-order sum - the caller need not zero it."""
    if det and (splitk > 1 or accumulate):
        L = capi.lib()
        wsb = L.smml_gemm_f32_det_workspace_bytes(M, N, nb0, nb1, splitk)
        ws = _scratch(wsb, C.device)
        capi.check(L.smml_gemm_f32_det(
            capi.fptr(A), capi.fptr(B), capi.fptr(C), None, None, M, N, K, sam, sak, sbk, sbn, ldc, 0, nb0, nb1, sa0, sa1, sb0, sb1, sc0, sc1,
            0, 0, 0, 1, 0, 0, splitk, 0, float(alpha), 1.0, capi.fptr(ws), wsb, capi.stream()), "gemm (deterministic)")
        return
    capi.check(capi.lib().smml_gemm_f32(
        capi.fptr(A), capi.fptr(B), capi.fptr(C), capi.fptr(bias), capi.fptr(residual), M, N, K,
        sam, sak, sbk, sbn, ldc, ldr, nb0, nb1, sa0, sa1, sb0, sb1, sc0, sc1, sbias0, sbias1,
        bias_mode, rows_per_bias, bias_ld, act, splitk, accumulate, float(alpha), float(beta), capi.stream()), "gemm")


class _prec:
    """GEMM precision mode (include/smml.h smml_gemm_set_mode) for the launches issued inside the block; mode 0 / None = leave."""

    def __init__(self, mode):
        self.mode = int(mode or 0)

    def __enter__(self):
        if self.mode:
            L = capi.lib()
            self.prev = L.smml_gemm_get_mode()
            L.smml_gemm_set_mode(self.mode)

    def __exit__(self, *a):
        if self.mode:
            capi.lib().smml_gemm_set_mode(self.prev)


def _splitk_for(out_rows: int, out_cols: int, k: int, batches: int = 1) -> int:
    tiles = ((out_rows + 127) // 128) * ((out_cols + 63) // 64) * batches
    want = max(1, 1024 // max(tiles, 1))
    return int(max(1, min(want, (k + 255) // 256, 65535 // max(batches, 1))))


def colsum(x2d_or_3d: torch.Tensor, scale: float = 1.0, det: Optional[bool] = None) -> torch.Tensor:
    """x [nb, R, C] -> [nb, C] column sums * scale.  det: the deterministic choice of the calling Function (None: the switch as it stands)."""
    x = x2d_or_3d
    nb, R, Cc = x.shape
    if DETERMINISTIC if det is None else det:
        L = capi.lib()
        out = torch.empty(nb, Cc, device=x.device, dtype=torch.float32)
        wsb = L.smml_colsum_det_workspace_bytes(nb, R, Cc)
        ws = _scratch(wsb, x.device)
        capi.check(L.smml_colsum_det_f32(capi.fptr(x), capi.fptr(out), nb, R, Cc, float(scale), capi.fptr(ws), wsb, capi.stream()),
                   "colsum (deterministic)")
        return out
    out = _ZEROS.zeros((nb, Cc), x.device)
    capi.check(capi.lib().smml_colsum_f32(capi.fptr(x), capi.fptr(out), nb, R, Cc, float(scale), capi.stream()), "colsum")
    return out


# ------------------------------------------------------------------------------------------------
# A gradient that two kernels produce, summed by the second of them
# ------------------------------------------------------------------------------------------------
GRAD_SUM = os.environ.get("SMML_GRAD_SUM", "1") != "0"       # measurement switch, beside deform_attention._GRAD_FORK


class GradSum:
    """A tensor that feeds two of this module's ops - `linear` (as x or as residual) and `layer_norm` - gets two [B, N, C] gradients that
    autograd would add with an elementwise kernel: two reads and a write of the tensor right after the second producer wrote its half.
    With a GradSum riding on the tensor (grad_sum below) the producer that runs FIRST parks its gradient here and returns it to autograd as
    usual; the one that runs SECOND adds its own contribution into that buffer in place - the LayerNorm backward with accumulate_dx = 1,
    the linear's dX product through the GEMM's residual epilogue (C = 1 * parked + A B, residual aliased to C) - and reports no gradient
    of its own.  Either way a + b is rounded once in fp32: the bits of the ATen add.  Whichever order autograd picks is handled; a
    parked gradient is only taken inside the backward pass that parked it (the engine's graph-task id), so partial or repeated backward
    passes fall back to plain autograd, as does a tensor the second producer cannot add into.

    Contract of the caller that attaches one: every consumer of the tensor is a `linear` / `layer_norm` of this module (a gradient that
    ATen adds BETWEEN the park and the take would be summed out of place and miss the second half), and the gradient a parking
    `linear(residual=...)` receives has no other reader (it is the buffer that is added into)."""
    __slots__ = ("parked", "owner", "task")

    def __init__(self):
        self.parked = self.owner = self.task = None

    @staticmethod
    def _task():
        fn = getattr(torch._C, "_current_graph_task_id", None)
        t = fn() if fn is not None else -1
        return None if t < 0 else t

    def take(self, who: str, like: torch.Tensor) -> Optional[torch.Tensor]:
        """The gradient the OTHER producer parked in this backward pass, if `who` can add into it; the slot is emptied."""
        t, task = self.parked, self._task()
        if t is None or self.owner == who or task is None or self.task != task:
            return None                       # nothing there, or a leftover of this producer / of another pass: park() replaces it
        self.parked = self.owner = self.task = None
        ok = t.dtype == torch.float32 and t.is_contiguous() and t.shape == like.shape and t.device == like.device and t.data_ptr() % 16 == 0
        return t if ok else None

    def park(self, who: str, t: torch.Tensor) -> None:
        task = self._task()
        self.parked, self.owner, self.task = (t, who, task) if task is not None else (None, None, None)


def grad_sum(t: torch.Tensor) -> torch.Tensor:
    """Attaches a fresh GradSum to t (see its contract) and returns t; a no-op with the switch off or where t needs no gradient."""
    if GRAD_SUM and t.requires_grad:
        t._smml_grad_sum = GradSum()
    return t


def _fork_of(t) -> Optional[GradSum]:
    return getattr(t, "_smml_grad_sum", None) if (GRAD_SUM and t is not None) else None


# ------------------------------------------------------------------------------------------------
# y = act(x W^T + bias) [+ residual]; bias is [N] or one row per block of `rows_per_bias` rows
# ------------------------------------------------------------------------------------------------
class _Linear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, act, rows_per_bias, residual, prec=0, xfork=None, rfork=None):
        ctx.xfork, ctx.rfork = xfork, rfork
        x = _c(x); weight = _c(weight)
        ctx.det = DETERMINISTIC
        ctx.prec = 3 if prec == 4 else prec          # fp16 operands are for forward-range values: the gradient products of mode 4 run in bf16
        K = x.shape[-1]
        M = x.numel() // K
        N = weight.shape[0]
        y = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.float32)
        bias_mode = 0
        if bias is not None:
            bias = _c(bias)
            bias_mode = 2 if bias.dim() == 2 else 1
        res = _c(residual) if residual is not None else None
        with _prec(prec):
            _gemm(x, weight, y, M=M, N=N, K=K, sam=K, sak=1, sbk=1, sbn=K, ldc=N, bias=bias, bias_mode=bias_mode,
                  rows_per_bias=rows_per_bias, bias_ld=N, residual=res, ldr=N, act=act)
        ctx.act, ctx.rows_per_bias, ctx.bias_mode = act, rows_per_bias, bias_mode
        ctx.has_res = residual is not None
        ctx.save_for_backward(x, weight, y if act != ACT_NONE else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        dy = _c(dy)
        K = x.shape[-1]
        M = x.numel() // K
        N = weight.shape[0]
        dres = dy if ctx.has_res else None
        if dres is not None and ctx.rfork is not None and ctx.needs_input_grad[5]:
            ctx.rfork.park("linear", dres)         # GradSum: the residual's other consumer adds its gradient into this buffer
        if ctx.act == ACT_RELU:
            dpre = torch.empty_like(dy)
            capi.check(capi.lib().smml_relu_bwd_f32(capi.fptr(dy), capi.fptr(y), capi.fptr(dpre), dy.numel(),
                                                    capi.stream()), "relu_bwd")
        elif ctx.act == ACT_TANH:
            dpre = dy * (1.0 - y * y)          # only ever [B, C]-sized (Pooler)
        elif ctx.act == ACT_SIGMOID:
            dpre = dy * (y * (1.0 - y))
        elif ctx.act == ACT_TANH_SIGMOID:          # the gated pooling forms these in its own backward kernel (attention_pool_gated)
            yv, yu = y[..., :N // 2], y[..., N // 2:]
            dpre = dy * torch.cat((1.0 - yv * yv, yu * (1.0 - yu)), dim=-1)
        else:
            dpre = dy
        dx = dw = db = None
        with _prec(ctx.prec):
            if ctx.needs_input_grad[0]:
                parked = ctx.xfork.take("linear", x) if ctx.xfork is not None else None
                if parked is not None:             # GradSum: x's other gradient is there - parked = 1 * parked + dpre W, in place
                    _gemm(dpre, weight, parked, M=M, N=K, K=N, sam=N, sak=1, sbk=K, sbn=1, ldc=K, residual=parked, ldr=K)
                else:
                    dx = torch.empty_like(x)
                    _gemm(dpre, weight, dx, M=M, N=K, K=N, sam=N, sak=1, sbk=K, sbn=1, ldc=K)
                    if ctx.xfork is not None:
                        ctx.xfork.park("linear", dx)
            if ctx.needs_input_grad[1]:
                dw = torch.empty_like(weight) if ctx.det else _zeros_like(weight)
                _gemm(dpre, x, dw, M=N, N=K, K=M, sam=1, sak=N, sbk=K, sbn=1, ldc=K, splitk=_splitk_for(N, K, M), det=ctx.det)
        if ctx.bias_mode and ctx.needs_input_grad[2]:
            if ctx.bias_mode == 1:
                db = colsum(dpre.reshape(1, M, N), det=ctx.det)[0]
            else:
                db = colsum(dpre.reshape(M // ctx.rows_per_bias, ctx.rows_per_bias, N), det=ctx.det)
        return dx, dw, db, None, None, dres, None, None, None


def linear(x, weight, bias=None, act: int = ACT_NONE, rows_per_bias: int = 1, residual=None, prec: int = 0):
    """act(x W^T + bias) (+ residual).  prec: GEMM precision mode of the forward and backward products (0 automatic / exact
    fp32, 2 three-term split bf16, 3 single-term bf16 operands - the 16-bit compute mode, 4 single-term fp16 operands in the forward
    product and bf16 ones in the two gradient products - the fp16 compute modes).
    act: ACT_NONE, ACT_RELU, ACT_TANH, ACT_SIGMOID or ACT_TANH_SIGMOID (tanh on the first half of the output columns, sigmoid on the second;
    an odd number of columns raises ValueError)."""
    if act == ACT_TANH_SIGMOID and weight.shape[0] % 2:
        raise ValueError(f"linear: ACT_TANH_SIGMOID splits the output columns in halves, got an odd N = {weight.shape[0]}")
    # a GradSum riding on x or on the residual (grad_sum): their gradients meet the other consumer's in one buffer
    return _Linear.apply(x, weight, bias, act, rows_per_bias, residual, prec, _fork_of(x), _fork_of(residual))


# ------------------------------------------------------------------------------------------------
# two ReLU(Linear) heads over ONE input: the two branches of DeformPathomicNet read the same bag (models/model.py:488-497,
# SURVEY.md K1) - one batched launch per direction, the bag's rows are addressed once per launch instead of once per branch
# ------------------------------------------------------------------------------------------------
class _DualLinearRelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1):
        x = _c(x)
        ctx.det = DETERMINISTIC
        K = x.shape[-1]
        M = x.numel() // K
        N = w0.shape[0]
        w = torch.stack((_c(w0), _c(w1)))                       # [2, N, K]
        b = torch.stack((_c(b0), _c(b1)))                       # [2, N]
        y = torch.empty(2, *x.shape[:-1], N, device=x.device, dtype=torch.float32)
        _gemm(x, w, y, M=M, N=N, K=K, sam=K, sak=1, sbk=1, sbn=K, ldc=N, bias=b, bias_mode=1, act=ACT_RELU, nb1=2, sa1=0,
              sb1=N * K, sc1=M * N, sbias1=N)
        ctx.save_for_backward(x, y)
        return y[0], y[1]

    @staticmethod
    def backward(ctx, dy0, dy1):
        x, y = ctx.saved_tensors
        K = x.shape[-1]
        M = x.numel() // K
        N = y.shape[-1]
        L = capi.lib()
        dpre = torch.empty_like(y)
        for i, dy in enumerate((dy0, dy1)):
            capi.check(L.smml_relu_bwd_f32(capi.fptr(_c(dy)), capi.fptr(y[i]), capi.fptr(dpre[i]), dy.numel(), capi.stream()), "relu_bwd")
        dx = None
        if ctx.needs_input_grad[0]:
            raise RuntimeError("dual_linear_relu: the shared input is a bag of features (no gradient path is built)")
        dw = torch.empty(2, N, K, device=x.device, dtype=torch.float32) if ctx.det else _ZEROS.zeros((2, N, K), x.device)
        _gemm(dpre, x, dw, M=N, N=K, K=M, sam=1, sak=N, sbk=K, sbn=1, ldc=K, nb1=2, sa1=M * N, sb1=0, sc1=N * K,
              splitk=_splitk_for(N, K, M, 2), det=ctx.det)
        db = colsum(dpre.reshape(2, M, N), det=ctx.det)
        return dx, dw[0], db[0], dw[1], db[1]


def dual_linear_relu(x, w0, b0, w1, b1):
    """(relu(x w0^T + b0), relu(x w1^T + b1)) for two heads of equal shape over one input."""
    return _DualLinearRelu.apply(x, w0, b0, w1, b1)


# ------------------------------------------------------------------------------------------------
# attention pooling of ABMIL (models/mil.py:66-75, csrc/attn_pool.hip): M[b] = sum_n softmax_n(h[b, n] . w2 + b2) x[b, n] - one streaming
# pass over the bag with an online softmax, per-split partials merged in a fixed order
# ------------------------------------------------------------------------------------------------
POOL_MAX_L, POOL_MAX_D = 1024, 256


def _pool_check(x, h, w2, b2):
    """Shapes the pooling kernels are built for (include/smml.h); raises ValueError before anything is launched."""
    if x.dim() != 3 or h.dim() != 3 or tuple(h.shape[:2]) != tuple(x.shape[:2]):
        raise ValueError(f"attention_pool: need x [B, N, L] and h [B, N, D] over the same bag, got {tuple(x.shape)} and {tuple(h.shape)}")
    B, N, L = x.shape
    D = h.shape[-1]
    if N < 1 or B < 1:
        raise ValueError(f"attention_pool: empty bag ({tuple(x.shape)})")
    if L % 256 or not 0 < L <= POOL_MAX_L:
        raise ValueError(f"attention_pool: the feature width L must be a multiple of 256 up to {POOL_MAX_L}, got {L}")
    if D % 64 or not 0 < D <= POOL_MAX_D:
        raise ValueError(f"attention_pool: the hidden width D must be a multiple of 64 up to {POOL_MAX_D}, got {D}")
    if w2.numel() != D or b2.numel() != 1:
        raise ValueError(f"attention_pool: one attention map (K = 1) - w2 must hold D = {D} values and b2 one, got {tuple(w2.shape)} and "
                         f"{tuple(b2.shape)}")
    return B, N, L, D


class _AttnPool(torch.autograd.Function):
    """hidden = False: h is an ordinary input and receives dh = ds w2.  hidden = True: h = tanh(x w1^T + b1) was formed outside the graph;
    the backward kernel writes the pre-activation gradient ds w2 (1 - h^2) in the same pass and dw1 / db1 come from it exactly as
    _Linear.backward forms them - no elementwise pass over a [B, N, D] tensor."""

    @staticmethod
    def forward(ctx, x, h, w2, b2, w1, b1, splits, scores_out):
        B, N, L, D = _pool_check(x, h, w2, b2)
        ctx.w2_shape, ctx.b2_shape = w2.shape, b2.shape
        x = _c(x); h = _c(h); w2 = _c(w2).reshape(D); b2 = _c(b2).reshape(1)
        ctx.det = DETERMINISTIC          # the pooling kernels have one form; the choice goes to the two reductions of the hidden layer's gradients
        ctx.hidden = w1 is not None
        ctx.splits = int(splits or 0)
        Lb = capi.lib()
        s = torch.empty(B, N, device=x.device, dtype=torch.float32)
        M = torch.empty(B, L, device=x.device, dtype=torch.float32)
        lse = torch.empty(B, device=x.device, dtype=torch.float32)
        wsb = Lb.smml_attn_pool_fwd_workspace_bytes(B, N, L, ctx.splits)
        ws = _scratch(wsb, x.device)
        capi.check(Lb.smml_attn_pool_fwd_f32(capi.fptr(x), capi.fptr(h), capi.fptr(w2), capi.fptr(b2), capi.fptr(s), capi.fptr(M), capi.fptr(lse),
                                             capi.fptr(ws), wsb, B, N, L, D, ctx.splits, capi.stream()), "attn_pool_fwd")
        if scores_out is not None:
            scores_out[:] = [s, lse]
        ctx.save_for_backward(x, h, w2, s, lse)      # M is not needed: the backward forms dM . M from its own row dots (csrc/attn_pool.hip)
        return M

    @staticmethod
    def backward(ctx, dM):
        x, h, w2, s, lse = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise RuntimeError("attention_pool: the pooled input is a bag of features (no gradient path is built)")
        B, N, L = x.shape
        D = h.shape[-1]
        dM = _c(dM)
        Lb = capi.lib()
        dh = torch.empty_like(h)
        dw2 = torch.empty(D, device=x.device, dtype=torch.float32)
        db2 = torch.empty(1, device=x.device, dtype=torch.float32)
        wsb = Lb.smml_attn_pool_bwd_workspace_bytes(B, N, D, ctx.splits)
        ws = _scratch(wsb, x.device)
        capi.check(Lb.smml_attn_pool_bwd_f32(capi.fptr(x), capi.fptr(h), capi.fptr(w2), capi.fptr(s), capi.fptr(lse), capi.fptr(dM),
                                             capi.fptr(dh), capi.fptr(dw2), capi.fptr(db2), capi.fptr(ws), wsb, B, N, L, D, ctx.splits,
                                             1 if ctx.hidden else 0, capi.stream()), "attn_pool_bwd")
        dw1 = db1 = None
        if ctx.hidden:
            R = B * N
            if ctx.needs_input_grad[4]:
                dw1 = torch.empty(D, L, device=x.device, dtype=torch.float32) if ctx.det else _ZEROS.zeros((D, L), x.device)
                _gemm(dh, x, dw1, M=D, N=L, K=R, sam=1, sak=D, sbk=L, sbn=1, ldc=L, splitk=_splitk_for(D, L, R), det=ctx.det)
            if ctx.needs_input_grad[5]:
                db1 = colsum(dh.reshape(1, R, D), det=ctx.det)[0]
            dh = None
        return None, dh, dw2.view(ctx.w2_shape), db2.view(ctx.b2_shape), dw1, db1, None, None


def attention_pool(x, h, w2, b2, *, hidden=None, splits=None, scores_out=None):
    """M [B, L] = sum_n softmax_n(h[b, n, :] . w2 + b2) x[b, n, :] for a bag x [B, N, L] and its hidden features h [B, N, D] (one attention
    map: w2 holds D values, b2 one).  L a multiple of 256 up to 1024, D a multiple of 64 up to 256, any N >= 1; other shapes raise
    ValueError.  x is a bag of features: it receives no gradient (x.requires_grad makes the backward raise RuntimeError).

    hidden = (w1, b1): h is tanh(x w1^T + b1) formed WITHOUT autograd (linear(x, w1, b1, act=ACT_TANH) on detached operands or under
    no_grad); the gradients of w1 and b1 are then produced here, from the pre-activation gradient the backward kernel writes in its one pass.
    Without it h is an ordinary differentiable input.
    splits: how many pieces a bag's rows are cut into (None: chosen by the library so that B x splits fills the chip); the result is a
    function of the inputs and this number alone.  scores_out: a list that receives [s [B, N], lse [B]], the raw scores and their
    log-sum-exp - softmax = exp(s - lse[:, None])."""
    _pool_check(x, h, w2, b2)
    w1, b1 = hidden if hidden is not None else (None, None)
    if hidden is not None and h.requires_grad:
        raise ValueError("attention_pool: with hidden = (w1, b1) h must be formed outside the autograd graph (its gradient is folded into dw1 / db1)")
    return _AttnPool.apply(x, h, w2, b2, w1, b1, splits, scores_out)


# ------------------------------------------------------------------------------------------------
# gated attention pooling (GatedABMIL, models/mil.py:102-152; csrc/attn_pool.hip): the score is sum_d w_d tanh(.)_d sigmoid(.)_d + b, the two
# hidden tensors are the halves of ONE buffer h2 [B, N, 2 D] - the output of one GEMM over x with the stacked weight [Wv; Wu]
# ------------------------------------------------------------------------------------------------
def _pool_gated_check(x, h2, w, b):
    """Shapes the gated pooling kernels are built for (include/smml.h); raises ValueError before anything is launched."""
    if x.dim() != 3 or h2.dim() != 3 or tuple(h2.shape[:2]) != tuple(x.shape[:2]):
        raise ValueError(f"attention_pool_gated: need x [B, N, L] and h2 [B, N, 2 D] over the same bag, got {tuple(x.shape)} and "
                         f"{tuple(h2.shape)}")
    B, N, L = x.shape
    D2 = h2.shape[-1]
    if N < 1 or B < 1:
        raise ValueError(f"attention_pool_gated: empty bag ({tuple(x.shape)})")
    if L % 256 or not 0 < L <= POOL_MAX_L:
        raise ValueError(f"attention_pool_gated: the feature width L must be a multiple of 256 up to {POOL_MAX_L}, got {L}")
    if D2 % 128 or not 0 < D2 <= 2 * POOL_MAX_D:
        raise ValueError(f"attention_pool_gated: h2 holds the tanh and the sigmoid half side by side - its width 2 D must be a multiple of "
                         f"128 up to {2 * POOL_MAX_D}, got {D2}")
    D = D2 // 2
    if w.numel() != D or b.numel() != 1:
        raise ValueError(f"attention_pool_gated: one attention map (K = 1) - w must hold D = {D} values and b one, got {tuple(w.shape)} and "
                         f"{tuple(b.shape)}")
    return B, N, L, D


class _AttnPoolGated(torch.autograd.Function):
    """hidden = False: h2 is an ordinary input and receives dh2 = (g hu | g hv), g = ds w.  hidden = True: h2 = (tanh(x Wv^T + bv) |
    sigmoid(x Wu^T + bu)) was formed outside the graph; the backward kernel writes the gradient of the stacked pre-activation in the same
    pass, one GEMM over x yields d[Wv; Wu] and one column sum d[bv; bu] - both split by views."""

    @staticmethod
    def forward(ctx, x, h2, w, b, wv, bv, wu, bu, splits, scores_out):
        B, N, L, D = _pool_gated_check(x, h2, w, b)
        ctx.w_shape, ctx.b_shape = w.shape, b.shape
        x = _c(x); h2 = _c(h2); w = _c(w).reshape(D); b = _c(b).reshape(1)
        ctx.det = DETERMINISTIC          # the pooling kernels have one form; the choice goes to the two reductions of the hidden layer's gradients
        ctx.hidden = wv is not None
        ctx.splits = int(splits or 0)
        Lb = capi.lib()
        s = torch.empty(B, N, device=x.device, dtype=torch.float32)
        M = torch.empty(B, L, device=x.device, dtype=torch.float32)
        lse = torch.empty(B, device=x.device, dtype=torch.float32)
        wsb = Lb.smml_attn_pool_fwd_workspace_bytes(B, N, L, ctx.splits)
        ws = _scratch(wsb, x.device)
        capi.check(Lb.smml_attn_pool_gated_fwd_f32(capi.fptr(x), capi.fptr(h2), capi.fptr(w), capi.fptr(b), capi.fptr(s), capi.fptr(M),
                                                   capi.fptr(lse), capi.fptr(ws), wsb, B, N, L, D, ctx.splits, capi.stream()),
                   "attn_pool_gated_fwd")
        if scores_out is not None:
            scores_out[:] = [s, lse]
        ctx.save_for_backward(x, h2, w, s, lse)
        return M

    @staticmethod
    def backward(ctx, dM):
        x, h2, w, s, lse = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise RuntimeError("attention_pool_gated: the pooled input is a bag of features (no gradient path is built)")
        B, N, L = x.shape
        D = h2.shape[-1] // 2
        dM = _c(dM)
        Lb = capi.lib()
        dh2 = torch.empty_like(h2)
        dw = torch.empty(D, device=x.device, dtype=torch.float32)
        db = torch.empty(1, device=x.device, dtype=torch.float32)
        wsb = Lb.smml_attn_pool_bwd_workspace_bytes(B, N, D, ctx.splits)
        ws = _scratch(wsb, x.device)
        capi.check(Lb.smml_attn_pool_gated_bwd_f32(capi.fptr(x), capi.fptr(h2), capi.fptr(w), capi.fptr(s), capi.fptr(lse), capi.fptr(dM),
                                                   capi.fptr(dh2), capi.fptr(dw), capi.fptr(db), capi.fptr(ws), wsb, B, N, L, D, ctx.splits,
                                                   1 if ctx.hidden else 0, capi.stream()), "attn_pool_gated_bwd")
        dwv = dbv = dwu = dbu = None
        if ctx.hidden:
            R = B * N
            if ctx.needs_input_grad[4] or ctx.needs_input_grad[6]:
                dwvu = torch.empty(2 * D, L, device=x.device, dtype=torch.float32) if ctx.det else _ZEROS.zeros((2 * D, L), x.device)
                _gemm(dh2, x, dwvu, M=2 * D, N=L, K=R, sam=1, sak=2 * D, sbk=L, sbn=1, ldc=L, splitk=_splitk_for(2 * D, L, R), det=ctx.det)
                dwv, dwu = dwvu[:D], dwvu[D:]
            if ctx.needs_input_grad[5] or ctx.needs_input_grad[7]:
                dbvu = colsum(dh2.reshape(1, R, 2 * D), det=ctx.det)[0]
                dbv, dbu = dbvu[:D], dbvu[D:]
            dh2 = None
        return None, dh2, dw.view(ctx.w_shape), db.view(ctx.b_shape), dwv, dbv, dwu, dbu, None, None


def attention_pool_gated(x, h2, w, b, *, hidden=None, splits=None, scores_out=None):
    """M [B, L] = sum_n softmax_n(sum_d w_d hv[b, n, d] hu[b, n, d] + b) x[b, n, :] for a bag x [B, N, L] and its two gates in ONE tensor
    h2 [B, N, 2 D]: hv = h2[..., :D] (the tanh units) and hu = h2[..., D:] (the sigmoid units); one attention map: w holds D values, b one.
    L a multiple of 256 up to 1024, D a multiple of 64 up to 256, any N >= 1; other shapes raise ValueError.  x is a bag of features: it
    receives no gradient (x.requires_grad makes the backward raise RuntimeError).

    hidden = (Wv, bv, Wu, bu): h2 is linear(x, cat(Wv, Wu), cat(bv, bu), act=ACT_TANH_SIGMOID) formed WITHOUT autograd (detached operands or
    no_grad); the four gradients are then produced here, from the pre-activation gradient the backward kernel writes in its one pass.
    Without it h2 is an ordinary differentiable input.  splits, scores_out: as in attention_pool."""
    _pool_gated_check(x, h2, w, b)
    wv, bv, wu, bu = hidden if hidden is not None else (None, None, None, None)
    if hidden is not None and h2.requires_grad:
        raise ValueError("attention_pool_gated: with hidden = (Wv, bv, Wu, bu) h2 must be formed outside the autograd graph (its gradient is "
                         "folded into the four parameter gradients)")
    return _AttnPoolGated.apply(x, h2, w, b, wv, bv, wu, bu, splits, scores_out)


# ------------------------------------------------------------------------------------------------
# few-query co-attention (models/MultiheadAttention.py with one head and L <= 8 queries over a bag; csrc/fewq_attn.hip): with
# q^ = (query Wq^T + bq) scaling, raw = u . x_s + c for u = q^ Wk, c = q^ . bk and the output is Wv z + bv for z = sum_s softmax(raw) y_s -
# the key / value projections fold into [B, L, E]-sized products and the bag streams once through few_query_attention
# ------------------------------------------------------------------------------------------------
FEWQ_MAX_L, FEWQ_MAX_E = 8, 512


def _fewq_width_ok(E: int) -> bool:
    return 0 < E <= FEWQ_MAX_E and E % 64 == 0


def coattn_why(*, L: int, heads: int, Ek: int, Ev: int, attn_mask: bool = False, add_bias_kv: bool = False, add_zero_attn: bool = False,
               dropout_active: bool = False, fused: bool = True) -> Optional[str]:
    """Why a MultiheadAttention call with L queries, `heads` heads and raw key / value widths Ek / Ev stays on the composed path (two
    bag-sized projections, matmul4, softmax_rows, matmul4); None: it takes the few-query kernels.  No GPU work."""
    if not fused:
        return "fused_few_query is off (the default)"
    if heads != 1:
        return f"{heads} heads (the few-query kernels are one-head)"
    if not 1 <= L <= FEWQ_MAX_L:
        return f"{L} queries (at most {FEWQ_MAX_L})"
    if attn_mask:
        return "an attn_mask (only key_padding_mask is fused)"
    if add_bias_kv:
        return "add_bias_kv (a learned key / value row outside the bag)"
    if add_zero_attn:
        return "add_zero_attn (a zero key / value row outside the bag)"
    if dropout_active:
        return "active attention dropout"
    if not _fewq_width_ok(Ek) or not _fewq_width_ok(Ev):
        return f"key / value widths {Ek} / {Ev} (multiples of 64 up to {FEWQ_MAX_E})"
    return None


def coattn_path(**kw) -> str:
    """'fewq' (the folded form on csrc/fewq_attn.hip) or 'composed' for a MultiheadAttention call: the arguments of coattn_why, which names
    the reason for 'composed'."""
    return "composed" if coattn_why(**kw) is not None else "fewq"


def _fewq_check(u, c, x, y):
    """Shapes the few-query kernels are built for (include/smml.h); raises ValueError before anything is launched."""
    if u.dim() != 3 or x.dim() != 3 or y.dim() != 3 or c.dim() != 2:
        raise ValueError(f"few_query_attention: need u [B, L, Ek], c [B, L], x [B, S, Ek], y [B, S, Ev], got {tuple(u.shape)}, {tuple(c.shape)}, "
                         f"{tuple(x.shape)}, {tuple(y.shape)}")
    B, L, Ek = u.shape
    S, Ev = x.shape[1], y.shape[2]
    if tuple(c.shape) != (B, L) or tuple(x.shape) != (B, S, Ek) or tuple(y.shape[:2]) != (B, S):
        raise ValueError(f"few_query_attention: u {tuple(u.shape)}, c {tuple(c.shape)}, x {tuple(x.shape)} and y {tuple(y.shape)} do not "
                         "describe one problem")
    if B < 1 or S < 1:
        raise ValueError(f"few_query_attention: empty bag ({tuple(x.shape)})")
    if not 1 <= L <= FEWQ_MAX_L:
        raise ValueError(f"few_query_attention: at most {FEWQ_MAX_L} queries, got {L}")
    if not _fewq_width_ok(Ek) or not _fewq_width_ok(Ev):
        raise ValueError(f"few_query_attention: the key and value widths must be multiples of 64 up to {FEWQ_MAX_E}, got {Ek} and {Ev}")
    return B, L, S, Ek, Ev


def _rows(t: torch.Tensor) -> torch.Tensor:
    """t [B, S, E] as the kernels read it in place: fp32, unit column stride, rows and bags a multiple of 4 floats apart, 16-byte aligned -
    a slice of a longer bag or a sequence-first tensor's transpose qualifies; anything else is copied."""
    if t.dtype != torch.float32:
        t = t.float()
    B, S, E = t.shape
    ok = (t.stride(2) == 1 and t.stride(1) >= E and t.stride(1) % 4 == 0 and (t.stride(0) % 4 == 0 or B == 1) and t.data_ptr() % 16 == 0)
    return t if ok else t.contiguous()


def _rows_ptr(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda or t.device.index != torch.cuda.current_device():
        raise RuntimeError(f"smml kernels need fp32 tensors on the current device (cuda:{torch.cuda.current_device()}), got {t.device}; "
                           "this path has no CPU fallback")
    return C_.c_void_p(t.data_ptr())


def _bs(t: torch.Tensor) -> int:
    return int(t.stride(0)) if t.shape[0] > 1 else 0


def _grad_rows(t: torch.Tensor) -> torch.Tensor:
    """An uninitialised gradient buffer for the rows t: t's own layout where that is dense (a sequence-first tensor gets its gradient
    sequence-first, no copy on the way to .grad), contiguous otherwise."""
    if t.transpose(0, 1).is_contiguous():
        return torch.empty_strided(t.shape, t.stride(), device=t.device, dtype=torch.float32)
    return torch.empty(t.shape, device=t.device, dtype=torch.float32)


def _fewq_fwd(u, c, x, yv, mask, splits: int):
    """One launch of the forward core on checked operands (u, c dense; x, yv as _rows leaves them; yv is x: the values are the keys)."""
    B, L, Ek = u.shape
    S, Ev = x.shape[1], yv.shape[2]
    Lb = capi.lib()
    z = torch.empty(B, L, Ev, device=x.device, dtype=torch.float32)
    raw = torch.empty(B, L, S, device=x.device, dtype=torch.float32)
    lse = torch.empty(B, L, device=x.device, dtype=torch.float32)
    wsb = Lb.smml_fewq_attn_fwd_workspace_bytes(B, L, S, Ev, splits)
    ws = _scratch(wsb, x.device)
    capi.check(Lb.smml_fewq_attn_fwd_f32(capi.fptr(u), capi.fptr(c), _rows_ptr(x), _rows_ptr(yv), capi.ptr(mask), capi.fptr(z), capi.fptr(raw),
                                         capi.fptr(lse), capi.fptr(ws), wsb, B, L, S, Ek, Ev, _bs(x), x.stride(1), _bs(yv), yv.stride(1),
                                         splits, capi.stream()), "fewq_attn_fwd")
    return z, raw, lse


def _fewq_bwd(u, x, y, raw, lse, z, dz, draw, dlse, want_dx: bool, want_dy: bool, splits: int):
    """One launch of the backward core -> (du, dc, dx, dy); y = None: the values are the keys and dx holds dx + dy.  dz / draw / dlse may
    be None (no gradient arrived for that output)."""
    yv = x if y is None else y
    B, L, Ek = u.shape
    S, Ev = x.shape[1], yv.shape[2]
    dz = _c(dz) if dz is not None else torch.zeros_like(z)
    draw = _c(draw) if draw is not None else None
    dlse = _c(dlse) if dlse is not None else None
    Lb = capi.lib()
    du = torch.empty_like(u)
    dc = torch.empty(B, L, device=x.device, dtype=torch.float32)
    dx = _grad_rows(x) if want_dx else None
    dy = _grad_rows(yv) if y is not None and want_dy else None
    wsb = Lb.smml_fewq_attn_bwd_workspace_bytes(B, L, S, Ek, splits)
    ws = _scratch(wsb, x.device)
    st = lambda t: (_bs(t), t.stride(1)) if t is not None else (0, 0)      # noqa: E731
    capi.check(Lb.smml_fewq_attn_bwd_f32(capi.fptr(u), _rows_ptr(x), _rows_ptr(yv), capi.fptr(raw), capi.fptr(lse), capi.fptr(z), capi.fptr(dz),
                                         capi.fptr(draw), capi.fptr(dlse), capi.fptr(du), capi.fptr(dc), _rows_ptr(dx), _rows_ptr(dy),
                                         capi.fptr(ws), wsb, B, L, S, Ek, Ev, *st(x), *st(yv), *st(dx), *st(dy), splits, capi.stream()),
               "fewq_attn_bwd")
    return du, dc, dx, dy


class _FewQueryAttention(torch.autograd.Function):
    """y = None: the value rows ARE the key rows - one read in the forward, one read and one written gradient row (dx + dy) in the backward."""

    @staticmethod
    def forward(ctx, u, c, x, y, mask, splits):
        B, L, S, Ek, Ev = _fewq_check(u, c, x, x if y is None else y)
        ctx.set_materialize_grads(False)
        u = _c(u); c = _c(c); x = _rows(x)
        yv = x if y is None else _value_rows(x, y)
        ctx.same = y is None
        ctx.splits = int(splits or 0)
        z, raw, lse = _fewq_fwd(u, c, x, yv, mask, ctx.splits)
        ctx.save_for_backward(u, x, None if ctx.same else yv, raw, lse, z)
        return z, raw, lse

    @staticmethod
    def backward(ctx, dz, draw, dlse):
        u, x, y, raw, lse, z = ctx.saved_tensors
        du, dc, dx, dy = _fewq_bwd(u, x, y, raw, lse, z, dz, draw, dlse, ctx.needs_input_grad[2],
                                   ctx.needs_input_grad[3], ctx.splits)
        return du, dc, dx, dy, None, None


def _same_rows(x: torch.Tensor, y: Optional[torch.Tensor]) -> bool:
    """y names x's rows AND the one gradient row dx + dy may go to x: the same tensor, two views of one base over the same memory (the two
    `bag.transpose(1, 0)` of a co-attention call: the base receives the sum either way), or aliases of which neither requires a gradient.
    A detached alias on one side (`mod(q, kv, kv.detach())`) is NOT the same rows: the side that requires a gradient gets its own part alone."""
    if y is None or y is x:
        return True
    if y.data_ptr() != x.data_ptr() or y.shape != x.shape or y.stride() != x.stride() or y.dtype != x.dtype:
        return False
    if y._base is not None and y._base is x._base:
        return True
    return not x.requires_grad and not y.requires_grad


def _value_rows(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """The value rows of the distinct form.  The C entry points read `y == x` (pointer and strides) as the one-row form; values that alias
    the keys without being the same rows for autograd (_same_rows) are therefore copied - the price of a call no model makes."""
    yv = _rows(y)
    same_memory = yv.data_ptr() == x.data_ptr() and yv.shape == x.shape and yv.stride() == x.stride()
    return yv.clone() if same_memory else yv


def few_query_attention(u, c, x, y=None, *, key_padding_mask=None, splits=None):
    """(z [B, L, Ev], raw [B, L, S], lse [B, L]) with raw[b, l, s] = u[b, l] . x[b, s] + c[b, l], z = sum_s softmax_s(raw) y[b, s] and
    lse = log sum_s exp(raw), for L <= 8 queries u [B, L, Ek], c [B, L] over a bag of keys x [B, S, Ek] and values y [B, S, Ev] - one
    streaming pass over the bag with an online softmax per query.  Ek and Ev multiples of 64 up to 512, any S >= 1; other shapes raise
    ValueError before anything is launched.  x and y are read in place when their columns are contiguous (a slice of a longer bag, the
    transpose of a sequence-first tensor).

    y = None (or x itself, or another view of x's base over the same memory): the values are the keys - the bag is read once, and x
    receives the ONE gradient row dx + dy.  A y that aliases x while only one of the two requires a gradient (x.detach()) is a distinct
    value tensor: it is copied and each side gets its own part alone.
    key_padding_mask [B, S] bool: masked keys get raw = -inf, weight 0 and a zero gradient row; a bag with every key masked gives NaN, as
    the reference does (not checked: that would be a host sync).
    All three outputs are differentiable; u, c, x and y receive gradients (x / y only where they require one - no buffer is written
    otherwise).
    splits: how many pieces a bag's rows are cut into (None: chosen by the library so that B x splits fills the chip); the result is a
    function of the inputs and this number alone - the same under functional.deterministic()."""
    same = _same_rows(x, y)
    _fewq_check(u, c, x, x if same else y)
    mask = None
    if key_padding_mask is not None:
        mask = key_padding_mask.to(torch.bool).contiguous().view(torch.uint8)
        if tuple(mask.shape) != (x.shape[0], x.shape[1]):
            raise ValueError(f"few_query_attention: key_padding_mask must be [B, S] = {(x.shape[0], x.shape[1])}, got {tuple(mask.shape)}")
    return _FewQueryAttention.apply(u, c, x, None if same else y, mask, splits)


def _lin(x2, w, b=None, alpha: float = 1.0):
    """alpha x2 [R, K] w [N, K]^T (+ b) -> [R, N]"""
    R, K = x2.shape
    N = w.shape[0]
    y = torch.empty(R, N, device=x2.device, dtype=torch.float32)
    _gemm(x2, w, y, M=R, N=N, K=K, sam=K, sak=1, sbk=1, sbn=K, ldc=N, bias=b, bias_mode=0 if b is None else 1, bias_ld=N, alpha=alpha)
    return y


def _mat(x2, w, alpha: float = 1.0):
    """alpha x2 [R, K] w [K, N] -> [R, N]"""
    R, K = x2.shape
    N = w.shape[1]
    y = torch.empty(R, N, device=x2.device, dtype=torch.float32)
    _gemm(x2, w, y, M=R, N=N, K=K, sam=K, sak=1, sbk=N, sbn=1, ldc=N, alpha=alpha)
    return y


def _wgrad(dy, x2, det: bool, alpha: float = 1.0):
    """alpha dy [R, N]^T x2 [R, K] -> [N, K], the weight gradient of _lin as _Linear.backward forms it"""
    R, N = dy.shape
    K = x2.shape[1]
    dw = torch.empty(N, K, device=dy.device, dtype=torch.float32) if det else _ZEROS.zeros((N, K), dy.device)
    _gemm(dy, x2, dw, M=N, N=K, K=R, sam=1, sak=N, sbk=K, sbn=1, ldc=K, splitk=_splitk_for(N, K, R), alpha=alpha, det=det)
    return dw


class _CoattnFewQuery(torch.autograd.Function):
    """The whole folded co-attention as ONE autograd node: the [B L, E]-sized products around the core are the same smml_gemm launches
    linear / matmul4 would issue (q^ = q Wq^T + bq; u = s q^ Wk, c = s q^ . bk with the scaling s as the products' alpha; Wv z + bv; the
    out-projection) and their gradients are formed as _Linear.backward forms them.  A chain of eight Functions computes the same values
    with the same kernels; at L <= 8 it spent several times the kernels' time in the host's per-node bookkeeping (33 launches against
    this node's 27: DESIGN.md 4c, profiles/coattn_fewq_kernel_stats.csv), which is what this node removes."""

    @staticmethod
    def forward(ctx, q, x, y, wq, bq, wk, bk, wv, bv, wo, bo, mask, splits, scaling):
        B, L, E = q.shape
        ctx.set_materialize_grads(False)
        ctx.det = DETERMINISTIC
        ctx.splits, ctx.scaling, ctx.same = int(splits or 0), float(scaling), y is None
        ctx.shapes = tuple(None if b is None else b.shape for b in (bq, bk, bv, bo))
        q2 = _c(q).reshape(B * L, E)
        wq, wk, wv, wo = _c(wq), _c(wk), _c(wv), _c(wo)
        bqc, bkc, bvc, boc = (None if b is None else _c(b).reshape(-1) for b in (bq, bk, bv, bo))
        x = _rows(x)
        yv = x if y is None else _value_rows(x, y)
        qh = _lin(q2, wq, bqc)
        u = _mat(qh, wk, alpha=ctx.scaling).view(B, L, -1)
        c = _lin(qh, bkc.view(1, E), alpha=ctx.scaling).view(B, L) if bkc is not None else torch.zeros(B, L, device=q.device)
        z, raw, lse = _fewq_fwd(u, c, x, yv, mask, ctx.splits)
        o = _lin(z.view(B * L, -1), wv, bvc)
        out = _lin(o, wo, boc).view(B, L, -1)
        ctx.save_for_backward(q2, qh, u, x, None if ctx.same else yv, raw, lse, z, o, wq, wk, bkc, wv, wo)
        return out, raw, lse

    @staticmethod
    def backward(ctx, dout, draw, dlse):
        q2, qh, u, x, y, raw, lse, z, o, wq, wk, bk, wv, wo = ctx.saved_tensors
        B, L, _ = u.shape
        R, s, det = B * L, ctx.scaling, ctx.det
        dout = (_c(dout) if dout is not None else torch.zeros(B, L, wo.shape[0], device=u.device)).reshape(R, -1)
        col = lambda g, shape: None if shape is None else colsum(g.reshape(1, R, -1), det=det)[0].view(shape)      # noqa: E731
        do = _mat(dout, wo)
        dwo, dbo = _wgrad(dout, o, det), col(dout, ctx.shapes[3])
        dz = _mat(do, wv).view(B, L, -1)
        dwv, dbv = _wgrad(do, z.view(R, -1), det), col(do, ctx.shapes[2])
        du, dc, dx, dy = _fewq_bwd(u, x, y, raw, lse, z, dz, draw, dlse, ctx.needs_input_grad[1], ctx.needs_input_grad[2], ctx.splits)
        du2, dc2 = du.view(R, -1), dc.view(R, 1)
        dqh = _lin(du2, wk, alpha=s)                                        # s du Wk^T ...
        dwk = _wgrad(qh, du2, det, alpha=s)
        dbk = None
        if bk is not None:
            dqh.addcmul_(dc2, bk.view(1, -1), value=s)                      # ... + s dc bk^T, [B L, E]-sized
            dbk = _wgrad(qh, dc2, det, alpha=s).view(ctx.shapes[1])
        dq = _mat(dqh, wq).view(B, L, -1) if ctx.needs_input_grad[0] else None
        dwq, dbq = _wgrad(dqh, q2, det), col(dqh, ctx.shapes[0])
        return dq, dx, dy, dwq, dbq, dwk, dbk, dwv, dbv, dwo, dbo, None, None, None


def coattn_few_query(q, x, y, wq, bq, wk, bk, wv, bv, wo, bo, *, scaling: float, key_padding_mask=None, splits=None):
    """(out [B, L, E], raw [B, L, S], lse [B, L]) of one-head co-attention in the folded form, batch first: q [B, L, E] queries, x [B, S, Ek]
    keys, y [B, S, Ev] values (None or x's rows: the values are the keys), Wq [E, E], Wk [E, Ek], Wv [E, Ev], Wo [E, E] and their biases
    (any may be None).  The bag-sized work is few_query_attention's core; shapes, masks, `splits` and determinism as there.  All three
    outputs and every input are differentiable."""
    same = _same_rows(x, y)
    if q.dim() != 3 or wk.dim() != 2 or wk.shape[0] != q.shape[-1] or wv.shape[0] != q.shape[-1]:
        raise ValueError(f"coattn_few_query: need q [B, L, E], Wk [E, Ek], Wv [E, Ev], got {tuple(q.shape)}, {tuple(wk.shape)}, {tuple(wv.shape)}")
    B, L, _ = q.shape
    _fewq_check(torch.empty(B, L, wk.shape[1], device="meta"), torch.empty(B, L, device="meta"), x, x if same else y)
    if wv.shape[1] != (x if same else y).shape[-1]:
        raise ValueError(f"coattn_few_query: Wv {tuple(wv.shape)} does not take values of width {(x if same else y).shape[-1]}")
    mask = None
    if key_padding_mask is not None:
        mask = key_padding_mask.to(torch.bool).contiguous().view(torch.uint8)
        if tuple(mask.shape) != (x.shape[0], x.shape[1]):
            raise ValueError(f"coattn_few_query: key_padding_mask must be [B, S] = {(x.shape[0], x.shape[1])}, got {tuple(mask.shape)}")
    return _CoattnFewQuery.apply(q, x, None if same else y, wq, bq, wk, bk, wv, bv, wo, bo, mask, splits, scaling)


# ------------------------------------------------------------------------------------------------
# few-key co-attention (the same module with a bag of queries over S <= 8 keys: CMTA's P_in_G_Att; csrc/fewk_attn.hip), the dual fold: with
# k^ = key Wk^T + bk and v^ = value Wv^T + bv, raw = x_l . u_j + c_j for u = s k^ Wq, c = s k^ . bq and the output is sum_j softmax(raw) w_j
# for w = v^ Wo^T + bo (bo folds in: the weights of a row sum to one) - the query and out projections become [B S, E]-sized products and the
# bag streams once through few_key_attention.  The launches take their arguments by the header's parameter names (capi.call); the key sets:
# ------------------------------------------------------------------------------------------------
FEWK_MAX_S, FEWK_MAX_E = 8, 512
_FEWK = "x u w B L S Eq Eo x_batch_stride x_row_stride splits stream workspace workspace_bytes "
FEWK_FWD_KEYS = frozenset((_FEWK + "c key_padding_mask out raw").split())
FEWK_BWD_KEYS = frozenset((_FEWK + "raw dout draw dx du dc dw dout_batch_stride dout_row_stride dx_batch_stride dx_row_stride").split())


def _fewk_width_ok(E: int) -> bool:
    return 0 < E <= FEWK_MAX_E and E % 64 == 0


def coattn_few_key_why(*, S: int, heads: int, Eq: int, attn_mask: bool = False, add_bias_kv: bool = False, add_zero_attn: bool = False,
                       dropout_active: bool = False, fused: bool = True) -> Optional[str]:
    """Why a MultiheadAttention call with S keys, `heads` heads and embedding width Eq (the width of the queries and of the output) stays
    on the composed path (two bag-sized projections, matmul4, softmax_rows, matmul4); None: it takes the few-key kernels.  Same contract
    as coattn_why, which is asked first: no GPU work."""
    if not fused:
        return "fused_few_key is off (the default)"
    if heads != 1:
        return f"{heads} heads (the few-key kernels are one-head)"
    if not 1 <= S <= FEWK_MAX_S:
        return f"{S} keys (at most {FEWK_MAX_S})"
    if attn_mask:
        return "an attn_mask (only key_padding_mask is fused)"
    if add_bias_kv:
        return "add_bias_kv (a learned key / value row outside the key set)"
    if add_zero_attn:
        return "add_zero_attn (a zero key / value row outside the key set)"
    if dropout_active:
        return "active attention dropout"
    if not _fewk_width_ok(Eq):
        return f"embedding width {Eq} (a multiple of 64 up to {FEWK_MAX_E})"
    return None


def _fewk_check(x, u, c, w):
    """Shapes the few-key kernels are built for (include/smml.h); raises ValueError before anything is launched."""
    if x.dim() != 3 or u.dim() != 3 or w.dim() != 3 or c.dim() != 2:
        raise ValueError(f"few_key_attention: need x [B, L, Eq], u [B, S, Eq], c [B, S], w [B, S, Eo], got {tuple(x.shape)}, {tuple(u.shape)}, "
                         f"{tuple(c.shape)}, {tuple(w.shape)}")
    B, L, Eq = x.shape
    S, Eo = u.shape[1], w.shape[2]
    if tuple(u.shape) != (B, S, Eq) or tuple(c.shape) != (B, S) or tuple(w.shape[:2]) != (B, S):
        raise ValueError(f"few_key_attention: x {tuple(x.shape)}, u {tuple(u.shape)}, c {tuple(c.shape)} and w {tuple(w.shape)} do not "
                         "describe one problem")
    if B < 1 or L < 1:
        raise ValueError(f"few_key_attention: empty bag ({tuple(x.shape)})")
    if not 1 <= S <= FEWK_MAX_S:
        raise ValueError(f"few_key_attention: between 1 and {FEWK_MAX_S} keys, got {S}")
    if not _fewk_width_ok(Eq) or not _fewk_width_ok(Eo):
        raise ValueError(f"few_key_attention: the query and output widths must be multiples of 64 up to {FEWK_MAX_E}, got {Eq} and {Eo}")
    return B, L, S, Eq, Eo


def _fewk_mask(name: str, key_padding_mask, B: int, S: int):
    if key_padding_mask is None:
        return None
    mask = key_padding_mask.to(torch.bool).contiguous().view(torch.uint8)
    if tuple(mask.shape) != (B, S):
        raise ValueError(f"{name}: key_padding_mask must be [B, S] = {(B, S)}, got {tuple(mask.shape)}")
    return mask


def _fewk_fwd(x, u, c, w, mask, splits: int):
    """One launch of the forward core on checked operands (u, c, w dense; x as _rows leaves it) -> (out [B, L, Eo], raw [B, L, S])"""
    B, L, Eq = x.shape
    S, Eo = u.shape[1], w.shape[2]
    out = torch.empty(B, L, Eo, device=x.device, dtype=torch.float32)
    raw = torch.empty(B, L, S, device=x.device, dtype=torch.float32)
    ns = dict(x=_rows_ptr(x), u=u, c=c, w=w, key_padding_mask=mask, out=out, raw=raw, workspace=None, workspace_bytes=0, B=B, L=L, S=S,
              Eq=Eq, Eo=Eo, x_batch_stride=_bs(x), x_row_stride=x.stride(1), splits=splits, stream=capi.stream())
    capi.check(capi.call("smml_fewk_attn_fwd_f32", ns, FEWK_FWD_KEYS), "fewk_attn_fwd")
    return out, raw


def _fewk_bwd(x, u, w, raw, dout, draw, want_dx: bool, splits: int):
    """One launch of the backward core -> (dx or None, du, dc, dw); dout / draw may be None (no gradient arrived for that output)."""
    B, L, Eq = x.shape
    S, Eo = u.shape[1], w.shape[2]
    dout = _rows(dout) if dout is not None else torch.zeros(B, L, Eo, device=x.device, dtype=torch.float32)
    draw = _c(draw) if draw is not None else None
    dx = _grad_rows(x) if want_dx else None
    du, dw = torch.empty_like(u), torch.empty_like(w)
    dc = torch.empty(B, S, device=x.device, dtype=torch.float32)
    dims = dict(B=B, L=L, S=S, Eq=Eq, Eo=Eo, splits=splits)
    wsb = capi.call("smml_fewk_attn_bwd_workspace_bytes", dims)
    ws = _scratch(wsb, x.device)
    ns = dict(dims, x=_rows_ptr(x), u=u, w=w, raw=raw, dout=_rows_ptr(dout), draw=draw, dx=_rows_ptr(dx), du=du, dc=dc, dw=dw, workspace=ws,
              workspace_bytes=wsb, x_batch_stride=_bs(x), x_row_stride=x.stride(1), dout_batch_stride=_bs(dout), dout_row_stride=dout.stride(1),
              dx_batch_stride=_bs(dx) if want_dx else 0, dx_row_stride=dx.stride(1) if want_dx else 0, stream=capi.stream())
    capi.check(capi.call("smml_fewk_attn_bwd_f32", ns, FEWK_BWD_KEYS), "fewk_attn_bwd")
    return dx, du, dc, dw


class _FewKeyAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, u, c, w, mask, splits):
        _fewk_check(x, u, c, w)
        ctx.set_materialize_grads(False)
        x = _rows(x); u = _c(u); c = _c(c); w = _c(w)
        ctx.splits = int(splits or 0)
        out, raw = _fewk_fwd(x, u, c, w, mask, ctx.splits)
        ctx.save_for_backward(x, u, w, raw)
        return out, raw

    @staticmethod
    def backward(ctx, dout, draw):
        x, u, w, raw = ctx.saved_tensors
        dx, du, dc, dw = _fewk_bwd(x, u, w, raw, dout, draw, ctx.needs_input_grad[0], ctx.splits)
        return dx, du, dc, dw, None, None


def few_key_attention(x, u, c, w, *, key_padding_mask=None, splits=None):
    """(out [B, L, Eo], raw [B, L, S]) with raw[b, l, j] = x[b, l] . u[b, j] + c[b, j] and out = sum_j softmax_j(raw) w[b, j], for a bag of
    rows x [B, L, Eq] over S <= 8 keys u [B, S, Eq], c [B, S] with output rows w [B, S, Eo] - one streaming pass over the bag: every row of x
    is read once, every row of out written once.  Eq and Eo multiples of 64 up to 512, any L >= 1; other shapes raise ValueError before
    anything is launched.  x is read in place when its columns are contiguous (a slice of a longer bag, the transpose of a sequence-first
    tensor).
    key_padding_mask [B, S] bool: masked keys get raw = -inf, weight 0 and zero gradient rows du, dc, dw; a bag with every key masked gives
    NaN, as the reference does (not checked: that would be a host sync).
    Both outputs are differentiable; u, c and w receive gradients, x only where it requires one (no buffer is written otherwise), in x's
    own layout where that is dense.
    splits: how many pieces a bag's rows are cut into (None: chosen by the library so that B x splits fills the chip); the gradients are
    a function of the inputs and this number alone, the outputs of the inputs alone - the same under functional.deterministic().
    Several heads would fold as h S virtual keys with a softmax per group of S; only one head is built."""
    B, _, S, _, _ = _fewk_check(x, u, c, w)
    return _FewKeyAttention.apply(x, u, c, w, _fewk_mask("few_key_attention", key_padding_mask, B, S), splits)


class _CoattnFewKey(torch.autograd.Function):
    """The whole folded co-attention as ONE autograd node, as _CoattnFewQuery is for the dual problem: the [B S, E]-sized products around
    the core are the same smml_gemm launches (k^ = k Wk^T + bk; u = s k^ Wq, c = s k^ . bq with the scaling s as the products' alpha;
    v^ = v Wv^T + bv; w = v^ Wo^T + bo) and their gradients are formed as _Linear.backward forms them.  v = None: the values are the keys
    (one tensor, one gradient dk + dv)."""

    @staticmethod
    def forward(ctx, q, k, v, wq, bq, wk, bk, wv, bv, wo, bo, mask, splits, scaling):
        B, S, _ = k.shape
        ctx.set_materialize_grads(False)
        ctx.det = DETERMINISTIC
        ctx.splits, ctx.scaling, ctx.same = int(splits or 0), float(scaling), v is None
        ctx.shapes = tuple(None if b is None else b.shape for b in (bq, bk, bv, bo))
        k2 = _c(k).reshape(B * S, -1)
        v2 = k2 if v is None else _c(v).reshape(B * S, -1)
        wq, wk, wv, wo = _c(wq), _c(wk), _c(wv), _c(wo)
        bqc, bkc, bvc, boc = (None if b is None else _c(b).reshape(-1) for b in (bq, bk, bv, bo))
        E = wq.shape[0]
        x = _rows(q)
        kh = _lin(k2, wk, bkc)
        u = _mat(kh, wq, alpha=ctx.scaling).view(B, S, -1)
        c = _lin(kh, bqc.view(1, E), alpha=ctx.scaling).view(B, S) if bqc is not None else torch.zeros(B, S, device=q.device)
        vh = _lin(v2, wv, bvc)
        w = _lin(vh, wo, boc).view(B, S, -1)
        out, raw = _fewk_fwd(x, u, c, w, mask, ctx.splits)
        ctx.save_for_backward(x, k2, None if ctx.same else v2, kh, vh, u, w, raw, wq, bqc, wk, wv, wo)
        return out, raw

    @staticmethod
    def backward(ctx, dout, draw):
        x, k2, v2, kh, vh, u, w, raw, wq, bq, wk, wv, wo = ctx.saved_tensors
        B, S, _ = u.shape
        R, s, det = B * S, ctx.scaling, ctx.det
        col = lambda g, shape: None if shape is None else colsum(g.reshape(1, R, -1), det=det)[0].view(shape)      # noqa: E731
        dx, du, dc, dw = _fewk_bwd(x, u, w, raw, dout, draw, ctx.needs_input_grad[0], ctx.splits)
        du2, dc2, dw2 = du.view(R, -1), dc.view(R, 1), dw.view(R, -1)
        dvh = _mat(dw2, wo)
        dwo, dbo = _wgrad(dw2, vh, det), col(dw2, ctx.shapes[3])
        dwv, dbv = _wgrad(dvh, k2 if ctx.same else v2, det), col(dvh, ctx.shapes[2])
        dkh = _lin(du2, wq, alpha=s)                                        # s du Wq^T ...
        dwq = _wgrad(kh, du2, det, alpha=s)
        dbq = None
        if bq is not None:
            dkh.addcmul_(dc2, bq.view(1, -1), value=s)                      # ... + s dc bq^T, [B S, E]-sized
            dbq = _wgrad(kh, dc2, det, alpha=s).view(ctx.shapes[0])
        dwk, dbk = _wgrad(dkh, k2, det), col(dkh, ctx.shapes[1])
        need_k, need_v = ctx.needs_input_grad[1], ctx.needs_input_grad[2] and not ctx.same
        dk = _mat(dkh, wk).view(B, S, -1) if need_k else None
        dv = _mat(dvh, wv).view(B, S, -1) if need_v or (need_k and ctx.same) else None
        if ctx.same and need_k:
            dk, dv = dk.add_(dv), None                                      # one tensor: its gradient is dk + dv
        return dx, dk, dv, dwq, dbq, dwk, dbk, dwv, dbv, dwo, dbo, None, None, None


def coattn_few_key(q, k, v, wq, bq, wk, bk, wv, bv, wo, bo, *, scaling: float, key_padding_mask=None, splits=None):
    """(out [B, L, E], raw [B, L, S]) of one-head co-attention in the few-key folded form, batch first: q [B, L, E] a bag of queries,
    k [B, S, Ek] keys, v [B, S, Ev] values (None, k itself or another view of k's base over the same memory: the values are the keys),
    Wq [E, E], Wk [E, Ek], Wv [E, Ev], Wo [Eo, E] and their biases (any may be None).  The bag-sized work is few_key_attention's core; shapes,
    masks, `splits` and determinism as there.  Both outputs and every input are differentiable; q receives a gradient only where it
    requires one."""
    same = _same_rows(k, v)
    if q.dim() != 3 or k.dim() != 3 or wq.dim() != 2 or wo.dim() != 2 or wq.shape[1] != q.shape[-1] or wk.shape[0] != wq.shape[0] or \
            wv.shape[0] != wo.shape[1] or wk.shape[1] != k.shape[-1]:
        raise ValueError(f"coattn_few_key: need q [B, L, E], k [B, S, Ek], Wq [E, E], Wk [E, Ek], Wv [E, Ev], Wo [Eo, E], got {tuple(q.shape)}, "
                         f"{tuple(k.shape)}, {tuple(wq.shape)}, {tuple(wk.shape)}, {tuple(wv.shape)}, {tuple(wo.shape)}")
    B, S = k.shape[:2]
    vv = k if same else v
    if tuple(vv.shape[:2]) != (B, S) or wv.shape[1] != vv.shape[-1]:
        raise ValueError(f"coattn_few_key: Wv {tuple(wv.shape)} and the keys {tuple(k.shape)} do not take values of shape {tuple(vv.shape)}")
    _fewk_check(q, torch.empty(B, S, q.shape[-1], device="meta"), torch.empty(B, S, device="meta"), torch.empty(B, S, wo.shape[0], device="meta"))
    mask = _fewk_mask("coattn_few_key", key_padding_mask, B, S)
    return _CoattnFewKey.apply(q, k, None if same else v, wq, bq, wk, bk, wv, bv, wo, bo, mask, splits, scaling)


# ------------------------------------------------------------------------------------------------
# sets of at most 8 tokens (MCAT_Surv after its co-attention, models/model.py:589-651; csrc/token_set.hip): multi-head self-attention from
# the packed projection and gated attention pooling WITH the gradient of the pooled rows - one launch per direction each, no workspace,
# no float atomics.  The launches take their arguments by the header's parameter names (capi.call); the key sets:
# ------------------------------------------------------------------------------------------------
TOKEN_MAX_T, TOKEN_MAX_E, TOKEN_MAX_D = 8, 512, 256
TOKEN_HEAD_DIMS = (32, 64)
_TOKEN_ATTN = "qkv keep B T E H qkv_batch_stride qkv_token_stride scale stream "
_TOKEN_POOL = "x h2 w B T E D x_batch_stride x_token_stride stream "
TOKEN_ATTN_FWD_KEYS = frozenset((_TOKEN_ATTN + "o p o_batch_stride o_token_stride").split())
TOKEN_ATTN_BWD_KEYS = frozenset((_TOKEN_ATTN + "p dout dqkv dout_batch_stride dout_token_stride dqkv_batch_stride dqkv_token_stride").split())
TOKEN_POOL_FWD_KEYS = frozenset((_TOKEN_POOL + "b s a out").split())
TOKEN_POOL_BWD_KEYS = frozenset((_TOKEN_POOL + "a dout dx dh2 dw db dx_batch_stride dx_token_stride").split())


def token_why(*, T: int, E: int, heads: Optional[int] = None, D: Optional[int] = None, attn_mask: bool = False,
              key_padding_mask: bool = False, fused: bool = True) -> Optional[str]:
    """Why an operation on a set of T tokens of width E stays on its composed form; None: it takes the token-set kernels.  heads: the
    call is a self-attention with that many heads (composed: coattention.MultiheadAttention - projections, permutes, matmul4,
    softmax_rows, matmul4).  D: the call is a gated pooling with D hidden units per gate (composed: softmax_rows and matmul4 after the
    head's three layers).  No GPU work."""
    if not fused:
        return "the fused token-set path is switched off"
    if not 1 <= T <= TOKEN_MAX_T:
        return f"{T} tokens (at most {TOKEN_MAX_T})"
    if E % 64 or not 0 < E <= TOKEN_MAX_E:
        return f"token width {E} (a multiple of 64 up to {TOKEN_MAX_E})"
    if heads is not None:
        if heads < 1 or E % heads or E // heads not in TOKEN_HEAD_DIMS:
            return f"head dim {E}/{heads} (the kernels are built for {' and '.join(map(str, TOKEN_HEAD_DIMS))})"
        if attn_mask:
            return "an attention mask (the token kernels take none)"
        if key_padding_mask:
            return "a key padding mask (the token kernels take none)"
    if D is not None and (D % 64 or not 0 < D <= TOKEN_MAX_D):
        return f"{D} hidden units per gate (a multiple of 64 up to {TOKEN_MAX_D})"
    return None


def token_path(**kw) -> str:
    """'token' (csrc/token_set.hip) or 'composed': the arguments of token_why, which names the reason for 'composed'."""
    return "composed" if token_why(**kw) is not None else "token"


def _like_rows(t: torch.Tensor, width: int) -> torch.Tensor:
    """An uninitialised [B, T, width] buffer in the layout of the rows t [B, T, .]: sequence-first memory where t's is (what follows reads
    it sequence-first without a copy), batch-first otherwise."""
    B, T = t.shape[:2]
    if t.transpose(0, 1).is_contiguous():
        return torch.empty(T, B, width, device=t.device, dtype=torch.float32).transpose(0, 1)
    return torch.empty(B, T, width, device=t.device, dtype=torch.float32)


def _token_attn_check(qkv, heads: int, keep):
    """Shapes the token self-attention kernels are built for (include/smml.h); raises ValueError before anything is launched."""
    if qkv.dim() != 3 or qkv.shape[-1] % 3:
        raise ValueError(f"token_self_attention: need the packed projection qkv [B, T, 3 E], got {tuple(qkv.shape)}")
    B, T, E = qkv.shape[0], qkv.shape[1], qkv.shape[2] // 3
    if B < 1:
        raise ValueError(f"token_self_attention: empty batch ({tuple(qkv.shape)})")
    why = token_why(T=T, E=E, heads=int(heads))
    if why is not None:
        raise ValueError(f"token_self_attention: {why}")
    if keep is not None and tuple(keep.shape) != (B, heads, T, T):
        raise ValueError(f"token_self_attention: keep must be [B, H, T, T] = {(B, heads, T, T)}, got {tuple(keep.shape)}")
    return B, T, E


class _TokenSelfAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, keep, heads, scale):
        B, T, E = _token_attn_check(qkv, heads, keep)
        qkv = _rows(qkv)
        keep = _c(keep) if keep is not None else None
        o = _like_rows(qkv, E)
        p = torch.empty(B, heads, T, T, device=qkv.device, dtype=torch.float32)
        ctx.dims = dict(B=B, T=T, E=E, H=int(heads), scale=float(scale))
        ns = dict(ctx.dims, qkv=_rows_ptr(qkv), keep=keep, o=_rows_ptr(o), p=p, qkv_batch_stride=_bs(qkv), qkv_token_stride=qkv.stride(1),
                  o_batch_stride=_bs(o), o_token_stride=o.stride(1), stream=capi.stream())
        capi.check(capi.call("smml_token_attn_fwd_f32", ns, TOKEN_ATTN_FWD_KEYS), "token_attn_fwd")
        ctx.save_for_backward(qkv, keep, p)
        ctx.mark_non_differentiable(p)
        return o, p

    @staticmethod
    def backward(ctx, dout, _dp):
        qkv, keep, p = ctx.saved_tensors
        dout = _rows(dout)
        dqkv = _grad_rows(qkv)
        ns = dict(ctx.dims, qkv=_rows_ptr(qkv), keep=keep, p=p, dout=_rows_ptr(dout), dqkv=_rows_ptr(dqkv), qkv_batch_stride=_bs(qkv),
                  qkv_token_stride=qkv.stride(1), dout_batch_stride=_bs(dout), dout_token_stride=dout.stride(1),
                  dqkv_batch_stride=_bs(dqkv), dqkv_token_stride=dqkv.stride(1), stream=capi.stream())
        capi.check(capi.call("smml_token_attn_bwd_f32", ns, TOKEN_ATTN_BWD_KEYS), "token_attn_bwd")
        return dqkv, None, None, None


def token_self_attention(qkv, *, heads: int, scale: Optional[float] = None, keep=None, probs_out=None):
    """o [B, T, E] = (softmax_rows(scale Q K^T) keep) V per head, heads merged, for a set of T <= 8 tokens from its packed projection
    qkv [B, T, 3 E] = [q | k | v] (head h reads columns [h hd, (h + 1) hd) of each third, hd = E / heads in {32, 64}; E a multiple of 64 up to
    512; other shapes raise ValueError before anything is launched).  qkv is read in place when its columns are contiguous: pass the
    sequence-first output [T, B, 3 E] of `linear` as its transpose(0, 1); o then comes back in the same memory order, and so does the
    gradient of qkv.  scale: default hd ** -0.5.  keep [B, H, T, T]: the multipliers of attention dropout, 0 or 1 / (1 - rate), drawn by
    the caller (no gradient); a row of zeros gives a zero output row.  probs_out: a list that receives [p], the softmax [B, H, T, T] before
    keep.  One launch per direction, identical bits run after run."""
    _token_attn_check(qkv, heads, keep)
    if scale is None:
        scale = float(qkv.shape[-1] // 3 // heads) ** -0.5
    o, p = _TokenSelfAttention.apply(qkv, keep, int(heads), float(scale))
    if probs_out is not None:
        probs_out[:] = [p]
    return o


def _token_pool_check(x, h2, w, b):
    """Shapes the token pooling kernels are built for (include/smml.h); raises ValueError before anything is launched."""
    if x.dim() != 3 or h2.dim() != 3 or tuple(h2.shape[:2]) != tuple(x.shape[:2]) or h2.shape[-1] % 2:
        raise ValueError(f"token_pool_gated: need x [B, T, E] and h2 [B, T, 2 D] over the same tokens, got {tuple(x.shape)} and {tuple(h2.shape)}")
    B, T, E = x.shape
    D = h2.shape[-1] // 2
    if B < 1:
        raise ValueError(f"token_pool_gated: empty batch ({tuple(x.shape)})")
    why = token_why(T=T, E=E, D=D)
    if why is not None:
        raise ValueError(f"token_pool_gated: {why}")
    if w.numel() != D or b.numel() != 1:
        raise ValueError(f"token_pool_gated: one attention map - w must hold D = {D} values and b one, got {tuple(w.shape)} and {tuple(b.shape)}")
    return B, T, E, D


class _TokenPoolGated(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, h2, w, b, scores_out):
        B, T, E, D = _token_pool_check(x, h2, w, b)
        ctx.w_shape, ctx.b_shape = w.shape, b.shape
        x = _rows(x); h2 = _c(h2); w = _c(w).reshape(D); b = _c(b).reshape(1)
        s = torch.empty(B, T, device=x.device, dtype=torch.float32)
        a = torch.empty(B, T, device=x.device, dtype=torch.float32)
        M = torch.empty(B, E, device=x.device, dtype=torch.float32)
        ctx.dims = dict(B=B, T=T, E=E, D=D)
        ns = dict(ctx.dims, x=_rows_ptr(x), h2=h2, w=w, b=b, s=s, a=a, out=M, x_batch_stride=_bs(x), x_token_stride=x.stride(1),
                  stream=capi.stream())
        capi.check(capi.call("smml_token_pool_gated_fwd_f32", ns, TOKEN_POOL_FWD_KEYS), "token_pool_gated_fwd")
        if scores_out is not None:
            scores_out[:] = [s, a]
        ctx.save_for_backward(x, h2, w, a)
        return M

    @staticmethod
    def backward(ctx, dM):
        x, h2, w, a = ctx.saved_tensors
        dM = _c(dM)
        dx = _grad_rows(x)
        dh2 = torch.empty_like(h2)
        dw = torch.empty(ctx.dims["D"], device=x.device, dtype=torch.float32)
        db = torch.empty(1, device=x.device, dtype=torch.float32)
        ns = dict(ctx.dims, x=_rows_ptr(x), h2=h2, w=w, a=a, dout=dM, dx=_rows_ptr(dx), dh2=dh2, dw=dw, db=db, x_batch_stride=_bs(x),
                  x_token_stride=x.stride(1), dx_batch_stride=_bs(dx), dx_token_stride=dx.stride(1), stream=capi.stream())
        capi.check(capi.call("smml_token_pool_gated_bwd_f32", ns, TOKEN_POOL_BWD_KEYS), "token_pool_gated_bwd")
        return dx, dh2, dw.view(ctx.w_shape), db.view(ctx.b_shape), None


def token_pool_gated(x, h2, w, b, *, scores_out=None):
    """M [B, E] = sum_t softmax_t(sum_d w_d hv[b, t, d] hu[b, t, d] + b) x[b, t, :] for a set of T <= 8 tokens x [B, T, E] and its two gates in
    ONE tensor h2 [B, T, 2 D] (hv = h2[..., :D], the tanh units; hu = h2[..., D:], the sigmoid units: the output of
    linear(..., act=ACT_TANH_SIGMOID) with the stacked weight); one attention map: w holds D values, b one.  E a multiple of 64 up to 512,
    D a multiple of 64 up to 256; other shapes raise ValueError before anything is launched.  x is read in place when its columns are
    contiguous (the transpose of a sequence-first tensor).  Unlike attention_pool_gated the pooled rows are activations: x, h2, w and b
    all receive gradients.  scores_out: a list that receives [s, a], the scores and their softmax, both [B, T].  One launch per direction;
    the sums over samples in dw and db have one owner and a fixed order: identical bits run after run."""
    _token_pool_check(x, h2, w, b)
    return _TokenPoolGated.apply(x, h2, w, b, scores_out)


# ------------------------------------------------------------------------------------------------
# self-normalising encoder stacks (SNN_Block, models/mcat_utils.py:81-95; MaxNet's encoder, models/model.py:142-187; csrc/snn_stack.hip):
# up to 8 networks of up to 4 layers Linear -> ELU -> AlphaDropout, every network of a model in ONE forward launch and TWO backward launches.
# The per-network and per-layer addresses travel as host tables (ctypes arrays, read during the call); the key sets of the two launches:
# ------------------------------------------------------------------------------------------------
SNN_MAX_NETS, SNN_MAX_DEPTH, SNN_MAX_WIDTH, SNN_MAX_INPUTS = 8, 4, 256, 2048
SNN_ALPHA = 1.7580993408473766          # torch's AlphaDropout: selu's scale times its alpha
_SNN = "x x_row_stride x_col_offset W widths keep acts out G depth B p final_relu stream "
SNN_FWD_KEYS = frozenset((_SNN + "b").split())
SNN_BWD_KEYS = frozenset((_SNN + "dout dz dW db dx").split())


def _flat(v) -> list:
    """the leaves of nested lists / tuples, in order"""
    out = []
    for u in v:
        if isinstance(u, (list, tuple)):
            out += _flat(u)
        else:
            out.append(u)
    return out


def snn_why(widths, *, rates=None, dtypes=None) -> Optional[str]:
    """Why a group of SNN encoders stays on its composed form (linear, ELU and AlphaDropout per layer); None: it takes the fused kernels.
    widths: one list [K_0, N_1, .., N_depth] per network.  rates: the AlphaDropout rates in force, any nesting (one rate serves the launch).
    dtypes: the parameters' dtypes.  No GPU work."""
    if not 1 <= len(widths) <= SNN_MAX_NETS:
        return f"{len(widths)} networks (1 to {SNN_MAX_NETS})"
    depth = len(widths[0]) - 1
    if any(len(w) - 1 != depth for w in widths):
        return f"unequal depths {[len(w) - 1 for w in widths]} (every network of a call has the same number of layers)"
    if not 1 <= depth <= SNN_MAX_DEPTH:
        return f"depth {depth} (1 to {SNN_MAX_DEPTH} layers)"
    for g, w in enumerate(widths):
        if not 1 <= w[0] <= SNN_MAX_INPUTS:
            return f"{w[0]} inputs of network {g} (1 to {SNN_MAX_INPUTS})"
        if not 1 <= min(w) <= max(w[1:]) <= SNN_MAX_WIDTH:
            l = next(i for i, n in enumerate(w[1:]) if not 1 <= n <= SNN_MAX_WIDTH)
            return f"width {w[l + 1]} of layer {l} of network {g} (1 to {SNN_MAX_WIDTH})"
    if rates is not None:
        rs = sorted({float(r) for r in _flat(rates)})
        if len(rs) > 1:
            return f"unequal dropout rates {rs} (one rate serves the launch)"
        if rs and not 0.0 <= rs[0] < 1.0:
            return f"dropout rate {rs[0]} (0 <= p < 1)"
    if dtypes is not None:
        other = sorted({str(d) for d in _flat(dtypes) if d != torch.float32})
        if other:
            return f"parameters of dtype {other} (the kernels are fp32)"
    return None


def snn_path(widths, **kw) -> str:
    """'snn' (csrc/snn_stack.hip) or 'composed': the arguments of snn_why, which names the reason for 'composed'."""
    return "composed" if snn_why(widths, **kw) is not None else "snn"


def snn_keep_numel(B: int, widths) -> int:
    """Length of the flat `keep` of snn_stack - the layout of the saved activations: dense [B, N_l] blocks in the order network 0 .. G - 1,
    within a network layer 1 .. depth."""
    return int(B) * sum(int(n) for w in widths for n in list(w)[1:])


def snn_draw_keep(B: int, widths, p: float, device) -> torch.Tensor:
    """The 0 / 1 multipliers of every layer of every network in ONE draw (bernoulli_ on one flat tensor, reproducible under
    torch.manual_seed)."""
    return torch.empty(snn_keep_numel(B, widths), device=device, dtype=torch.float32).bernoulli_(1.0 - float(p))


def _snn_check(xs, weights, biases, p, keep):
    """(G, depth, B, widths) of a call the kernels take; raises ValueError, naming the quantity, before anything is launched."""
    if not (isinstance(xs, (list, tuple)) and isinstance(weights, (list, tuple)) and isinstance(biases, (list, tuple))) or \
            not len(xs) == len(weights) == len(biases) or any(len(w) != len(b) for w, b in zip(weights, biases)):
        raise ValueError("snn_stack: need one input, one list of weights and one list of biases per network")
    widths = []
    for g, (x, ws, bs) in enumerate(zip(xs, weights, biases)):
        if x.dim() != 2 or any(w.dim() != 2 for w in ws) or not ws:
            raise ValueError(f"snn_stack: network {g} needs x [B, K] and weights [N, K]")
        w = [int(x.shape[1])]
        for l, (W, b) in enumerate(zip(ws, bs)):
            if W.shape[1] != w[-1] or b.numel() != W.shape[0]:
                raise ValueError(f"snn_stack: layer {l} of network {g}: weight {tuple(W.shape)} and bias {tuple(b.shape)} do not follow {w[-1]} columns")
            w.append(int(W.shape[0]))
        widths.append(w)
    why = snn_why(widths, rates=(p,), dtypes=[t.dtype for ts in (*weights, *biases) for t in ts])
    if why is not None:
        raise ValueError(f"snn_stack: {why}")
    B = int(xs[0].shape[0])
    if B < 1 or any(int(x.shape[0]) != B for x in xs):
        raise ValueError(f"snn_stack: every network takes the same B >= 1 rows, got {[tuple(x.shape) for x in xs]}")
    if (p > 0) != (keep is not None):
        raise ValueError("snn_stack: keep is required with p > 0 and must be None with p = 0")
    if keep is not None and keep.numel() != snn_keep_numel(B, widths):
        raise ValueError(f"snn_stack: keep must hold {snn_keep_numel(B, widths)} values (snn_keep_numel), got {tuple(keep.shape)}")
    return len(xs), len(weights[0]), B, widths


def _snn_addrs(tensors, device):
    """The host table of the device addresses of contiguous fp32 tensors on `device` (0 for None): the checks of capi.fptr, the device
    looked up once by the caller"""
    for t in tensors:
        if t is not None and not (t.device == device and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError(f"smml fp32 kernels need contiguous fp32 tensors on {device}, got {t.dtype} on {t.device}, strides {t.stride()}")
    return (C_.c_ulonglong * len(tensors))(*[0 if t is None else t.data_ptr() for t in tensors])


def _snn_rows(t: torch.Tensor) -> torch.Tensor:
    """The input rows as the kernels read them: fp32 on the current device with unit column stride - a column range of a wider tensor
    stays the view it is (capi.ptr's checks without its contiguity rule)"""
    if t.dtype != torch.float32 or not (t.stride(1) == 1 or t.shape[1] == 1) or t.stride(0) < 0:
        t = _c(t)
    if not t.is_cuda or t.device.index != torch.cuda.current_device():
        raise RuntimeError(f"smml kernels need tensors resident in the HBM of the current device, got one on {t.device}; this path has no CPU fallback")
    return t


class _SnnStack(torch.autograd.Function):
    """tensors: the G inputs, then the G depth weights, then the G depth biases (network-major)"""

    @staticmethod
    def forward(ctx, keep, p, final_relu, stacked, widths, *tensors):
        ctx.set_materialize_grads(False)
        G, depth = len(widths), len(widths[0]) - 1
        xs = [_snn_rows(t) for t in tensors[:G]]
        Ws = [_c(t) for t in tensors[G:G + G * depth]]
        bs = [_c(t) for t in tensors[G + G * depth:]]
        B, dev = xs[0].shape[0], xs[0].device
        keep = _c(keep).reshape(-1) if keep is not None else None
        acts = torch.empty(snn_keep_numel(B, widths), device=dev, dtype=torch.float32)
        last = [w[-1] for w in widths]
        if min(last) == max(last):
            buf = torch.empty(G, B, last[0], device=dev, dtype=torch.float32)
            outs = [t.detach() for t in buf.unbind(0)]
        else:
            buf, outs = None, [torch.empty(B, n, device=dev, dtype=torch.float32) for n in last]
        L = C_.c_longlong * G
        offs = [x.storage_offset() for x in xs]
        ctx.tables = dict(x=(C_.c_ulonglong * G)(*[x.data_ptr() - 4 * o for x, o in zip(xs, offs)]), x_row_stride=L(*[x.stride(0) for x in xs]),
                          x_col_offset=L(*offs), W=_snn_addrs(Ws, dev), widths=(C_.c_int * (G * (depth + 1)))(*[n for w in widths for n in w]),
                          out=_snn_addrs(outs, dev), G=G, depth=depth, B=B, p=p, final_relu=int(final_relu))
        ns = dict(ctx.tables, b=_snn_addrs(bs, dev), keep=keep, acts=acts, stream=capi.stream())
        capi.check(capi.call("smml_snn_stack_fwd_f32", ns, SNN_FWD_KEYS), "snn_stack_fwd")
        ctx.save_for_backward(keep, acts, *xs, *Ws, *outs)
        ctx.dims = (G, depth, stacked)
        ctx.bias_shapes = [t.shape for t in tensors[G + G * depth:]]
        return buf if stacked else tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        G, depth, stacked = ctx.dims
        keep, acts, *rest = ctx.saved_tensors
        xs, Ws = rest[:G], rest[G:G + G * depth]
        if stacked:                                                              # one gradient [G, B, N]: its slices
            douts = _c(douts[0]).unbind(0) if douts[0] is not None else [None] * G
        douts = [_c(d) if d is not None else None for d in douts]
        dev = acts.device
        dz = torch.empty_like(acts)
        dW = [torch.empty_like(w) for w in Ws]                                  # one allocation per parameter: autograd adopts them as they are
        db = [torch.empty(w.shape[0], device=dev, dtype=torch.float32) for w in Ws]
        dx = [torch.empty(x.shape, device=dev, dtype=torch.float32) if ctx.needs_input_grad[5 + g] else None for g, x in enumerate(xs)]
        ns = dict(ctx.tables, keep=keep, acts=acts, dz=dz, dout=_snn_addrs(douts, dev), dW=_snn_addrs(dW, dev), db=_snn_addrs(db, dev),
                  dx=_snn_addrs(dx, dev), stream=capi.stream())
        capi.check(capi.call("smml_snn_stack_bwd_f32", ns, SNN_BWD_KEYS), "snn_stack_bwd")
        return (None,) * 5 + tuple(dx) + tuple(dW) + tuple(t.view(s) for t, s in zip(db, ctx.bias_shapes))


def snn_stack(xs, weights, biases, *, p: float = 0.0, keep=None, final_relu: bool = False, stacked: bool = False):
    """G independent self-normalising encoders in one launch per direction (two backward): network g runs x_g [B, K_0] through its layers
        e_l = ELU(a_{l-1} W_l^T + b_l)      a_l = e_l   or, with p > 0,   A keep e_l + A alpha' (keep - 1) + A alpha' p
    (torch's AlphaDropout for the given 0 / 1 tensor, alpha' = SNN_ALPHA, A = ((alpha'^2 p + 1)(1 - p))^-1/2) and returns
    max(a_depth, 0) with final_relu, a_depth otherwise: a tuple of one [B, N_g] tensor per network.
    xs: one [B, K_0] tensor per network; a column range x_all[:, a:b] of a wider tensor is read in place.  weights, biases: per network the list
    of its layers' nn.Linear parameters ([N_l, K_l] and [N_l]).  Up to 8 networks of the same depth <= 4, K_0 <= 2048, every N_l <= 256, fp32
    parameters, one rate; anything else raises ValueError, naming the quantity, before anything is launched (snn_why tells without raising).
    keep: ONE flat float tensor of 0 and 1 in the layout of the saved activations (snn_keep_numel; snn_draw_keep draws it in one call), drawn
    by the caller; required with p > 0, None otherwise.
    Where all last widths agree the returned tensors are the slices of one contiguous [G, B, N] tensor; stacked=True returns that tensor itself
    (what torch.stack of the slices would copy).  Every weight and bias receives its gradient in a buffer of its own, the inputs only where they
    require one.  No float atomics, one owner and one order per sum: identical bits run after run, with and without deterministic()."""
    p = float(p)
    G, depth, _, widths = _snn_check(xs, weights, biases, p, keep)
    if stacked and len({w[-1] for w in widths}) != 1:
        raise ValueError(f"snn_stack: stacked=True needs equal last widths, got {[w[-1] for w in widths]}")
    return _SnnStack.apply(keep, p, bool(final_relu), bool(stacked), widths, *xs, *[t for ws in weights for t in ws], *[t for bs in biases for t in bs])


# ------------------------------------------------------------------------------------------------
# bf16-storage linear (csrc/gemm_b16.hip): x bf16 [.., K], W an fp32 parameter [N, K] -> y bf16 or fp32 [.., N]
# ------------------------------------------------------------------------------------------------
def _bptr(t: torch.Tensor):
    if t.dtype != torch.bfloat16:
        raise RuntimeError(f"smml bf16 kernel got dtype {t.dtype}")
    return capi.ptr(t)


def gemm_b16(A, B, C, *, M, N, K, lda, ldb, ldc, trans=False, bias=None, splitk=1, nb=1, sa=0, sb=0, sc=0, a_off=0, b_off=0, c_off=0):
    """C = A B^T (trans False: A [M, K], B [N, K]) or A^T B (trans True: A [K, M], B [K, N]); A, B bf16, C bf16 or fp32.  nb problems at
    element strides sa / sb / sc (sc = 0: they add up in one zeroed fp32 output); *_off: element offsets of the first problem."""
    if C.dtype not in (torch.bfloat16, torch.float32):
        raise RuntimeError(f"gemm_b16: output dtype {C.dtype}")
    _bptr(A), _bptr(B), capi.ptr(C)                            # device / contiguity checks
    pa = C_.c_void_p(A.data_ptr() + 2 * a_off)
    pb = C_.c_void_p(B.data_ptr() + 2 * b_off)
    pc = C_.c_void_p(C.data_ptr() + C.element_size() * c_off)
    capi.check(capi.lib().smml_gemm_b16_batched(pa, pb, pc, capi.fptr(bias), M, N, K, lda, ldb, ldc, int(trans),
                                                int(C.dtype == torch.bfloat16), splitk, nb, sa, sb, sc, capi.stream()), "gemm_b16")


class _LinearB16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, out_bf16, skip):
        if x.dtype != torch.bfloat16:
            raise RuntimeError("linear_b16: x must be bf16 (the caller casts once)")
        ctx.det = DETERMINISTIC
        x = x if x.is_contiguous() else x.contiguous()
        wb = weight.detach().to(torch.bfloat16)                 # the parameter stays fp32; [N, K] bf16 is 1.5 MB at most here
        K = x.shape[-1]
        N = weight.shape[0]
        if skip:
            if x.dim() != 3 or not 0 < skip < x.shape[1]:
                raise RuntimeError("linear_b16: skip needs x [b, rows, K] with 0 < skip < rows")
            b, rows = x.shape[0], x.shape[1]
            y = torch.empty(b, rows - skip, N, device=x.device, dtype=torch.bfloat16 if out_bf16 else torch.float32)
            gemm_b16(x, wb, y, M=rows - skip, N=N, K=K, lda=K, ldb=K, ldc=N, bias=_c(bias) if bias is not None else None, nb=b,
                     sa=rows * K, sc=(rows - skip) * N, a_off=skip * K)
        else:
            M = x.numel() // K
            y = torch.empty(*x.shape[:-1], N, device=x.device, dtype=torch.bfloat16 if out_bf16 else torch.float32)
            gemm_b16(x, wb, y, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=_c(bias) if bias is not None else None)
        ctx.has_bias = bias is not None
        ctx.skip = skip
        ctx.save_for_backward(x, wb)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wb = ctx.saved_tensors
        K = x.shape[-1]
        N = wb.shape[0]
        skip = ctx.skip
        if ctx.det and ctx.needs_input_grad[1]:
            _no_det("linear_b16 backward (weight gradient)", "the bf16-storage GEMM adds the slices of its split reduction with float atomics "
                    "(smml_gemm_b16 / smml_gemm_b16_batched)")
        rows_y = dy.numel() // N
        db = None
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = colsum(_c(dy).reshape(1, rows_y, N), det=ctx.det)[0]
        dyb = dy if dy.dtype == torch.bfloat16 else dy.to(torch.bfloat16)
        dyb = dyb if dyb.is_contiguous() else dyb.contiguous()
        dx = dw = None
        if skip:
            b, rows = x.shape[0], x.shape[1]
            n = rows - skip
            if ctx.needs_input_grad[0]:
                wt = wb.t().contiguous()
                dx = torch.empty_like(x)
                dx[:, :skip].zero_()                                # the skipped rows took no part
                gemm_b16(dyb, wt, dx, M=n, N=K, K=N, lda=N, ldb=N, ldc=K, nb=b, sa=n * N, sc=rows * K, c_off=skip * K)
            if ctx.needs_input_grad[1]:
                dw = _ZEROS.zeros((N, K), x.device)
                gemm_b16(dyb, x, dw, M=N, N=K, K=n, lda=N, ldb=K, ldc=K, trans=True, splitk=0, nb=b,
                         sa=n * N, sb=rows * K, sc=0, b_off=skip * K)
            return dx, dw, db, None, None
        M = x.numel() // K
        if ctx.needs_input_grad[0]:
            wt = wb.t().contiguous()                            # [K, N]: dx = dy (W^T)^T is the k-contiguous form again
            dx = torch.empty_like(x)
            gemm_b16(dyb, wt, dx, M=M, N=K, K=N, lda=N, ldb=N, ldc=K)
        if ctx.needs_input_grad[1]:
            dw = _ZEROS.zeros((N, K), x.device)
            gemm_b16(dyb, x, dw, M=N, N=K, K=M, lda=N, ldb=K, ldc=K, trans=True, splitk=0)
        return dx, dw, db, None, None


def linear_b16(x, weight, bias=None, out_bf16: bool = True, skip: int = 0):
    """x W^T (+ bias) with bf16 operands in memory and fp32 accumulation; x bf16, weight / bias fp32 parameters (gradients fp32), the
    result bf16 (out_bf16) or fp32; dx is bf16.  skip > 0 (x [b, rows, K]): the first `skip` rows of every bag are left out - the result
    is [b, rows - skip, N] (the zero rows the Nystrom block pads in front of a bag never reach the output projection)."""
    return _LinearB16.apply(x, weight, bias, out_bf16, skip)


# ------------------------------------------------------------------------------------------------
# The bf16-storage pipeline of the Nystrom block (bf16 compute mode): q / k / v stay in the token-major bf16 buffer qkv [b, n, 3, h, 64]
# the projection writes; the four Functions below read them there at their strides and assemble ONE gradient buffer dqkv of the same
# layout, which the projection's backward consumes.  The buffer is threaded through the chain as an extra output of each stage
#   qkv_project16 -> attention16_keys_long -> resconv16 -> attention16_queries_long
# (each stage returns qkv itself): in backward the chain runs in reverse, the LAST stage allocates dqkv and writes dq, resconv16 writes the v
# part, attention16_keys_long writes dk and adds its dv, qkv_project16 adds the landmark means' gradients and runs the two GEMMs - no stage
# returns a full-size gradient of its own for autograd to add up (six n'-sized adds / copies per step in the fp32-storage composition).
# A stage modifies the incoming dqkv in place: it was produced by the stage after it for this purpose and nobody else holds it.
# ------------------------------------------------------------------------------------------------
def _qkv_dims(qkv, heads):
    b, n, c = qkv.shape
    if qkv.dtype != torch.bfloat16 or not qkv.is_contiguous() or c % (3 * heads):
        raise RuntimeError("qkv must be a contiguous bf16 [b, n, 3 h d] buffer")
    d = c // (3 * heads)
    if d != 64:
        raise RuntimeError("the bf16-storage attention is built for head dim 64")
    return b, n, c, d


def _part(t, i, hd):
    """device pointer of part i (0 q, 1 k, 2 v) of a qkv-shaped bf16 buffer (same strides, shifted base)"""
    _bptr(t)
    return C_.c_void_p(t.data_ptr() + 2 * i * hd)


class _QKVProject16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, heads, l, pad):
        if x.dtype != torch.bfloat16:
            raise RuntimeError("qkv_project16: x must be bf16")
        ctx.det = DETERMINISTIC
        x = x if x.is_contiguous() else x.contiguous()
        wb = weight.detach().to(torch.bfloat16)
        b, n0, K = x.shape
        n = n0 + pad                                               # rows of a bag in the buffers: `pad` zero rows in front
        N = weight.shape[0]
        d = N // (3 * heads)
        qkv = torch.empty(b, n, N, device=x.device, dtype=torch.bfloat16)
        if pad:
            qkv[:, :pad].zero_()                                   # x W^T of a zero row (the projection has no bias)
        gemm_b16(x, wb, qkv, M=n0, N=N, K=K, lda=K, ldb=K, ldc=N, nb=b, sa=n0 * K, sc=n * N, c_off=pad * N)
        m = n // l
        ql = torch.empty(b, heads, m, d, device=x.device, dtype=torch.float32)
        kl = torch.empty_like(ql)
        capi.check(capi.lib().smml_segment_mean_b16(_bptr(qkv), capi.fptr(ql), capi.fptr(kl), b, n, l, heads, d, capi.stream()), "segment_mean_b16")
        ctx.cfg = (heads, l, d, pad)
        ctx.save_for_backward(x, wb)
        return qkv, ql, kl

    @staticmethod
    def backward(ctx, dqkv, dql, dkl):
        x, wb = ctx.saved_tensors
        heads, l, d, pad = ctx.cfg
        if ctx.det and ctx.needs_input_grad[1]:
            _no_det("qkv_project16 backward (weight gradient)", "the bf16-storage GEMM adds the slices of its split reduction with float "
                    "atomics (smml_gemm_b16_batched)")
        b, n0, K = x.shape
        n = n0 + pad
        N = wb.shape[0]
        if dqkv is None:
            dqkv = torch.zeros(b, n, N, device=x.device, dtype=torch.bfloat16)
        dqkv = dqkv if dqkv.is_contiguous() else dqkv.contiguous()
        if dql is not None or dkl is not None:
            zero = None
            if dql is None or dkl is None:
                zero = torch.zeros(b, heads, n // l, d, device=x.device, dtype=torch.float32)
            capi.check(capi.lib().smml_segment_mean_bwd_add_b16(_bptr(dqkv), capi.fptr(_c(dql) if dql is not None else zero),
                                                                capi.fptr(_c(dkl) if dkl is not None else zero), b, n, l, heads, d,
                                                                capi.stream()), "segment_mean_bwd_add_b16")
        dx = dw = None
        if ctx.needs_input_grad[0]:
            wt = wb.t().contiguous()
            dx = torch.empty_like(x)
            gemm_b16(dqkv, wt, dx, M=n0, N=K, K=N, lda=N, ldb=N, ldc=K, nb=b, sa=n * N, sc=n0 * K, a_off=pad * N)
        if ctx.needs_input_grad[1]:
            dw = _ZEROS.zeros((N, K), x.device)
            gemm_b16(dqkv, x, dw, M=N, N=K, K=n0, lda=N, ldb=K, ldc=K, trans=True, splitk=0, nb=b,
                     sa=n * N, sb=n0 * K, sc=0, a_off=pad * N)
        return dx, dw, None, None, None


def qkv_project16(x, weight, heads: int, l: int, pad: int = 0):
    """x bf16 [b, n0, K] -> (qkv bf16 [b, n, 3 h d], n = pad + n0: `pad` zero rows in front of every bag (NystromAttention.py:82), then x W^T;
    ql, kl fp32 [b, h, n / l, d] = means of q / k over l consecutive tokens).  The padded bag is never materialised: the GEMMs address
    a bag's real rows in place."""
    return _QKVProject16.apply(x, weight, heads, l, pad)


class _Attention16KeysLong(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ql, qkv, heads, scale, dv_accumulate):
        b, n, c, d = _qkv_dims(qkv, heads)
        ql = _c(ql)
        m = ql.shape[2]
        out = torch.empty(b, heads, m, d, device=qkv.device, dtype=torch.float32)
        lse2 = torch.empty(b * heads, m, device=qkv.device, dtype=torch.float32)
        L = capi.lib()
        wsb = L.smml_attn16_fwd_workspace_bytes(b * heads, m, n)
        ws = torch.empty((wsb + 3) // 4, device=qkv.device, dtype=torch.float32) if wsb else None
        hd = heads * d
        capi.check(L.smml_attn16_fwd_b16(capi.fptr(ql), _part(qkv, 1, hd), _part(qkv, 2, hd), capi.fptr(out), None, capi.fptr(lse2),
                                         capi.fptr(ws), wsb, b, heads, m, n, float(scale), 0, n * c, d, c, 0, 0, 0, capi.stream()),
                   "attn16_fwd_b16 (keys long)")
        ctx.cfg = (heads, float(scale), bool(dv_accumulate))
        ctx.save_for_backward(ql, qkv, out, lse2)
        return out, qkv

    @staticmethod
    def backward(ctx, dout, dqkv):
        ql, qkv, out, lse2 = ctx.saved_tensors
        heads, scale, dv_acc = ctx.cfg
        b, n, c, d = _qkv_dims(qkv, heads)
        m = ql.shape[2]
        hd = heads * d
        if dqkv is None:                                   # nothing after this stage contributed: start the buffer here
            dqkv = torch.zeros_like(qkv)
            dv_acc = True
        if dout is None:                                   # this product has no gradient: its parts of the buffer must still be defined
            parts = dqkv.view(b, n, 3, hd)
            parts[:, :, 1].zero_()
            if not dv_acc:
                parts[:, :, 2].zero_()
            return None, dqkv, None, None, None
        dout = _c(dout)
        dql = torch.empty_like(ql)
        L = capi.lib()
        wsb = L.smml_attn16_bwd_workspace_bytes(b * heads, m, n)
        ws = torch.empty((wsb + 3) // 4, device=qkv.device, dtype=torch.float32)
        capi.check(L.smml_attn16_bwd_b16(capi.fptr(ql), _part(qkv, 1, hd), _part(qkv, 2, hd), capi.fptr(out), None, capi.fptr(dout),
                                         capi.fptr(lse2), capi.fptr(dql), _part(dqkv, 1, hd), _part(dqkv, 2, hd), capi.fptr(ws), wsb, b,
                                         heads, m, n, scale, 0, n * c, d, c, 0, 0, 0, n * c, d, c, int(dv_acc), capi.stream()),
                   "attn16_bwd_b16 (keys long)")
        return dql, dqkv, None, None, None


def attention16_keys_long(ql, qkv, *, heads: int, scale: float, dv_accumulate: bool):
    """softmax(scale ql k^T) v with k / v read in the qkv buffer -> (fp32 [b, h, m, 64], qkv).  Backward writes dk into the k part of the
    threaded gradient buffer and writes (dv_accumulate False) or adds (True: a stage after this one already wrote dv) its dv."""
    return _Attention16KeysLong.apply(ql, qkv, heads, scale, dv_accumulate)


class _ResConv16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, w, heads):
        b, n, c, d = _qkv_dims(qkv, heads)
        ctx.det = DETERMINISTIC
        hd = heads * d
        kw = w.shape[2]
        w2 = _c(w.reshape(heads, kw))
        res = torch.empty(b, n, hd, device=qkv.device, dtype=torch.bfloat16)
        capi.check(capi.lib().smml_resconv_b16(_part(qkv, 2, hd), capi.fptr(w2), _bptr(res), b, heads, n, d, kw, n * c, c, n * hd, hd, 0,
                                               capi.stream()), "resconv_b16")
        ctx.cfg = (heads, kw, tuple(w.shape))
        ctx.save_for_backward(qkv, w2)
        return res, qkv

    @staticmethod
    def backward(ctx, dres, dqkv):
        qkv, w2 = ctx.saved_tensors
        heads, kw, wshape = ctx.cfg
        if ctx.det and dres is not None and ctx.needs_input_grad[1]:
            _no_det("resconv16 backward (weight gradient)", "the depthwise-convolution weight gradient of the Nystrom block is summed with "
                    "float atomics (smml_resconv_wgrad_b16)")
        b, n, c, d = _qkv_dims(qkv, heads)
        hd = heads * d
        if dqkv is None:
            dqkv = torch.zeros_like(qkv)
        dw = None
        if dres is None:                                   # no gradient through the convolution: the v part must still be defined
            dqkv.view(b, n, 3, hd)[:, :, 2].zero_()
        else:
            dres = dres if dres.is_contiguous() else dres.contiguous()
            L = capi.lib()
            capi.check(L.smml_resconv_b16(_bptr(dres), capi.fptr(w2), _part(dqkv, 2, hd), b, heads, n, d, kw, n * hd, hd, n * c, c, 1,
                                          capi.stream()), "resconv_b16 (data gradient)")
            if ctx.needs_input_grad[1]:
                dw2 = _ZEROS.zeros((heads, kw), qkv.device)
                capi.check(L.smml_resconv_wgrad_b16(_bptr(dres), _part(qkv, 2, hd), capi.fptr(dw2), b, heads, n, d, kw, n * hd, hd, n * c, c,
                                                    capi.stream()), "resconv_wgrad_b16")
                dw = dw2.view(wshape)
        return dqkv, dw, None


def resconv16(qkv, w, *, heads: int):
    """depthwise 33-tap convolution of v over tokens, v read in the qkv buffer -> (bf16 [b, n, h 64], qkv).  Backward WRITES the v part of the
    threaded gradient buffer (it is the first stage of the backward chain that touches it)."""
    return _ResConv16.apply(qkv, w, heads)


class _Attention16QueriesLong(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, kl, w, residual, heads, scale):
        b, n, c, d = _qkv_dims(qkv, heads)
        kl, w = _c(kl), _c(w)
        m = kl.shape[2]
        hd = heads * d
        if residual is not None and (residual.dtype != torch.bfloat16 or tuple(residual.shape) != (b, n, hd) or not residual.is_contiguous()):
            raise RuntimeError("attention16_queries_long: the residual is a contiguous bf16 [b, n, h 64] tensor")
        out = torch.empty(b, n, hd, device=qkv.device, dtype=torch.bfloat16)
        lse2 = torch.empty(b * heads, n, device=qkv.device, dtype=torch.float32)
        capi.check(capi.lib().smml_attn16_fwd_b16(_part(qkv, 0, hd), capi.fptr(kl), capi.fptr(w), _bptr(out),
                                                  _bptr(residual) if residual is not None else None, capi.fptr(lse2), None, 0, b, heads, n, m,
                                                  float(scale), 1, n * c, d, c, n * hd, d, hd, capi.stream()), "attn16_fwd_b16 (queries long)")
        ctx.cfg = (heads, float(scale), residual is not None)
        ctx.save_for_backward(qkv, kl, w, out, residual, lse2)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, kl, w, out, residual, lse2 = ctx.saved_tensors
        heads, scale, has_res = ctx.cfg
        b, n, c, d = _qkv_dims(qkv, heads)
        m = kl.shape[2]
        hd = heads * d
        if dout.dtype != torch.bfloat16:
            dout = dout.to(torch.bfloat16)
        dout = dout if dout.is_contiguous() else dout.contiguous()
        dqkv = torch.empty_like(qkv)                       # the head of the backward chain: q part written here, k / v parts by the earlier stages
        dkl, dw = torch.empty_like(kl), torch.empty_like(w)
        L = capi.lib()
        wsb = L.smml_attn16_bwd_workspace_bytes(b * heads, n, m)
        ws = torch.empty((wsb + 3) // 4, device=qkv.device, dtype=torch.float32)
        capi.check(L.smml_attn16_bwd_b16(_part(qkv, 0, hd), capi.fptr(kl), capi.fptr(w), _bptr(out), _bptr(residual) if has_res else None,
                                         _bptr(dout), capi.fptr(lse2), _part(dqkv, 0, hd), capi.fptr(dkl), capi.fptr(dw), capi.fptr(ws), wsb,
                                         b, heads, n, m, scale, 1, n * c, d, c, n * hd, d, hd, n * c, d, c, 0, capi.stream()),
                   "attn16_bwd_b16 (queries long)")
        return dqkv, dkl, dw, (dout if has_res else None), None, None


def attention16_queries_long(qkv, kl, w, residual=None, *, heads: int, scale: float):
    """softmax(scale q kl^T) w + residual with q read in the qkv buffer -> bf16 [b, n, h 64] (the output projection's operand).  Backward
    allocates the threaded gradient buffer dqkv and writes its q part; the k and v parts are left to the stages before this one."""
    return _Attention16QueriesLong.apply(qkv, kl, w, residual, heads, scale)


class _HeadMajorQKV(torch.autograd.Function):
    """qkv [b, n, 3 h d] (bf16 or fp32, token-major: what the projection writes) -> q, k, v fp32 [b, h, n, d], three slices of one buffer filled by
    ONE strided copy; backward writes the three gradients into one token-major buffer of the input's dtype (no stack / cat of head-major pieces)."""

    @staticmethod
    def forward(ctx, qkv, heads):
        b, n, c = qkv.shape
        d = c // (3 * heads)
        ctx.shape = (b, n, heads, d)
        ctx.in_dtype = qkv.dtype                  # bf16 (the bf16 projections) or fp32 (exact path, fp16 mode): the gradient buffer follows it
        buf = torch.empty(3, b, heads, n, d, device=qkv.device, dtype=torch.float32)
        buf.copy_(qkv.view(b, n, 3, heads, d).permute(2, 0, 3, 1, 4))
        return buf[0], buf[1], buf[2]

    @staticmethod
    def backward(ctx, dq, dk, dv):
        b, n, h, d = ctx.shape
        dqkv = torch.empty(b, n, 3, h, d, device=dq.device, dtype=ctx.in_dtype)
        view = dqkv.permute(2, 0, 3, 1, 4)
        for i, g in enumerate((dq, dk, dv)):
            if g is None:
                view[i].zero_()
            else:
                view[i].copy_(g)
        return dqkv.view(b, n, 3 * h * d), None


def head_major_qkv(qkv, heads: int):
    return _HeadMajorQKV.apply(qkv, heads)


# ------------------------------------------------------------------------------------------------
# grouped 1x1 convolution on token-major data: x [B, n, Cin], w [Cout, Cin / groups] -> [B, n, Cout]
# ------------------------------------------------------------------------------------------------
class _GroupedPointwise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, groups):
        x = _c(x)
        ctx.det = DETERMINISTIC
        w = _c(weight).reshape(weight.shape[0], -1)
        Cin, Cout = x.shape[-1], w.shape[0]
        cin_g, cout_g = Cin // groups, Cout // groups
        assert w.shape[1] == cin_g, "weight does not match the group structure"
        M = x.numel() // Cin
        y = torch.empty(*x.shape[:-1], Cout, device=x.device, dtype=torch.float32)
        # the streaming kernels (csrc/grouped_pointwise.hip) where the group shape is theirs; every other shape is a batch over the groups
        ctx.streaming = bool(capi.lib().smml_grouped_pointwise_applies(groups, cin_g, cout_g)) and _al16(x, w)
        if ctx.streaming:
            capi.check(capi.lib().smml_grouped_pointwise_fwd_f32(capi.fptr(x), capi.fptr(w), capi.fptr(y), M, groups, cin_g, cout_g,
                                                                 capi.stream()), "grouped_pointwise fwd")
        else:
            _gemm(x, w, y, M=M, N=cout_g, K=cin_g, sam=Cin, sak=1, sbk=1, sbn=cin_g, ldc=Cout, nb1=groups,
                  sa1=cin_g, sb1=cout_g * cin_g, sc1=cout_g)
        ctx.groups = groups
        ctx.wshape = weight.shape
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _c(dy)
        G = ctx.groups
        Cin, Cout = x.shape[-1], w.shape[0]
        cin_g, cout_g = Cin // G, Cout // G
        M = x.numel() // Cin
        dx = dw = None
        if ctx.streaming and _al16(dy):
            L = capi.lib()
            if ctx.needs_input_grad[0]:
                dx = torch.empty_like(x)
                capi.check(L.smml_grouped_pointwise_dx_f32(capi.fptr(dy), capi.fptr(w), capi.fptr(dx), M, G, cin_g, cout_g, capi.stream()),
                           "grouped_pointwise dx")
            if ctx.needs_input_grad[1]:
                # one form for both modes: per-workgroup partials added in a fixed order, no zero fill and no float atomics
                dw = torch.empty_like(w)
                wsb = L.smml_grouped_pointwise_dw_workspace_bytes(M, G, cin_g, cout_g)
                ws = _scratch(wsb, dy.device)
                capi.check(L.smml_grouped_pointwise_dw_f32(capi.fptr(dy), capi.fptr(x), capi.fptr(dw), M, G, cin_g, cout_g, capi.fptr(ws), wsb,
                                                           capi.stream()), "grouped_pointwise dw")
                dw = dw.reshape(ctx.wshape)
            return dx, dw, None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _gemm(dy, w, dx, M=M, N=cin_g, K=cout_g, sam=Cout, sak=1, sbk=cin_g, sbn=1, ldc=Cin, nb1=G,
                  sa1=cout_g, sb1=cout_g * cin_g, sc1=cin_g)
        if ctx.needs_input_grad[1]:
            dw = torch.empty_like(w) if ctx.det else _zeros_like(w)
            _gemm(dy, x, dw, M=cout_g, N=cin_g, K=M, sam=1, sak=Cout, sbk=Cin, sbn=1, ldc=cin_g, nb1=G,
                  sa1=cout_g, sb1=cin_g, sc1=cout_g * cin_g, splitk=_splitk_for(cout_g, cin_g, M, G), det=ctx.det)
            dw = dw.reshape(ctx.wshape)
        return dx, dw, None


def grouped_pointwise(x, weight, groups: int = 1):
    return _GroupedPointwise.apply(x, weight, groups)


# ------------------------------------------------------------------------------------------------
# LayerNorm (optionally followed by the mean over tokens, Pooler's first step)
# ------------------------------------------------------------------------------------------------
class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, token_mean, fork=None):
        ctx.fork = fork
        x = _c(x); gamma = _c(gamma); beta = _c(beta)
        Cc = x.shape[-1]
        R = x.numel() // Cc
        mean = torch.empty(R, device=x.device, dtype=torch.float32)
        rstd = torch.empty(R, device=x.device, dtype=torch.float32)
        ctx.token_mean = token_mean
        ctx.det = DETERMINISTIC
        ctx.save_for_backward(x, gamma, mean, rstd)
        if token_mean:
            assert x.dim() == 3
            if Cc == 128 and _al16(x, gamma, beta):       # the path's width: one pass over x, the normalised tensor is never stored
                return _layernorm_mean128(x, gamma, beta, mean, rstd, float(eps), ctx.det)
        y = torch.empty_like(x)
        capi.check(capi.lib().smml_layernorm_fwd_f32(capi.fptr(x), capi.fptr(gamma), capi.fptr(beta), capi.fptr(y),
                                                     capi.fptr(mean), capi.fptr(rstd), R, Cc, float(eps),
                                                     capi.stream()), "layernorm_fwd")
        if token_mean:
            return colsum(y, 1.0 / x.shape[1], det=ctx.det)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        dy = _c(dy)
        Cc = x.shape[-1]
        R = x.numel() // Cc
        fork = ctx.fork if ctx.needs_input_grad[0] else None
        parked = fork.take("norm", x) if fork is not None else None
        acc = parked is not None                   # GradSum: x's other gradient is there - this one is added into it (accumulate_dx = 1)
        dx = parked if acc else torch.empty_like(x)
        dg = _zeros_like(gamma)
        db = _zeros_like(gamma)
        rows_per_dy, scale = (x.shape[1], 1.0 / x.shape[1]) if ctx.token_mean else (1, 1.0)
        if ctx.det:
            L = capi.lib()
            wsb = L.smml_layernorm_bwd_det_workspace_bytes(R, Cc)
            ws = _scratch(wsb, x.device)
            capi.check(L.smml_layernorm_bwd_det_f32(capi.fptr(x), capi.fptr(dy), capi.fptr(gamma), capi.fptr(mean), capi.fptr(rstd),
                                                    capi.fptr(dx), capi.fptr(dg), capi.fptr(db), R, Cc, rows_per_dy, float(scale), int(acc),
                                                    capi.fptr(ws), wsb, capi.stream()), "layernorm_bwd (deterministic)")
        else:
            capi.check(capi.lib().smml_layernorm_bwd_f32(capi.fptr(x), capi.fptr(dy), capi.fptr(gamma), capi.fptr(mean),
                                                         capi.fptr(rstd), capi.fptr(dx), capi.fptr(dg), capi.fptr(db), R, Cc,
                                                         rows_per_dy, float(scale), int(acc), capi.stream()), "layernorm_bwd")
        if fork is not None and not acc:
            fork.park("norm", dx)
        return (None if acc else dx), dg, db, None, None, None


def _layernorm_mean128(x, gamma, beta, mean, rstd, eps: float, det: bool) -> torch.Tensor:
    """x [B, n, 128] -> the mean over tokens of LayerNorm(x) [B, 128]; fills mean / rstd (include/smml.h smml_layernorm_fwd_mean_f32)"""
    L = capi.lib()
    nb, n, Cc = x.shape
    if det:
        out = torch.empty(nb, Cc, device=x.device, dtype=torch.float32)
        wsb = L.smml_layernorm_fwd_mean_det_workspace_bytes(nb, n, Cc)
        ws = _scratch(wsb, x.device)
        capi.check(L.smml_layernorm_fwd_mean_det_f32(capi.fptr(x), capi.fptr(gamma), capi.fptr(beta), capi.fptr(mean), capi.fptr(rstd),
                                                     capi.fptr(out), nb, n, Cc, eps, capi.fptr(ws), wsb, capi.stream()),
                   "layernorm_fwd_mean (deterministic)")
        return out
    out = _ZEROS.zeros((nb, Cc), x.device)
    capi.check(L.smml_layernorm_fwd_mean_f32(capi.fptr(x), capi.fptr(gamma), capi.fptr(beta), capi.fptr(mean), capi.fptr(rstd),
                                             capi.fptr(out), nb, n, Cc, eps, capi.stream()), "layernorm_fwd_mean")
    return out


def layer_norm(x, gamma, beta, eps: float = 1e-5):
    return _LayerNorm.apply(x, gamma, beta, eps, False, _fork_of(x))       # a GradSum riding on x (grad_sum)


def layer_norm_token_mean(x, gamma, beta, eps: float = 1e-5):
    """mean over tokens of LayerNorm(x): x [B, n, C] -> [B, C]."""
    return _LayerNorm.apply(x, gamma, beta, eps, True, None)


# ------------------------------------------------------------------------------------------------
# offset network: q [B, Hh, Ww, G*dg] -> vgrid [(B G), posdim, th, tw] (or [(B G), t]), vs [(B G), J, posdim]
# ------------------------------------------------------------------------------------------------
class GradFork:
    """q feeds two consumers - the offsets network and the fused attention core - and autograd would add their two [B, N, 512] gradients with
    an elementwise kernel (492 MB of traffic per 8-bag step).  The attention's backward always runs first (the offsets network's backward
    needs the d vs it produces): it parks its dq here, the offsets backward ADDS its own contribution into that buffer in place
    (smml_offsets_bwd_f32, accumulate_dq = 1) and reports no gradient of its own for q.  One object per forward call; None = plain autograd."""
    __slots__ = ("dq",)

    def __init__(self):
        self.dq = None


class _Offsets(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, w0, b0, w2, groups, ks, r, posdim, offset_scale, fork=None):
        ctx.fork = fork
        q = _c(q); w0c = _c(w0); b0c = _c(b0); w2c = _c(w2)
        B, Hh, Ww, inner = q.shape
        dg = inner // groups
        L = capi.lib()
        tw = L.smml_offsets_out_len(Ww, ks, r)
        th = L.smml_offsets_out_len(Hh, ks, r) if posdim == 2 else 1
        if th <= 0 or tw <= 0:
            raise RuntimeError("token grid too small for the offset convolution")
        J = th * tw
        vgrid = torch.empty((B * groups, 2, th, tw) if posdim == 2 else (B * groups, tw), device=q.device,
                            dtype=torch.float32)
        vs = torch.empty(B * groups, J, posdim, device=q.device, dtype=torch.float32)
        capi.check(L.smml_offsets_fwd_f32(capi.fptr(q), capi.fptr(w0c), capi.fptr(b0c), capi.fptr(w2c),
                                          capi.fptr(vgrid), capi.fptr(vs), B, Hh, Ww, groups, dg, ks, r, posdim,
                                          float(offset_scale), capi.stream()), "offsets_fwd")
        ctx.cfg = (groups, ks, r, posdim, float(offset_scale))
        ctx.save_for_backward(q, w0c, b0c, w2c)
        return vgrid, vs

    @staticmethod
    def backward(ctx, dvgrid, dvs):
        q, w0, b0, w2 = ctx.saved_tensors
        groups, ks, r, posdim, offset_scale = ctx.cfg
        B, Hh, Ww, inner = q.shape
        dg = inner // groups
        fork = ctx.fork
        parked = fork.dq if fork is not None else None
        if fork is not None:
            fork.dq = None
        acc = parked is not None and parked.numel() == q.numel() and parked.is_contiguous() and parked.dtype == torch.float32
        dq = parked if acc else torch.empty_like(q)
        dw0, db0, dw2 = torch.empty_like(w0), torch.empty_like(b0), torch.empty_like(w2)
        dvgrid = _c(dvgrid) if dvgrid is not None else None
        dvs = _c(dvs) if dvs is not None else None
        L = capi.lib()
        wsb = L.smml_offsets_bwd_workspace_bytes(B, Hh, Ww, groups, dg, ks, r, posdim)
        ws = torch.empty((wsb + 3) // 4, device=q.device, dtype=torch.float32)
        capi.check(L.smml_offsets_bwd_f32(capi.fptr(q), capi.fptr(w0), capi.fptr(b0), capi.fptr(w2),
                                          capi.fptr(dvgrid), capi.fptr(dvs), capi.fptr(dq), capi.fptr(dw0),
                                          capi.fptr(db0), capi.fptr(dw2), capi.fptr(ws), wsb, B, Hh, Ww, groups, dg, ks, r,
                                          posdim, offset_scale, 1 if acc else 0, capi.stream()), "offsets_bwd")
        # acc: the contribution went into the attention's dq in place - autograd already holds that tensor as q's gradient
        return (None if acc else dq), dw0, db0, dw2, None, None, None, None, None, None


def offsets(q, w0, b0, w2, *, groups, ks, r, posdim, offset_scale, fork=None):
    """fork: a GradFork shared with the deform_attention call that consumes the same q (see GradFork)."""
    return _Offsets.apply(q, w0, b0, w2, groups, ks, r, posdim, offset_scale, fork)


# ------------------------------------------------------------------------------------------------
# bilinear sampling: x [B, Hh, Ww, C], vs [(B G), J, posdim] -> kv [B, J, C]
# ------------------------------------------------------------------------------------------------
class _Sample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, vs, groups, posdim):
        x = _c(x); vs = _c(vs)
        B, Hh, Ww, Cc = x.shape
        J = vs.shape[1]
        kv = torch.empty(B, J, Cc, device=x.device, dtype=torch.float32)
        capi.check(capi.lib().smml_bilinear_sample_fwd_f32(capi.fptr(x), capi.fptr(vs), capi.fptr(kv), B, Hh, Ww, groups,
                                                           Cc // groups, J, posdim, capi.stream()), "sample_fwd")
        ctx.cfg = (groups, posdim)
        ctx.det = DETERMINISTIC
        ctx.save_for_backward(x, vs)
        if DECISION_TAP is not None:
            DECISION_TAP.append({"kind": "sample", "vs": vs.detach(), "Hh": Hh, "Ww": Ww, "posdim": posdim})
        return kv

    @staticmethod
    def backward(ctx, dkv):
        x, vs = ctx.saved_tensors
        groups, posdim = ctx.cfg
        B, Hh, Ww, Cc = x.shape
        J = vs.shape[1]
        if ctx.det:        # dx is a gather in a fixed order (written in full: no zero fill); dvs has one owner per point either way
            L = capi.lib()
            dx = torch.empty_like(x)
            dvs = _zeros_like(vs)
            wsb = L.smml_bilinear_sample_bwd_det_workspace_bytes(B, Hh, Ww, groups, J)
            ws = _scratch(wsb, x.device)
            capi.check(L.smml_bilinear_sample_bwd_det_f32(capi.fptr(x), capi.fptr(vs), capi.fptr(_c(dkv)), capi.fptr(dx), capi.fptr(dvs),
                                                          capi.fptr(ws), wsb, B, Hh, Ww, groups, Cc // groups, J, posdim, capi.stream()),
                       "sample_bwd (deterministic)")
            return dx, dvs, None, None
        dx = torch.zeros_like(x)
        dvs = _zeros_like(vs)
        capi.check(capi.lib().smml_bilinear_sample_bwd_f32(capi.fptr(x), capi.fptr(vs), capi.fptr(_c(dkv)), capi.fptr(dx),
                                                           capi.fptr(dvs), B, Hh, Ww, groups, Cc // groups, J, posdim,
                                                           capi.stream()), "sample_bwd")
        return dx, dvs, None, None


def bilinear_sample(x, vs, *, groups, posdim):
    return _Sample.apply(x, vs, groups, posdim)


def bilinear_corners(vs, Hh: int, Ww: int, posdim: int):
    """Integer path of the sampler for vs [n, posdim]: (cx [n,4] int32, cy [n,4] int32, mask [n,4] uint8)."""
    vs = _c(vs).reshape(-1, posdim)
    n = vs.shape[0]
    cx = torch.empty(n, 4, device=vs.device, dtype=torch.int32)
    cy = torch.empty(n, 4, device=vs.device, dtype=torch.int32)
    cm = torch.empty(n, 4, device=vs.device, dtype=torch.uint8)
    capi.check(capi.lib().smml_bilinear_corners_f32(capi.fptr(vs), capi.ptr(cx), capi.ptr(cy), capi.ptr(cm), n, Hh, Ww,
                                                    posdim, capi.stream()), "corners")
    return cx, cy, cm


# ------------------------------------------------------------------------------------------------
# fused attention core with continuous position bias
# ------------------------------------------------------------------------------------------------
_DTYPE16 = {"bf16": (0, torch.bfloat16), "fp16": (1, torch.float16)}


def prec16(compute_dtype) -> int:
    """GEMM precision mode (`linear(..., prec=)`) that goes with a 16-bit compute mode: None -> 0 (exact), 'bf16' -> 3, 'fp16' -> 4."""
    m = _dtype16(compute_dtype)
    return 0 if m is None else (4 if m[0] == 1 else 3)


def _dtype16(compute_dtype):
    """None (the fp32-grade path) or the (C-ABI code, torch dtype) of the 16-bit compute mode."""
    if compute_dtype is None:
        return None
    key = {"bfloat16": "bf16", "float16": "fp16", "half": "fp16"}.get(str(compute_dtype).replace("torch.", ""),
                                                                      str(compute_dtype).replace("torch.", ""))
    if key not in _DTYPE16:
        raise ValueError(f"compute_dtype must be None, 'bf16' or 'fp16' (got {compute_dtype!r})")
    return _DTYPE16[key]


# layer-2 decisions of a cpb_table='forward' backward: 'table' (mask table, include/smml.h) or 'recompute' (layer 2 per pair); measurement / test switch
TABLE_FORWARD_MASKS = os.environ.get("SMML_TABFWD_MASKS", "table")


# fp32-grade path, 2-D positions: the position bias per LINEAR REGION of its MLP (csrc/cpb_regions.h, include/smml.h) - exact, and the
# default wherever it applies (signed-log offsets, one head per offset group, J <= REGION_MAX_KEYS).  SMML_CPB_REGIONS=0 keeps the per-pair MLP
# kernels (the cross-check of tests/test_gpu_regions.py, and the path of every other configuration).
CPB_REGIONS = os.environ.get("SMML_CPB_REGIONS", "1") != "0"
REGION_MAX_KEYS = 16384      # RG_MAX_KEYS of csrc/cpb_regions.h
REGION_LDS_CAP = 0           # tests: regions with an id >= this take the global-memory path of the region kernels (0: the default, 2048)


REGION_GRID, REGION_SUB, REGION_SUBCAP, REGION_EDGES, REGION_RCAP = 1024, 8, 16384, 1 << 15, 4096     # csrc/cpb_regions.h
REGION_CODE_SUB0, REGION_CODE_EDGE0 = 4096, 4096 + 16384
REGION_HASH, REGION_CANDCAP, REGION_WD = 16384, 1 << 18, 1232                                         # csrc/cpb_regions.h (build scratch)


def _blocks(tables: torch.Tensor, *sizes):
    """Consecutive blocks of a table buffer, each starting on a 256-byte boundary (the take() of region_layout() / region1d_layout())."""
    out, o = [], 0
    for n in sizes:
        out.append(tables[o:o + n])
        o += (n + 255) & ~255
    return out


def region_tables_view(tables: torch.Tensor):
    """Views into a region-table buffer (tests / diagnostics; layout: region_layout() of csrc/cpb_regions.h): header counters,
    (a0, a1, c) per region, ReLU patterns (D1 | D2 << 32), 16-bit codes of the cells and sub-cells, single-kink records by slot, and
    "reg1": the (a0, a1, c) of the MLP's second output (tables of two heads per offset group, smml_cpb_regions_mh_build)."""
    G, SUB = REGION_GRID, REGION_SUB
    blocks = _blocks(tables, 256, REGION_RCAP * 16, REGION_RCAP * 8, G * G * 2, REGION_SUBCAP * SUB * SUB * 2, REGION_EDGES * 16,
                     # build scratch: t0, t1, ekey, hkey, hid, sublist, cand, klist, corners, subcorners, wd; then the second output's (a, c)
                     G * G * 4, REGION_SUBCAP * SUB * SUB * 4, REGION_EDGES * 4, REGION_HASH * 8, REGION_HASH * 4, REGION_SUBCAP * 4,
                     REGION_CANDCAP * 8, REGION_HASH * 12, (G + 1) ** 2 * 8, REGION_SUBCAP * (SUB + 1) ** 2 * 8, REGION_WD * 8,
                     REGION_RCAP * 16)
    hdr, reg, pat, t0, t1, edge = blocks[:6]
    reg1 = blocks[-1]
    hdr = hdr.view(torch.int32)
    n_sub, n_edge, n_regions = int(hdr[0]), int(hdr[1]), int(hdr[3])
    return {"n_sub": n_sub, "n_edge": n_edge, "n_cand": int(hdr[2]), "n_regions": n_regions, "n_keys": int(hdr[4]), "overflow": int(hdr[5]),
            "n_cand1": int(hdr[6]), "pmax": float(hdr[8:9].view(torch.float32)), "cs": float(hdr[9:10].view(torch.float32)),
            "co": float(hdr[10:11].view(torch.float32)),
            "reg": reg.view(torch.float32).view(REGION_RCAP, 4)[:n_regions],
            "pat": pat.view(torch.int64)[:n_regions],
            "t0": t0.view(torch.int16).view(G, G),
            "t1": t1.view(torch.int16).view(REGION_SUBCAP, SUB * SUB)[:max(min(n_sub, REGION_SUBCAP), 1)],
            "edge": edge.view(torch.float32).view(REGION_EDGES, 4),
            "reg1": reg1.view(torch.float32).view(REGION_RCAP, 4)[:n_regions]}


def region_patterns(region_ids: torch.Tensor, tables: torch.Tensor):
    """(D1, D2) int64 words of the linear piece of every pair of `region_ids` (tests: the ReLU decisions the region kernels stand for);
    pairs without a region (0xFFFF: they evaluated the MLP itself) get -1."""
    pat = region_tables_view(tables)["pat"]
    ids = region_ids.to(torch.int64) & 0xFFFF
    none = ids == 0xFFFF
    p = pat[ids.clamp_max(max(pat.numel() - 1, 0))] if pat.numel() else torch.zeros_like(ids)
    d1, d2 = p & 0xFFFFFFFF, (p >> 32) & 0xFFFFFFFF
    return torch.where(none, torch.full_like(d1, -1), d1), torch.where(none, torch.full_like(d2, -1), d2)


def cpb_regions_build(w1, b1, w2, b2, w3, b3, pmax: float, tables: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The region tables of the position-bias MLP with these parameters over [-pmax, pmax]^2 (uint8 scratch owned by the caller), built
    on the current stream.  w3 [outputs, 32] with outputs = heads per offset group: a second output adds its (a, c) (one buffer size
    for both)."""
    return _tables_build("cpb_regions_build" if w3.shape[0] == 1 else "cpb_regions_mh_build", capi.lib().smml_cpb_regions_bytes(),
                         (w1, b1, w2, b2, w3, b3), pmax, tables)


def _tables_build(entry: str, nbytes: int, mlp, pmax: float, tables: Optional[torch.Tensor]) -> torch.Tensor:
    """The 2-D region tables or the 1-D piece tables of the bias MLP `mlp` = (w1, b1, w2, b2, w3, b3), into `tables` (None: allocated)."""
    tables = torch.empty(nbytes, device=mlp[0].device, dtype=torch.uint8) if tables is None else tables
    w1, b1, w2, b2, w3, b3 = (_c(t) for t in mlp)
    ns = dict(w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3, outputs=int(w3.shape[0]), pmax=float(pmax), tables=tables, tables_bytes=nbytes,
              stream=capi.stream())
    capi.check(capi.call("smml_" + entry, ns, BUILD_KEYS), entry)
    return tables


# fp32-grade path, 1-D positions: the position bias per linear PIECE of its MLP (csrc/cpb_regions1d.h) - exact, opt-in (cpb_regions=True
# with 1-D positions; None keeps the per-pair kernels): signed-log offsets, heads // groups in {1, 2}, J <= REGION_MAX_KEYS.
REGION1D_MAXBP, REGION1D_CELLS, REGION1D_HPG = 32 + 33 * 32, 2048, 2          # csrc/cpb_regions1d.h


def region1d_tables_view(tables: torch.Tensor):
    """Views into a 1-D piece-table buffer (tests / diagnostics; layout: region1d_layout() of csrc/cpb_regions1d.h): breakpoint count,
    the sorted breakpoints (fp32 and fp64), per piece its ReLU pattern (D1 | D2 << 32) and (a, c) per output [pieces, outputs, 2], the index
    grid (first piece per cell) and its mapping cell = floor(p * inv + off)."""
    nb, npc, cells = REGION1D_MAXBP, REGION1D_MAXBP + 1, REGION1D_CELLS
    hdr, bp, pat, coef, first, bpd = _blocks(tables, 256, nb * 4, npc * 8, npc * 16, (cells + 1) * 2, nb * 8)
    hdr = hdr.view(torch.int32)
    n_bp, hpg = int(hdr[0]), int(hdr[1])
    return {"n_bp": n_bp, "n_pieces": n_bp + 1, "outputs": hpg, "pmax": float(hdr[4:5].view(torch.float32)),
            "inv": float(hdr[5:6].view(torch.float32)), "off": float(hdr[6:7].view(torch.float32)),
            "bp": bp.view(torch.float32)[:n_bp],
            "bpd": bpd.view(torch.float64)[:n_bp],
            "pat": pat.view(torch.int64)[:n_bp + 1],
            "coef": coef.view(torch.float32).view(npc, REGION1D_HPG, 2)[:n_bp + 1, :hpg],
            "first": first.view(torch.int16)}


def cpb_regions1d_build(w1, b1, w2, b2, w3, b3, pmax: float = 0.0, tables: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The piece tables of the 1-D position-bias MLP with these parameters (index grid over [-pmax, pmax]; 0: the span of the breakpoints),
    built on the current stream into uint8 scratch owned by the caller."""
    return _tables_build("cpb_regions1d_build", capi.lib().smml_cpb_regions1d_bytes(), (w1, b1, w2, b2, w3, b3), pmax, tables)


def _region_why(posdim: int, keys: int, w2_shape, w3_shape, heads: int, groups: int, compute_dtype, cpb_table, cpb_regions, log_distance: bool,
                region_pmax_given: bool, capturing: bool):
    """Why the exact position-bias path asked for (posdim 1: per linear piece; posdim 2: per linear region, one or two heads per offset
    group) cannot take a call; None: it can.  The rules of both, in the order each reports them."""
    hpg = heads // groups if groups > 0 and heads % groups == 0 else 0
    if not log_distance:
        return "raw distances (cpb_log_distance=False)"
    if posdim == 1 and compute_dtype is not None:
        return "the 16-bit compute modes"
    if cpb_table:
        return "the table modes"
    if cpb_regions is not None and not bool(cpb_regions):
        return "cpb_regions=False (the per-pair kernels)"
    if hpg not in (1, 2):
        return f"heads // groups = {heads // groups if groups > 0 else 0} (supported: 1, 2)"
    if keys > REGION_MAX_KEYS:
        return f"{keys} keys (at most {REGION_MAX_KEYS})"
    if tuple(w2_shape) != (32, 32) or tuple(w3_shape) != (hpg, 32):
        return f"a bias MLP other than {posdim} -> 32 -> 32 -> heads // groups"
    if posdim == 2 and capturing and not region_pmax_given:
        return "a hipGraph capture without cpb_region_pmax (its pmax would come from the data: a host sync)"
    return None


def region1d_unsupported(vs, k, w2, w3, *, heads: int, groups: int, compute_dtype=None, cpb_table=False, log_distance: bool = True):
    """Why the 1-D piece path cannot take this call (None: it can)."""
    if vs.shape[-1] != 1:
        return "the piece path is the 1-D position bias (posdim 1)"
    return _region_why(1, k.shape[1], w2.shape, w3.shape, heads, groups, compute_dtype, cpb_table, True, log_distance, True, False)


WIDE_W2_SHAPES = ((64, 64), (128, 128))      # layer 2 of the bias MLP at dim = 256 / 512: the wide family (csrc/deform_attn_wide.hip)


def _wide_path(posdim, heads, groups, w2_shape, w3_shape, log_distance, compute_dtype, cpb_table, cpb_regions, regions_multi_head) -> str:
    """'pair_wide', or ValueError naming the option the wide family (bias-MLP width 64 / 128) does not have: it is the fp32-grade per-pair
    core alone."""
    W = int(w2_shape[0])
    what = f"a position-bias MLP of width {W} (dim = {4 * W})"
    if _dtype16(compute_dtype) is not None:
        raise ValueError(f"compute_dtype={compute_dtype!r}: the 16-bit compute modes are built for width 32 (dim = 128), not for {what}")
    if cpb_table:
        raise ValueError(f"cpb_table={cpb_table!r}: the table modes are built for width 32 (dim = 128), not for {what}")
    if regions_multi_head:
        raise ValueError(f"cpb_regions_multi_head=True: the 2-D region path is built for width 32 (dim = 128), not for {what}")
    if cpb_regions is not None and bool(cpb_regions):
        name = "cpb_regions=True (the 1-D piece path, cpb_regions_1d)" if posdim == 1 else "cpb_regions=True (the region path)"
        raise ValueError(f"{name} is built for width 32 (dim = 128), not for {what}")
    if not log_distance and posdim != 1:
        raise NotImplementedError("the raw-offset position transform (cpb_log_distance=False) exists for 1-D positions without the table modes")
    hpg = heads // groups if groups > 0 and heads % groups == 0 else 0
    if hpg not in (1, 2) or tuple(w3_shape) != (hpg, W):
        raise ValueError(f"{what} needs heads // groups in (1, 2) and w3 of shape (heads // groups, {W}); got heads {heads}, groups {groups}, "
                         f"w3 {tuple(w3_shape)}")
    return "pair_wide"


def deform_path(*, posdim: int, heads: int, groups: int, keys: int, w2_shape=(32, 32), w3_shape=(1, 32), log_distance: bool = True,
                compute_dtype=None, cpb_table=False, cpb_regions=None, region_pmax_given: bool = False, capturing: bool = False,
                regions_multi_head: bool = False) -> str:
    """The core a deform_attention call with these shapes and options takes: 'region1d' (the 1-D position bias per linear piece), 'table',
    'pair_table_forward' (per-pair backward of a table forward), 'region' (2-D, per linear region; fp32-grade or 16-bit core), 'pair'
    (the per-pair MLP; fp32-grade or 16-bit core) or 'pair_wide' (bias-MLP width 64 / 128, w2_shape (64, 64) / (128, 128): the per-pair MLP in
    exact fp32, fp32-grade core only - every region, table or 16-bit option raises ValueError there).  Raises on a combination no core supports.  No GPU work; the module switches
    (CPB_REGIONS) are read at call time.  capturing: the call is being captured in a hipGraph (a 2-D region call then needs its pmax).
    regions_multi_head (2-D positions): the region path on request for one or two heads per offset group, in either compute mode; any
    combination it does not support raises ValueError (never a silent fall-back).  Without it the rules above are unchanged."""
    if cpb_table not in (False, True, None, "forward", "full"):
        raise ValueError("cpb_table must be False, True / 'full' or 'forward'")
    if tuple(w2_shape) in WIDE_W2_SHAPES:
        return _wide_path(posdim, heads, groups, w2_shape, w3_shape, log_distance, compute_dtype, cpb_table, cpb_regions, regions_multi_head)
    if cpb_regions is not None and bool(cpb_regions) and posdim == 1:
        # 1-D positions: the piece path only on request (cpb_regions=True), and never a silent fall-back from it
        why = _region_why(1, keys, w2_shape, w3_shape, heads, groups, compute_dtype, cpb_table, True, log_distance, True, False)
        if why is not None:
            raise ValueError(f"cpb_regions=True with 1-D positions: the piece path does not support {why}")
        return "region1d"
    if regions_multi_head and posdim == 2:
        _dtype16(compute_dtype)
        why = _region_why(2, keys, w2_shape, w3_shape, heads, groups, compute_dtype, cpb_table, cpb_regions, log_distance, region_pmax_given,
                          capturing)
        if why is not None:
            raise ValueError(f"cpb_regions_multi_head=True: the 2-D region path does not support {why}")
        return "region"
    m16 = _dtype16(compute_dtype)
    if cpb_table and cpb_table != "forward" and DETERMINISTIC:
        _no_det(f"the table mode of the position bias (cpb_table={cpb_table!r})", "its backward adds d table with float atomics "
                "(cpb_table_bwd_kernel, dtab)")
    if cpb_table:
        if not log_distance:
            raise NotImplementedError("the table modes are built for the signed-log position transform only")
        if m16 is None and cpb_table == "forward":
            raise ValueError("cpb_table belongs to the 16-bit compute modes: pass compute_dtype='bf16' or 'fp16'")
        if m16 is None:
            raise ValueError("the table mode belongs to the 16-bit compute modes: pass compute_dtype='bf16' or 'fp16'")
        return "pair_table_forward" if cpb_table == "forward" else "table"
    if not log_distance and posdim != 1:
        raise NotImplementedError("the raw-offset position transform (cpb_log_distance=False) exists for 1-D positions without the table modes")
    # the position bias per linear region wherever that applies (CPB_REGIONS; cpb_regions False / True overrides it); its pmax comes from
    # the data when not given - a host sync, impossible inside a hipGraph capture: such a call keeps the per-pair kernels
    use_regions = CPB_REGIONS if cpb_regions is None else bool(cpb_regions)
    if (use_regions and log_distance and posdim == 2 and heads == groups and keys <= REGION_MAX_KEYS and tuple(w3_shape) == (1, 32)
            and (region_pmax_given or not capturing)):
        return "region"
    return "pair"


# ---- shared pieces of the fused-core Functions
def _check_core(q, heads: int, w2=None):
    if q.shape[-1] != heads * 64:
        raise RuntimeError("the attention kernels are built for dim_head = 64")
    if w2 is not None and tuple(w2.shape) != (32, 32):
        raise RuntimeError("the position-bias kernels are built for a hidden width of 32 (dim = 128)")


def _score_tiles(q, heads: int, J: int, dtype, *inner):
    """A score-shaped tensor, stored per 32-query tile (include/smml.h): [B, H, nst / 32, J, *inner, 32]."""
    B, N, _ = q.shape
    nst = capi.lib().smml_deform_attn_nst(N)
    return torch.empty(B, heads, nst // 32, J, *inner, 32, device=q.device, dtype=dtype)


class AttnScores:
    """Sink for what ONE deform_attention call saved of its softmax (deform_attention(..., attn_scores=AttnScores())): the score tiles
    logits_t [B, H, nst / 32, J, 32] fp32 and lse [B, H, N] of include/smml.h, kept whether or not a backward follows - the fused forward
    writes them in the same launch that computes `out`.  deform_attention_maps turns them into maps.  Detached; the fp32-grade cores only."""

    def __init__(self):
        self.logits = self.lse = None
        self.heads = self.groups = None


def _core_inputs(ctx, tensors, heads, groups, scale, dropout_p, dropout_seed, seed_offset, compute_dtype, fork, w2=None):
    """Prologue of a fused core's forward: the call's settings on ctx, the shape rules of every core -> (the contiguous tensors, m16).
    seed_offset: a device int64 [1] owned by this call (hipGraph replays: deform_attention)."""
    ctx.fork, ctx.seed_offset = fork, seed_offset
    tensors = tuple(_c(t) for t in tensors)
    _check_core(tensors[0], heads, w2)
    m16 = _dtype16(compute_dtype)
    ctx.cfg = (heads, groups, float(scale), float(dropout_p), int(dropout_seed), m16)
    return tensors, m16


def _core_outputs(ctx, q, heads: int, J: int, m16, scores=None):
    """out, lse and the score tiles (fp32; 16-bit core: fp16) - the tiles only where a backward or an AttnScores sink will read them (the
    entry points save the scores and their side tensor together or not at all)."""
    B, N, _ = q.shape
    out, lse = torch.empty_like(q), torch.empty(B, heads, N, device=q.device, dtype=torch.float32)
    keep = any(ctx.needs_input_grad) or scores is not None
    return out, lse, (_score_tiles(q, heads, J, torch.float32 if m16 is None else torch.float16) if keep else None)


def _core_done(ctx, inputs, out, lse, logits, side=(), scores=None, tap=None):
    """Epilogue of a fused core's forward: saves (*inputs, out, lse, logits, *side) for the backward, fills the AttnScores sink, appends
    the call's DECISION_TAP entry - the keys of every core plus `tap`, the core's own (tests/helpers.py reads them)."""
    ctx.save_for_backward(*inputs, out, lse, logits, *side)
    heads, groups = ctx.cfg[:2]
    if scores is not None:
        scores.logits, scores.lse, scores.heads, scores.groups = logits.detach(), lse.detach(), int(heads), int(groups)
    if DECISION_TAP is not None:
        q, k, _, vs, gq = inputs[:5]
        DECISION_TAP.append({"kind": "attn", "vs": vs.detach(), "gq": gq.detach(), "B": q.shape[0], "N": q.shape[1], "J": k.shape[1],
                             "heads": heads, "groups": groups, **tap})
    return out


def _core_backward(ctx, dout, logits, like, ws_keys: frozenset, dims: dict, ws_dtype=torch.float32):
    """The buffers of a fused core's backward: dout (contiguous), the d scores (the scores' shape; fp32, 16-bit core: bf16), one
    gradient per tensor of `like`, the workspace and its size in bytes - what the core's size function answers for `dims`."""
    dout = _c(dout)
    wsb = capi.call(core_entry_points(ctx.path, ctx.multi_head, ctx.cfg[5] is not None)[2], dims, ws_keys)
    dlogits = torch.empty(logits.shape, device=logits.device, dtype=torch.float32 if ctx.cfg[5] is None else torch.bfloat16)
    grads = tuple(torch.empty_like(t) for t in like)
    return dout, dlogits, grads, torch.empty(wsb if ws_dtype == torch.uint8 else (wsb + 3) // 4, device=dout.device, dtype=ws_dtype), wsb


def _grads(ctx, *grads):
    """A backward's return: the gradients of the leading inputs, None for the rest.  dq (the first) is also parked for the offsets
    network's backward (GradFork); it is still returned to autograd."""
    dq = grads[0]
    if ctx.fork is not None and ctx.needs_input_grad[0]:
        ctx.fork.dq = dq.view(dq.shape[0], dq.shape[1], -1)
    return grads + (None,) * (len(ctx.needs_input_grad) - len(grads))


# (the core deform_path names, multi-head, 16-bit) -> the stems of its forward's and its backward's entry point in include/smml.h ("smml_" +
# stem + "_fwd" / "_bwd", "_f32" behind the fp32-grade ones; stem + "_fwd" / "_bwd" is the capi.check name too), the TIMER events of the
# forward and of the bias backward.  No argument lists: a launch takes its arguments by name (capi.bind) from a namespace - see below.
_CORE_ENTRY = {
    ("pair", False, False): ("deform_attn", "deform_attn", "deform_attn_fwd", "cpb_bwd"),
    ("pair", False, True): ("deform_attn16", "deform_attn16", "deform16_fwd", "cpb16_bwd"),
    ("pair_table_forward", False, True): ("deform_attn_table", "deform_attn16", "deform_table_fwd", "cpb16_bwd"),
    ("pair_wide", False, False): ("deform_attn_wide", "deform_attn_wide", "deform_wide_fwd", "cpb_wide_bwd"),
    ("table", False, True): ("deform_attn_table", "deform_attn_table", "deform_table_fwd", "cpb_table_bwd"),
    ("region1d", False, False): ("deform_attn_region1d", "deform_attn_region1d", "deform_region1d_fwd", "cpb_region1d_bwd"),
    ("region", False, False): ("deform_attn_region", "deform_attn_region", "deform_region_fwd", "cpb_region_bwd"),
    ("region", False, True): ("deform_attn16_region", "deform_attn16_region", "deform16_region_fwd", "cpb16_region_bwd"),
    ("region", True, False): ("deform_attn_region_mh", "deform_attn_region_mh", "deform_region_mh_fwd", "cpb_region_mh_bwd"),
    ("region", True, True): ("deform_attn16_region_mh", "deform_attn16_region_mh", "deform16_region_mh_fwd", "cpb16_region_mh_bwd"),
}


# A namespace holds all the call has under include/smml.h's parameter names: a score-shaped tensor under each name a prototype gives it,
# None where the core has no use for a value.  The key sets (tests/test_named_launch.py holds them against the header):
_RUN = "scale dropout_p dropout_seed dtype ev_start ev_stop stream opts"
_MLP = "q k v vs gq w1 b1 w2 b2 w3 b3 tables out lse logits_t logits16 relu_masks region_ids B N J H G W posdim " + _RUN
_TABLE = "q k v vs gq table out lse logits16 B N J H G posdim table_g table_pmax " + _RUN
_BWD = " dout dq dk dv dvs workspace workspace_bytes "
MLP_WS_KEYS, TABLE_WS_KEYS = frozenset("B N J H G W".split()), frozenset("B N J H posdim".split())
MLP_FWD_KEYS = frozenset((_MLP + " table table_g table_pmax bias_t").split())
MLP_BWD_KEYS = frozenset((_MLP + _BWD + "dlogits_t dlogits16 dw1 db1 dw2 db2 dw3 db3").split())
TABLE_FWD_KEYS = frozenset(_TABLE.split())
TABLE_BWD_KEYS = frozenset((_TABLE + _BWD + "dlogits16 dtable grid_h grid_w").split())
BUILD_KEYS = frozenset("w1 b1 w2 b2 w3 b3 outputs pmax tables tables_bytes stream".split())
MASK_TABLE_KEYS = frozenset("w1 b1 w2 b2 table posdim pmax stream".split())
RELU1_KEYS = frozenset("vs gq w1 b1 masks B N J G posdim stream opts".split())
WIDE_DECISIONS_KEYS = RELU1_KEYS | {"w2", "b2", "W"}
DROPOUT_MASK_KEYS = frozenset("mask B N J H dropout_p dropout_seed stream opts".split())


def core_entry_points(path: str, multi_head: bool, m16: bool):
    """A core's forward, backward and backward-workspace-size function in include/smml.h (a 16-bit core shares its sibling's size)."""
    (fwd, bwd), f32 = _CORE_ENTRY[(path, multi_head, m16)][:2], "" if m16 else "_f32"
    return f"smml_{fwd}_fwd{f32}", f"smml_{bwd}_bwd{f32}", f"smml_{bwd.replace('attn16', 'attn')}_bwd_workspace_bytes"


def _launch(ctx, direction: str, keys: frozenset, ns: dict):
    """This call's launch in `direction` ('fwd' / 'bwd') from the namespace `ns`, plus the TIMER events and the stream."""
    core, bwd = (ctx.path, ctx.multi_head, ctx.cfg[5] is not None), direction == "bwd"
    ns["ev_start"], ns["ev_stop"], ns["stream"] = *TIMER.events(_CORE_ENTRY[core][2 + bwd], ns["B"] * ns["H"] * ns["N"] * ns["J"]), capi.stream()
    capi.check(capi.call(core_entry_points(*core)[bwd], ns, keys), f"{_CORE_ENTRY[core][bwd]}_{direction}")


_REGION_STREAMS = {}
REGION_PREFETCH = os.environ.get("SMML_REGION_PREFETCH", "1") != "0"


class RegionPrefetch:
    """Region tables being built on a side stream (they depend on the bias MLP's parameters only, not on the bag): started at the top of
    the module's forward, joined by the attention launch - the ~0.3 ms of the build run beside the projections, the offsets network and
    the sampler instead of in front of the attention kernel."""

    def __init__(self, w1, b1, w2, b2, w3, b3, pmax: float):
        dev = w1.device
        main = torch.cuda.current_stream(dev)
        key = dev.index if dev.index is not None else torch.cuda.current_device()
        side = _REGION_STREAMS.get(key)
        if side is None:
            side = _REGION_STREAMS[key] = torch.cuda.Stream(device=dev)
        self.pmax = float(pmax)
        self.params = tuple(t.data_ptr() for t in (w1, b1, w2, b2, w3, b3)) + tuple(t._version for t in (w1, b1, w2, b2, w3, b3))
        # allocated from the MAIN stream's pool (that is where it is used last and freed); the side stream starts behind everything the
        # main stream has queued so far, i.e. behind the previous owner of the block
        self.tables = torch.empty(capi.lib().smml_cpb_regions_bytes(), device=dev, dtype=torch.uint8)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            cpb_regions_build(w1.detach(), b1.detach(), w2.detach(), b2.detach(), w3.detach(), b3.detach(), pmax, self.tables)
            self.event = torch.cuda.Event()
            self.event.record(side)
        # a prefetch that is dropped without join() (the forward found other parameters or another square) frees the block on the main
        # stream while the side stream may still be writing it: the allocator must not hand it out before the side stream is done
        self.tables.record_stream(side)

    def matches(self, w1, b1, w2, b2, w3, b3, pmax: float) -> bool:
        return (self.pmax == float(pmax) and
                self.params == tuple(t.data_ptr() for t in (w1, b1, w2, b2, w3, b3)) + tuple(t._version for t in (w1, b1, w2, b2, w3, b3)))

    def join(self) -> torch.Tensor:
        torch.cuda.current_stream(self.tables.device).wait_event(self.event)
        return self.tables


def wide_decisions(vs, gq, w1, b1, w2, b2, *, B: int, N: int, J: int, groups: int, log_distance: bool = True):
    """Tests: the ReLU decisions of the wide position-bias MLP (width 64 / 128) exactly as its forward and backward take them
    (smml_deform_attn_wide_decisions) -> (m1, m2) bool [(B groups), N, J, W]: [x1 > 0], [x2 > 0] per pair and hidden channel."""
    W = w2.shape[0]
    words = torch.empty(B * groups, N, J, 2, W // 32, device=vs.device, dtype=torch.int32)
    vs, gq, w1, b1, w2, b2 = (_c(t.detach()) for t in (vs, gq, w1, b1, w2, b2))
    ns = dict(vs=vs, gq=gq, w1=w1, b1=b1, w2=w2, b2=b2, masks=words, B=B, N=N, J=J, G=groups, W=W, posdim=vs.shape[-1], stream=capi.stream(),
              opts=capi.deform_opts(None, log_distance))
    capi.check(capi.call("smml_deform_attn_wide_decisions", ns, WIDE_DECISIONS_KEYS), "deform_attn_wide_decisions")
    bits = ((words[..., None] >> torch.arange(32, device=vs.device, dtype=torch.int32)) & 1).bool()      # [..., 2, W / 32, 32]
    bits = bits.reshape(B * groups, N, J, 2, W)
    return bits[..., 0, :], bits[..., 1, :]


# ------------------------------------------------------------------------------------------------
# table mode of the 16-bit core: the position-bias MLP evaluated once per call on a grid, interpolated per pair (include/smml.h)
# ------------------------------------------------------------------------------------------------
_TABLE_POINTS = {}


def _table_points(points: int, posdim: int, pmax: float, device) -> torch.Tensor:
    """[points^posdim, posdim] grid of signed-log offsets, point (i0, i1) in row i1 * points + i0 (a constant per (pmax, device))."""
    key = (points, posdim, float(pmax), str(device))
    g = _TABLE_POINTS.get(key)
    if g is None:
        ax = (-pmax + torch.arange(points, dtype=torch.float64) * (2.0 * pmax / (points - 1))).float()
        if posdim == 2:
            g = torch.stack((ax.view(1, points).expand(points, points), ax.view(points, 1).expand(points, points)), dim=-1).reshape(-1, 2)
        else:
            g = ax.view(points, 1)
        if len(_TABLE_POINTS) > 16:
            _TABLE_POINTS.clear()
        g = _TABLE_POINTS[key] = g.contiguous().to(device)
    return g


def cpb_table_fn(w1, b1, w2, b2, w3, b3, *, posdim: int, pmax: float, device):
    """The position-bias MLP (DeformableAttention2D.py:129-152 / DeformableAttention1D.py:69-98, already log-transformed input) on the
    table grid: [heads // groups, points^posdim], fp32, three exact-fp32 GEMM launches; autograd carries d table back to the six tensors."""
    points = capi.lib().smml_deform_attn_table_points(posdim)
    pts = _table_points(points, posdim, pmax, device)
    h = linear(pts, w1, b1, act=ACT_RELU)
    h = linear(h, w2, b2, act=ACT_RELU)
    t = linear(h, w3, b3)                                   # [cells, o]
    return t.reshape(1, -1) if t.shape[1] == 1 else t.t().contiguous()


class _DeformAttnMLP(torch.autograd.Function):
    """The fused cores that differentiate the six tensors of the position-bias MLP; `path` is what deform_path answered:
    'pair'  the per-pair MLP (csrc/deform_attn.hip; with compute_dtype csrc/deform_attn16.hip), saving layer 2's ReLU decisions;
    'pair_table_forward'  (16-bit) the forward takes its bias from the table of half-width pmax, the backward takes layer 2's decisions
        from a mask table (or recomputes them per pair: TABLE_FORWARD_MASKS);
    'region' / 'region1d'  the bias per linear region (2-D, csrc/cpb_regions.h; fp32-grade or 16-bit core; multi_head: the "_mh" entry
        points of one or two heads per offset group) / per linear piece (1-D, csrc/cpb_regions1d.h; fp32-grade core), saving every pair's
        region id.  pmax: half-width of the tables' square / index grid (1-D; None: the span of the breakpoints); prefetch: a
        RegionPrefetch of the 2-D tables, if any;
    'pair_wide'  a bias MLP of width 64 / 128 (csrc/deform_attn_wide.hip; fp32-grade core): the forward evaluates the MLP once per pair
        into bias tiles and runs the attention kernel on them, the backward is the dq / dkv passes of the width-32 core followed by the
        wide bias backward, which recomputes the MLP - no ReLU mask is saved.  No host synchronisation and no float atomics: the call
        captures in a hipGraph as it stands and is run-to-run identical with or without functional.deterministic()."""

    @staticmethod
    def forward(ctx, q, k, v, vs, gq, w1, b1, w2, b2, w3, b3, path, heads, groups, scale, dropout_p, dropout_seed, seed_offset, compute_dtype,
                fork, log_distance, pmax, prefetch, multi_head, scores):
        ctx.path, ctx.multi_head, ctx.log_distance = path, bool(multi_head), bool(log_distance)
        wide, region = path == "pair_wide", path in ("region", "region1d")
        inputs, m16 = _core_inputs(ctx, (q, k, v, vs, gq, w1, b1, w2, b2, w3, b3), heads, groups, scale, dropout_p, dropout_seed, seed_offset,
                                   compute_dtype, fork, None if wide else w2)
        q, k, v, vs, gq, w1, b1, w2, b2, w3, b3 = inputs
        (B, N, _), J, posdim, W = q.shape, k.shape[1], vs.shape[-1], w2.shape[0]
        if wide and (tuple(w1.shape) != (W, posdim) or tuple(w3.shape) != (heads // groups, W) or tuple(b1.shape) != (W,)
                     or tuple(b2.shape) != (W,)):
            raise RuntimeError(f"the wide position-bias MLP is {posdim} -> {W} -> {W} -> heads // groups; got w1 {tuple(w1.shape)}, "
                               f"w3 {tuple(w3.shape)}")
        tables = table = bias = points = tpmax = None
        if path == "region1d":
            tables = cpb_regions1d_build(w1, b1, w2, b2, w3, b3, float(pmax or 0.0))
        elif region and prefetch is not None and prefetch.matches(w1, b1, w2, b2, w3, b3, pmax):
            tables = prefetch.join()                 # built beside the layers in front of the attention (RegionPrefetch)
        elif region:
            tables = cpb_regions_build(w1, b1, w2, b2, w3, b3, pmax)
        out, lse, logits = _core_outputs(ctx, q, heads, J, m16, scores)
        ctx.table_pmax = pmax if path == "pair_table_forward" else None
        ctx.export_masks = side = None               # side: the score-shaped tensor the core saves beside the scores
        if region and logits is not None:
            side = _score_tiles(q, heads, J, torch.int16)                     # the linear piece of every pair, per head
        elif path == "pair" and logits is not None:
            side = _score_tiles(q, heads, J, torch.int16, 2)                  # layer-2 ReLU decisions of the bias MLP (per lane half)
        elif wide and logits is None:
            # training: the bias tiles are built in logits_t and overwritten in place by the scores; inference: a scratch buffer of that size
            # (a call that hands out its scores takes the training form: the same launch, the scores kept)
            bias = _score_tiles(q, heads, J, torch.float32)
        elif path == "pair_table_forward":
            if logits is not None and DECISION_TAP is not None:               # tests: the backward writes the decisions it recomputed here
                ctx.export_masks = _score_tiles(q, heads, J, torch.int16, 2).zero_()
            with torch.no_grad():
                table = cpb_table_fn(w1, b1, w2, b2, w3, b3, posdim=posdim, pmax=pmax, device=q.device)
            points, tpmax = capi.lib().smml_deform_attn_table_points(posdim), float(pmax)
        _launch(ctx, "fwd", MLP_FWD_KEYS, dict(
            q=q, k=k, v=v, vs=vs, gq=gq, w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3, tables=tables, table=table, out=out, lse=lse,
            logits_t=logits, logits16=logits, relu_masks=side, region_ids=side, bias_t=bias, B=B, N=N, J=J, H=heads, G=groups, W=W,
            posdim=posdim, table_g=points, table_pmax=tpmax, scale=float(scale), dropout_p=float(dropout_p), dropout_seed=int(dropout_seed),
            dtype=m16 and m16[0], opts=capi.deform_opts(seed_offset, ctx.log_distance, region_lds_cap=REGION_LDS_CAP if region else 0)))
        tap = None
        if DECISION_TAP is not None and region:
            # the 1-D ids index the piece tables (region1d_tables_view), not the 2-D region tables: keys of their own
            ids, tabs = ("region1d_ids", "region1d_tables") if path == "region1d" else ("region_ids", "tables")
            tap = {"w1": w1.detach(), "b1": b1.detach(), "w2": w2.detach(), "b2": b2.detach(), "masks2": None, ids: side, tabs: tables,
                   "table_pmax": None, "log_distance": True}
        elif DECISION_TAP is not None and wide:
            m1, m2 = wide_decisions(vs, gq, w1, b1, w2, b2, B=B, N=N, J=J, groups=groups, log_distance=ctx.log_distance)
            tap = {"wide": W, "masks1": m1, "masks2": m2, "log_distance": ctx.log_distance}
        elif DECISION_TAP is not None:
            tap = {"w1": w1.detach(), "b1": b1.detach(), "masks2": side if path == "pair" else ctx.export_masks, "table_pmax": ctx.table_pmax,
                   "log_distance": ctx.log_distance}
        return _core_done(ctx, inputs, out, lse, logits, (side, tables), scores, tap)

    @staticmethod
    def backward(ctx, dout):
        q, k, v, vs, gq, w1, b1, w2, b2, w3, b3, out, lse, logits, side, tables = ctx.saved_tensors
        heads, groups, scale, dropout_p, dropout_seed, m16 = ctx.cfg
        (B, N, _), J, posdim, W = q.shape, k.shape[1], vs.shape[-1], w2.shape[0]
        path, region = ctx.path, ctx.path in ("region", "region1d")
        dout, dlogits, (dq, dk, dv, dvs, dw1, db1, dw2, db2, dw3, db3), ws, wsb = _core_backward(
            ctx, dout, logits, (q, k, v, vs, w1, b1, w2, b2, w3, b3), MLP_WS_KEYS, dict(B=B, N=N, J=J, H=heads, G=groups, W=W),
            torch.uint8 if region else torch.float32)
        opts = capi.deform_opts(ctx.seed_offset, ctx.log_distance, region_lds_cap=REGION_LDS_CAP if region else 0)
        if path in ("pair", "pair_table_forward") and m16 is not None:
            mtab = None
            if path == "pair_table_forward" and TABLE_FORWARD_MASKS == "table":
                # layer-2 decisions from a mask table (include/smml.h) built from the current weights - one small launch
                cells = capi.lib().smml_cpb_mask_table_cells(posdim)
                mtab = torch.empty(cells ** posdim, device=q.device, dtype=torch.int32)
                ns = dict(w1=w1, b1=b1, w2=w2, b2=b2, table=mtab, posdim=posdim, pmax=float(ctx.table_pmax), stream=capi.stream())
                capi.check(capi.call("smml_cpb_mask_table", ns, MASK_TABLE_KEYS), "cpb_mask_table")
            opts = capi.deform_opts(ctx.seed_offset, ctx.log_distance, mtab, float(ctx.table_pmax or 0.0), ctx.export_masks)
        _launch(ctx, "bwd", MLP_BWD_KEYS, dict(
            q=q, k=k, v=v, vs=vs, gq=gq, w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3, tables=tables, out=out, dout=dout, lse=lse,
            logits_t=logits, logits16=logits, relu_masks=side, region_ids=side, dlogits_t=dlogits, dlogits16=dlogits, dq=dq, dk=dk, dv=dv,
            dvs=dvs, dw1=dw1, db1=db1, dw2=dw2, db2=db2, dw3=dw3, db3=db3, workspace=ws, workspace_bytes=wsb, B=B, N=N, J=J, H=heads,
            G=groups, W=W, posdim=posdim, scale=scale, dropout_p=dropout_p, dropout_seed=dropout_seed, dtype=m16 and m16[0], opts=opts))
        return _grads(ctx, dq, dk, dv, dvs, None, dw1, db1, dw2, db2, dw3, db3)


class _DeformAttnTable(torch.autograd.Function):
    """The 16-bit core with the position bias interpolated from `table` (include/smml.h, table mode); differentiates the table, which
    cpb_table_fn carries back to the MLP."""

    @staticmethod
    def forward(ctx, q, k, v, vs, gq, table, heads, groups, scale, dropout_p, dropout_seed, seed_offset, compute_dtype, fork, pmax, grid):
        ctx.path, ctx.multi_head = "table", False
        inputs, m16 = _core_inputs(ctx, (q, k, v, vs, gq, table), heads, groups, scale, dropout_p, dropout_seed, seed_offset, compute_dtype, fork)
        q, k, v, vs, gq, table = inputs
        (B, N, _), J, posdim = q.shape, k.shape[1], vs.shape[-1]
        points = capi.lib().smml_deform_attn_table_points(posdim)
        if tuple(table.shape) != (heads // groups, points ** posdim):
            raise RuntimeError(f"table must be [{heads // groups}, {points ** posdim}] (got {tuple(table.shape)})")
        grid_h, grid_w = (int(x) for x in grid) if grid else (0, 0)
        ctx.table = dict(table_g=points, table_pmax=float(pmax), grid_h=grid_h, grid_w=grid_w)
        out, lse, logits = _core_outputs(ctx, q, heads, J, m16)
        _launch(ctx, "fwd", TABLE_FWD_KEYS, dict(
            q=q, k=k, v=v, vs=vs, gq=gq, table=table, out=out, lse=lse, logits16=logits, B=B, N=N, J=J, H=heads, G=groups, posdim=posdim,
            table_g=points, table_pmax=float(pmax), scale=float(scale), dropout_p=float(dropout_p), dropout_seed=int(dropout_seed),
            dtype=m16[0], opts=capi.deform_opts(seed_offset)))
        # no per-pair ReLU decisions in this mode: the MLP runs on grid points only
        return _core_done(ctx, inputs, out, lse, logits, tap={"masks2": None, "table_pmax": float(pmax)})

    @staticmethod
    def backward(ctx, dout):
        q, k, v, vs, gq, table, out, lse, logits = ctx.saved_tensors
        heads, groups, scale, dropout_p, dropout_seed, m16 = ctx.cfg
        (B, N, _), J, posdim = q.shape, k.shape[1], vs.shape[-1]
        dout, dlogits, (dq, dk, dv, dvs, dtable), ws, wsb = _core_backward(ctx, dout, logits, (q, k, v, vs, table), TABLE_WS_KEYS,
                                                                           dict(B=B, N=N, J=J, H=heads, posdim=posdim))
        _launch(ctx, "bwd", TABLE_BWD_KEYS, dict(
            ctx.table, q=q, k=k, v=v, vs=vs, gq=gq, table=table, out=out, dout=dout, lse=lse, logits16=logits, dlogits16=dlogits, dq=dq,
            dk=dk, dv=dv, dvs=dvs, dtable=dtable, workspace=ws, workspace_bytes=wsb, B=B, N=N, J=J, H=heads, G=groups, posdim=posdim,
            scale=scale, dropout_p=dropout_p, dropout_seed=dropout_seed, dtype=m16[0], opts=capi.deform_opts(ctx.seed_offset)))
        return _grads(ctx, dq, dk, dv, dvs, None, dtable)


def table_pmax(gq_bound: float, vs_bound: float) -> float:
    """Half-width of the table in signed-log units for |gq| <= gq_bound, |vs| <= vs_bound (positions beyond it take the edge value)."""
    return float(math.log1p(gq_bound + vs_bound) * 1.0001)


_REPLAY_COUNTER = {}         # device index -> int64 [1]: bumped once per dropout call inside a captured graph


def graph_seed_offset(device, allocate_only: bool = False):
    """The per-call seed offset of a dropout launch that is being captured in a hipGraph: a device-resident counter is bumped and
    copied (both operations are part of the graph), so every replay - and every call within a replay - draws a new mask while the
    forward and the backward of one call read the same value.  The counter itself must exist before the capture starts (it would
    otherwise live in the graph's private pool and be re-zeroed by every replay): any eager dropout call on the device creates it."""
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    ctr = _REPLAY_COUNTER.get(key)
    capturing = torch.cuda.is_current_stream_capturing()
    if ctr is None:
        if capturing:
            raise RuntimeError("run one eager training step before capturing it in a graph (the dropout replay counter is created "
                               "by the first eager call)")
        ctr = _REPLAY_COUNTER[key] = torch.zeros(1, device=dev, dtype=torch.int64)
    if allocate_only or not capturing:
        return None
    ctr.add_(1)
    return ctr.clone()


def deform_attention(q, k, v, vs, gq, w1, b1, w2, b2, w3, b3, *, heads: int, groups: int, scale: float,
                     dropout_p: float = 0.0, dropout_seed: int = 0, dropout_seed_offset=None, compute_dtype=None, fork=None,
                     cpb_table: bool = False, cpb_table_pmax=None, cpb_table_grid=None, log_distance: bool = True,
                     cpb_regions=None, cpb_region_pmax=None, cpb_region_prefetch=None, cpb_regions_multi_head: bool = False,
                     attn_scores: Optional["AttnScores"] = None):
    """dropout(softmax(scale q k^T + CPB(gq - vs))) v.  q [B, N, H*64], k/v [B, J, H*64], vs [(B G), J, P], gq [N, P].
    dropout_p > 0 applies nn.Dropout semantics to the probabilities with a counter-based mask from dropout_seed
    (+ the value of the device tensor dropout_seed_offset at run time, see graph_seed_offset).
    compute_dtype None: fp32-grade split products (csrc/deform_attn.hip); 'bf16' / 'fp16': the 16-bit compute mode
    (csrc/deform_attn16.hip: single-term 16-bit MFMA operands, 16-bit score storage; inputs, outputs and gradients stay fp32).
    log_distance False (1-D positions only): the bias MLP reads the raw offset gq - vs (DeformableAttention1D.py:92, cpb_log_distance=False).
    cpb_table (with a 16-bit compute_dtype): True / 'full' - the position-bias MLP is evaluated once on a grid and interpolated per pair,
    forward and backward (include/smml.h, "table mode": approximate parameter gradients); 'forward' - only the forward takes its bias from the
    table (|error| <= ~1e-3 of the bias range, below the 16-bit operand rounding), the backward differentiates the per-pair MLP itself, recomputing
    layer 2 (parity-grade gradients at the 16-bit mode's tolerances); cpb_table_pmax = half-width of the grid in signed-log units (table_pmax(); None: taken from the data, one host sync);
    cpb_table_grid = (rows, cols) asserts that the queries sit on a regular grid, gq[y * cols + x] = (X[x], Y[y]) - the backward then
    builds d table on the matrix pipe instead of with LDS atomics.
    cpb_regions True with 1-D positions: the position bias per linear piece of its MLP (csrc/cpb_regions1d.h; signed-log offsets, the
    fp32-grade core, heads // groups in {1, 2}; anything else raises), cpb_region_pmax = half-width of its index grid (None: the span of
    the breakpoints; no host sync either way).
    cpb_regions_multi_head True with 2-D positions: the position bias per linear region also for two heads per offset group (w3 [2, 32];
    include/smml.h "_mh" entry points; signed-log offsets, either compute mode, no table mode; anything else raises).
    w2 of shape (64, 64) / (128, 128) (dim = 256 / 512 of the modules): the wide family (csrc/deform_attn_wide.hip) - the per-pair MLP in exact
    fp32, fp32-grade core, one or two heads per group, all three position forms; compute_dtype, cpb_table, cpb_regions and
    cpb_regions_multi_head raise ValueError there.
    attn_scores (an AttnScores, default None: nothing changes): the call also keeps the score tiles and lse its forward writes - with or
    without grad mode, in the one fused launch - and hands them out there for deform_attention_maps.  The fp32-grade cores only:
    compute_dtype (2-byte score tiles) and cpb_table raise ValueError."""
    if attn_scores is not None:
        if cpb_table:
            raise ValueError(f"cpb_table={cpb_table!r}: attention maps (attn_scores) are built for the fp32-grade cores, not for the table modes")
        if compute_dtype is not None:
            raise ValueError(f"compute_dtype={compute_dtype!r}: attention maps (attn_scores) are built for the fp32-grade cores, whose score tiles "
                             "are fp32; the 16-bit compute modes save 2-byte tiles")
        if not isinstance(attn_scores, AttnScores):
            raise TypeError("attn_scores must be a functional.AttnScores")
    mh = bool(cpb_regions_multi_head) and vs.shape[-1] == 2
    path = deform_path(posdim=vs.shape[-1], heads=heads, groups=groups, keys=k.shape[1], w2_shape=w2.shape, w3_shape=w3.shape,
                       log_distance=log_distance, compute_dtype=compute_dtype, cpb_table=cpb_table, cpb_regions=cpb_regions,
                       region_pmax_given=cpb_region_pmax is not None,
                       capturing=cpb_region_pmax is None and q.is_cuda and torch.cuda.is_current_stream_capturing(),
                       regions_multi_head=mh)
    # the half-width the core's tables need, if it has any (width 64 / 128: the region tables, their prefetch and pmax are not consulted)
    pmax = {"region": cpb_region_pmax, "region1d": cpb_region_pmax, "pair_table_forward": cpb_table_pmax, "table": cpb_table_pmax}.get(path)
    if pmax is None and path in ("region", "pair_table_forward", "table"):      # from the data: one host sync
        pmax = table_pmax(float(gq.detach().abs().max()), float(vs.detach().abs().max()))
    if path == "table":
        table = cpb_table_fn(w1, b1, w2, b2, w3, b3, posdim=vs.shape[-1], pmax=pmax, device=q.device)
        return _DeformAttnTable.apply(q, k, v, vs, gq, table, heads, groups, scale, dropout_p, dropout_seed, dropout_seed_offset,
                                      compute_dtype, fork, pmax, cpb_table_grid)
    return _DeformAttnMLP.apply(q, k, v, vs, gq, w1, b1, w2, b2, w3, b3, path, heads, groups, scale, dropout_p, dropout_seed, dropout_seed_offset,
                                compute_dtype, fork, log_distance, pmax, cpb_region_prefetch if path == "region" else None, mh, attn_scores)


def deform_attention_dropout_mask(B: int, N: int, J: int, H: int, dropout_p: float, dropout_seed: int, device, seed_offset=None):
    """The keep mask (0 / 1) [B, H, N, J] a launch with this (p, seed[, device-resident replay offset]) applies; tests only."""
    mask = torch.empty(B, H, N, J, device=device, dtype=torch.float32)
    ns = dict(mask=mask, B=B, N=N, J=J, H=H, dropout_p=float(dropout_p), dropout_seed=int(dropout_seed), stream=capi.stream(),
              opts=capi.deform_opts(seed_offset))
    capi.check(capi.call("smml_deform_attn_dropout_mask_f32", ns, DROPOUT_MASK_KEYS), "dropout_mask")
    return mask


def deform_attention_maps(sink_or_scores, vs=None, *, heads: int, groups: int, grid_hw=None, dense: bool = False):
    """Where a deform_attention call looked, from the scores it saved (include/smml.h, smml_attn_maps_f32 / smml_attn_splat_f32).
    sink_or_scores: the AttnScores the call filled, or (logits_t, lse).  The probabilities are the softmax BEFORE dropout.  Returns a dict of
    detached tensors:
      key_mass  [B, H, J]        the share of the bag's attention each sampled key receives (rows sum to 1)
      patch_map [B, G, Hh, Ww]   with 2-D sample positions vs [(B G), J, 2] and grid_hw = (Hh, Ww): the group's mean mass distributed to the
                                 patch grid with the sampler's corner weights and masks (mass outside the map is dropped: sums to <= 1)
      attn      [B, H, N, J]     with dense=True: the probabilities themselves (B H N J floats - small bags and tests)
    No host synchronisation (captures in a hipGraph), no autograd, no float atomics: run-to-run identical."""
    logits, lse = (sink_or_scores.logits, sink_or_scores.lse) if isinstance(sink_or_scores, AttnScores) else sink_or_scores
    if logits is None or lse is None:
        raise ValueError("no scores: pass the AttnScores a deform_attention(..., attn_scores=...) call filled, or (logits_t, lse)")
    if logits.dtype != torch.float32:
        raise ValueError(f"attention maps read the fp32 score tiles of the fp32-grade cores; got {logits.dtype} tiles (compute_dtype: the 16-bit "
                         "compute modes are not supported)")
    B, H, N = lse.shape
    J = logits.shape[3]
    if H != heads or heads % groups or tuple(logits.shape) != (B, H, capi.lib().smml_deform_attn_nst(N) // 32, J, 32):
        raise ValueError(f"scores of shape {tuple(logits.shape)} / lse {tuple(lse.shape)} do not belong to a call with heads {heads}, groups {groups}")
    L = capi.lib()
    with torch.no_grad():
        logits, lse = _c(logits.detach()), _c(lse.detach())
        key_mass = torch.empty(B, H, J, device=lse.device, dtype=torch.float32)
        attn = torch.empty(B, H, N, J, device=lse.device, dtype=torch.float32) if dense else None
        wsb = L.smml_attn_maps_workspace_bytes(B, N, J, H)
        ws = torch.empty((wsb + 3) // 4, device=lse.device, dtype=torch.float32)
        capi.check(L.smml_attn_maps_f32(capi.fptr(logits), capi.fptr(lse), capi.fptr(key_mass), capi.fptr(attn), capi.fptr(ws), wsb, B, N, J, H,
                                        capi.stream()), "attn_maps")
        res = {"key_mass": key_mass}
        if grid_hw is not None and vs is not None and vs.shape[-1] == 2:
            Hh, Ww = int(grid_hw[0]), int(grid_hw[1])
            vsc = _c(vs.detach())
            if tuple(vsc.shape) != (B * groups, J, 2):
                raise ValueError(f"vs of shape {tuple(vsc.shape)}: expected {(B * groups, J, 2)}")
            patch_map = torch.empty(B, groups, Hh, Ww, device=lse.device, dtype=torch.float32)
            capi.check(L.smml_attn_splat_f32(capi.fptr(key_mass), capi.fptr(vsc), capi.fptr(patch_map), B, H, groups, J, Hh, Ww, capi.stream()),
                       "attn_splat")
            res["patch_map"] = patch_map
        if dense:
            res["attn"] = attn
    return res


# ------------------------------------------------------------------------------------------------
# token mean / token tile / Gram matrices (Pooler, omic tiling, BatchLoss)
# ------------------------------------------------------------------------------------------------
class _TokenMean(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        ctx.n = x.shape[1]
        return colsum(x, 1.0 / x.shape[1], det=DETERMINISTIC)

    @staticmethod
    def backward(ctx, dy):
        return (dy / ctx.n).unsqueeze(1).expand(-1, ctx.n, -1).contiguous()


def token_mean(x):
    """x [B, n, C] -> mean over tokens [B, C]."""
    return _TokenMean.apply(x)


class _TileTokens(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, n):
        ctx.det = DETERMINISTIC
        # the broadcast view, not a copy (41 MB per 8-bag step that BatchLoss never reads: it takes _smml_compact): equal values; whoever
        # needs the rows in memory (reshape, .contiguous(), a kernel's _c) materialises them then
        return v.unsqueeze(1).expand(-1, n, -1)

    @staticmethod
    def backward(ctx, dy):
        return colsum(_c(dy), det=ctx.det), None


def tile_tokens(v, n: int):
    """v [B, C] -> [B, n, C] (values of v.unsqueeze(1).repeat(1, n, 1), as a broadcast view); backward is a column sum.
    The result carries the un-tiled vector as `_smml_compact`: BatchLoss uses it to gather [B, C] instead of the
    n-times larger tile across ranks (the Gram of a tile is n x the Gram of the vector, and the row normalisation
    that follows cancels the factor)."""
    out = _TileTokens.apply(v, n)
    out._smml_compact = v
    return out


class _Gram(torch.autograd.Function):
    """x [nb, R, K] -> x x^T [nb, R, R]: skinny, HBM-bound (K up to N*C = 1.28 M): split-K over the long axis."""

    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        nb, R, K = x.shape
        det = DETERMINISTIC                        # the forward VALUE is a split-K sum; the backward product is not split
        g = (torch.empty if det else torch.zeros)(nb, R, R, device=x.device, dtype=torch.float32)
        splitk = int(max(1, min((K + 255) // 256, 1024 // max(nb, 1), 65535 // nb)))   # R x R outputs: the K axis is all there is to spread
        _gemm(x, x, g, M=R, N=R, K=K, sam=K, sak=1, sbk=1, sbn=K, ldc=R, nb0=nb, sa0=R * K, sb0=R * K, sc0=R * R,
              splitk=splitk, det=det)
        ctx.save_for_backward(x)
        return g

    @staticmethod
    def backward(ctx, dg):
        (x,) = ctx.saved_tensors
        nb, R, K = x.shape
        s = _c(dg + dg.transpose(1, 2))
        dx = torch.empty_like(x)
        _gemm(s, x, dx, M=R, N=K, K=R, sam=R, sak=1, sbk=K, sbn=1, ldc=K, nb0=nb, sa0=R * R, sb0=R * K, sc0=R * K)
        return dx


def gram(x):
    return _Gram.apply(x)


class _BatchLossTail(torch.autograd.Function):
    """(go / ||go||_row - mean_g gv[g] / ||gv[g]||_row)^2 / n on [R, R] matrices (utils/loss.py:26-40): one launch per direction."""

    @staticmethod
    def forward(ctx, go, gv, n_total):
        go, gv = _c(go), _c(gv)
        R, nv = go.shape[-1], gv.shape[0]
        out = torch.empty(R, R, device=go.device, dtype=torch.float32)
        capi.check(capi.lib().smml_batchloss_tail_f32(capi.fptr(go), capi.fptr(gv), None, capi.fptr(out), None, None, R, nv, float(n_total),
                                                      capi.stream()), "batchloss_tail")
        ctx.n_total = float(n_total)
        ctx.save_for_backward(go, gv)
        return out

    @staticmethod
    def backward(ctx, dl):
        go, gv = ctx.saved_tensors
        R, nv = go.shape[-1], gv.shape[0]
        dgo, dgv = torch.empty_like(go), torch.empty_like(gv)
        capi.check(capi.lib().smml_batchloss_tail_f32(capi.fptr(go), capi.fptr(gv), capi.fptr(_c(dl)), None, capi.fptr(dgo), capi.fptr(dgv), R, nv,
                                                      ctx.n_total, capi.stream()), "batchloss_tail_bwd")
        return dgo, dgv, None


def batchloss_tail(go, gv, n_total):
    """go [R, R] (Gram of the omic rows), gv [nv, R, R] (Grams of the vgrid groups) -> the BatchLoss matrix [R, R]."""
    return _BatchLossTail.apply(go, gv, n_total)


# ------------------------------------------------------------------------------------------------
# generic batched product on the matrix cores: C = alpha * op(A) @ op(B) + beta * R
# (Nystrom sims / landmark products / pinv iteration, co-attention)
# ------------------------------------------------------------------------------------------------
def _op_view(T, trans):
    """(rows, cols, row stride, col stride, batch strides) of op(T) for a contiguous [t0, t1, r, c] tensor."""
    t0, t1, r, c = T.shape
    s0 = t1 * r * c if t0 > 1 else 0
    s1 = r * c if t1 > 1 else 0
    return (c, r, 1, c, s0, s1) if trans else (r, c, c, 1, s0, s1)


class _MatMul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, R, ta, tb, alpha, beta, merged):
        A, B = _c(A), _c(B)
        M, K, sam, sak, sa0, sa1 = _op_view(A, ta)
        K2, N, sbk, sbn, sb0, sb1 = _op_view(B, tb)
        if K != K2:
            raise RuntimeError(f"matmul4: inner dimensions differ ({K} vs {K2})")
        nb0, nb1 = max(A.shape[0], B.shape[0]), max(A.shape[1], B.shape[1])
        if merged:
            Cm = torch.empty(nb0, M, nb1 * N, device=A.device, dtype=torch.float32)
            ldc, sc0, sc1 = nb1 * N, M * nb1 * N, N
        else:
            Cm = torch.empty(nb0, nb1, M, N, device=A.device, dtype=torch.float32)
            ldc, sc0, sc1 = N, nb1 * M * N, M * N
        Rc = None
        if R is not None:
            Rc = _c(R)
            if Rc.shape != Cm.shape:
                raise RuntimeError("matmul4: residual must have the output's shape")
        # few output tiles and a long reduction (attn3 @ v: 256 x 64 outputs over n' keys): the K range is cut into S slices
        # that run as an extra batch dimension into a partial-sum buffer, added up in a fixed order afterwards (no atomics:
        # identical inputs give bit-identical outputs)
        nbt = nb0 * nb1
        full = (A.shape[0] == nb0 and A.shape[1] == nb1 and B.shape[0] == nb0 and B.shape[1] == nb1)
        S = _splitk_for(M, N, K, nbt) if (Rc is None and not merged and full and K >= 1024) else 1
        while S > 1 and (K % S or (K // S) % 4):
            S -= 1
        if S > 1:
            Kc = K // S
            part = torch.empty(S, nb0, nb1, M, N, device=A.device, dtype=torch.float32)
            _gemm(A, B, part, M=M, N=N, K=Kc, sam=sam, sak=sak, sbk=sbk, sbn=sbn, ldc=N, nb0=nbt, nb1=S,
                  sa0=A.shape[2] * A.shape[3], sa1=Kc * sak, sb0=B.shape[2] * B.shape[3], sb1=Kc * sbk,
                  sc0=M * N, sc1=nbt * M * N, alpha=alpha)
            torch.sum(part, dim=0, out=Cm)
        else:
            _gemm(A, B, Cm, M=M, N=N, K=K, sam=sam, sak=sak, sbk=sbk, sbn=sbn, ldc=ldc, residual=Rc, ldr=ldc, nb0=nb0,
                  nb1=nb1, sa0=sa0, sa1=sa1, sb0=sb0, sb1=sb1, sc0=sc0, sc1=sc1, alpha=alpha, beta=beta)
        ctx.cfg = (ta, tb, float(alpha), float(beta), merged, nb0, nb1, M, N, K, R is not None)
        ctx.det = DETERMINISTIC
        ctx.save_for_backward(A, B)
        return Cm

    @staticmethod
    def backward(ctx, dC):
        A, B = ctx.saved_tensors
        ta, tb, alpha, beta, merged, nb0, nb1, M, N, K, has_r = ctx.cfg
        dC = _c(dC)
        if merged:
            ldc, sc0, sc1 = nb1 * N, M * nb1 * N, N
        else:
            ldc, sc0, sc1 = N, nb1 * M * N, M * N
        _, _, a_sr, a_sc, sa0, sa1 = _op_view(A, ta)       # strides of op(A)[m, k]
        _, _, b_sr, b_sc, sb0, sb1 = _op_view(B, tb)       # strides of op(B)[k, n]
        dA = dB = dR = None

        def run(like, Mx, Nx, Kx, Xa, xa, Xb, xb, ld_out, bcast):
            nb = nb0 * nb1
            splitk = _splitk_for(Mx, Nx, Kx, nb)
            acc = 1 if (bcast or splitk > 1) else 0
            out = torch.zeros_like(like) if (acc and not ctx.det) else torch.empty_like(like)   # zero-fill only what atomics accumulate into
            _gemm(Xa, Xb, out, M=Mx, N=Nx, K=Kx, sam=xa[0], sak=xa[1], sbk=xb[0], sbn=xb[1], ldc=ld_out, nb0=nb0, nb1=nb1,
                  sa0=xa[2], sa1=xa[3], sb0=xb[2], sb1=xb[3],
                  sc0=(out.shape[1] * out.shape[2] * out.shape[3] if out.shape[0] > 1 else 0),
                  sc1=(out.shape[2] * out.shape[3] if out.shape[1] > 1 else 0), alpha=alpha, splitk=splitk,
                  accumulate=acc, det=ctx.det)
            return out

        if ctx.needs_input_grad[0]:
            bcast = (A.shape[0] < nb0) or (A.shape[1] < nb1)
            if not ta:   # dA[m, k] = sum_n dC[m, n] opB[k, n]
                dA = run(A, M, K, N, dC, (ldc, 1, sc0, sc1), B, (b_sc, b_sr, sb0, sb1), A.shape[3], bcast)
            else:        # A stored [K, M]: dA[k, m] = sum_n opB[k, n] dC[m, n]
                dA = run(A, K, M, N, B, (b_sr, b_sc, sb0, sb1), dC, (1, ldc, sc0, sc1), A.shape[3], bcast)
        if ctx.needs_input_grad[1]:
            bcast = (B.shape[0] < nb0) or (B.shape[1] < nb1)
            if not tb:   # B stored [K, N]: dB[k, n] = sum_m opA[m, k] dC[m, n]
                dB = run(B, K, N, M, A, (a_sc, a_sr, sa0, sa1), dC, (ldc, 1, sc0, sc1), B.shape[3], bcast)
            else:        # B stored [N, K]: dB[n, k] = sum_m dC[m, n] opA[m, k]
                dB = run(B, N, K, M, dC, (1, ldc, sc0, sc1), A, (a_sr, a_sc, sa0, sa1), B.shape[3], bcast)
        if has_r and ctx.needs_input_grad[2]:
            dR = dC * beta if beta != 1.0 else dC
        return dA, dB, dR, None, None, None, None, None


def matmul4(A, B, R=None, *, ta=False, tb=False, alpha=1.0, beta=1.0, merged=False):
    """alpha * op(A) @ op(B) + beta * R for [nb0, nb1, rows, cols] tensors (size-1 batch dims broadcast);
    merged=True lays the result out as [nb0, M, nb1 * N] (heads merged)."""
    return _MatMul.apply(A, B, R, ta, tb, alpha, beta, merged)


class gemm_precision:
    """with gemm_precision(3): ...  - every tiled product launched inside runs with single-term bf16 operands (fp32 storage and
    accumulation); 2 = three-term split (fp32-grade); 0 restores the automatic choice.  Kernel selection happens on the host at
    launch time, so the switch covers exactly the launches issued inside the block (linear(..., prec=mode) re-enters it in its
    backward, so that the gradient products use the same operand precision as the forward one)."""

    def __init__(self, mode: int):
        self.mode = int(mode)

    def __enter__(self):
        L = capi.lib()
        self.prev = L.smml_gemm_get_mode()
        L.smml_gemm_set_mode(self.mode)
        return self

    def __exit__(self, *a):
        capi.lib().smml_gemm_set_mode(self.prev)


class _Attention16(torch.autograd.Function):
    """softmax(scale q k^T) v (+ residual) on the 16-bit matrix pipe, fp32 storage (csrc/attn16.hip)."""

    @staticmethod
    def forward(ctx, q, k, v, residual, scale, fp16, merged):
        q, k, v = _c(q), _c(k), _c(v)
        Bn, H, Lq, D = q.shape
        Lk = k.shape[2]
        if D != 64 or k.shape != (Bn, H, Lk, D) or v.shape != (Bn, H, Lk, D):
            raise RuntimeError("attention16: q [B, h, Lq, 64], k / v [B, h, Lk, 64] expected")
        if residual is not None:
            if not merged or tuple(residual.shape) != (Bn, Lq, H * D):
                raise RuntimeError("attention16: the residual is added in the heads-merged layout [B, Lq, h * 64]")
            out = _c(residual).clone()
        else:
            out = torch.empty((Bn, Lq, H * D) if merged else (Bn, H, Lq, D), device=q.device, dtype=torch.float32)
        lse2 = torch.empty(Bn * H, Lq, device=q.device, dtype=torch.float32)
        L = capi.lib()
        wsb = L.smml_attn16_fwd_workspace_bytes(Bn * H, Lq, Lk)
        ws = torch.empty((wsb + 3) // 4, device=q.device, dtype=torch.float32) if wsb else None
        capi.check(L.smml_attn16_fwd_f32(capi.fptr(q), capi.fptr(k), capi.fptr(v), capi.fptr(out), capi.fptr(lse2), capi.fptr(ws), wsb,
                                         Bn * H, Lq, Lk, D, float(scale), int(bool(fp16)), H if merged else 0,
                                         1 if residual is not None else 0, capi.stream()), "attn16_fwd")
        ctx.cfg = (float(scale), int(bool(fp16)), H if merged else 0, residual is not None)
        ctx.save_for_backward(q, k, v, out, lse2, _c(residual) if residual is not None else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse2, residual = ctx.saved_tensors
        scale, fp16, merged, has_res = ctx.cfg
        Bn, H, Lq, D = q.shape
        Lk = k.shape[2]
        dout = _c(dout)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        L = capi.lib()
        wsb = L.smml_attn16_bwd_workspace_bytes(Bn * H, Lq, Lk)
        ws = torch.empty((wsb + 3) // 4, device=q.device, dtype=torch.float32)
        capi.check(L.smml_attn16_bwd_f32(capi.fptr(q), capi.fptr(k), capi.fptr(v), capi.fptr(out), capi.fptr(residual), capi.fptr(dout),
                                         capi.fptr(lse2), capi.fptr(dq), capi.fptr(dk), capi.fptr(dv), capi.fptr(ws), wsb, Bn * H, Lq, Lk,
                                         D, scale, fp16, merged, capi.stream()), "attn16_bwd")
        return dq, dk, dv, (dout if has_res else None), None, None, None


def attention16(q, k, v, *, scale: float, fp16: bool = False, merged: bool = False, residual=None):
    """softmax(scale q k^T) v for q [B, h, Lq, 64], k / v [B, h, Lk, 64] with bf16 (or fp16) matrix-pipe operands and fp32
    accumulation; no [Lq, Lk] matrix is materialised.  merged=True returns [B, Lq, h * 64]; `residual` (that layout) is added."""
    return _Attention16.apply(q, k, v, residual, scale, fp16, merged)


class _SoftmaxRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        L = x.shape[-1]
        y = torch.empty_like(x)
        capi.check(capi.lib().smml_softmax_fwd_f32(capi.fptr(x), capi.fptr(y), x.numel() // L, L, capi.stream()), "softmax_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        L = y.shape[-1]
        dx = torch.empty_like(y)
        capi.check(capi.lib().smml_softmax_bwd_f32(capi.fptr(y), capi.fptr(_c(dy)), capi.fptr(dx), y.numel() // L, L,
                                                   capi.stream()), "softmax_bwd")
        return dx


def softmax_rows(x):
    return _SoftmaxRows.apply(x)


class _SegmentMean(torch.autograd.Function):
    """x [..., n, d] -> mean over l consecutive tokens -> [..., n / l, d]."""

    @staticmethod
    def forward(ctx, x, l):
        x = _c(x)
        n, d = x.shape[-2:]
        lead = x.numel() // (n * d)
        m = n // l
        ctx.l = l
        ctx.shape = x.shape
        return colsum(x.view(lead * m, l, d), 1.0 / l, det=DETERMINISTIC).view(*x.shape[:-2], m, d)

    @staticmethod
    def backward(ctx, dy):
        dy = _c(dy)
        d = dy.shape[-1]
        nb = dy.numel() // d
        dx = torch.empty(ctx.shape, device=dy.device, dtype=torch.float32)
        capi.check(capi.lib().smml_tile_rows_f32(capi.fptr(dy), capi.fptr(dx), nb, ctx.l, d, 1.0 / ctx.l, capi.stream()),
                   "tile_rows")
        return dx, None


def segment_mean(x, l: int):
    return _SegmentMean.apply(x, l)


class _ResConv(torch.autograd.Function):
    """Depthwise convolution along the tokens, per head: v [B, h, n, d], w [h, KW] -> [B, n, h*d] (heads merged)."""

    @staticmethod
    def forward(ctx, v, w):
        v = _c(v)
        w2 = _c(w).reshape(w.shape[0], -1)
        B, H, n, D = v.shape
        ctx.det = DETERMINISTIC
        out = torch.empty(B, n, H * D, device=v.device, dtype=torch.float32)
        capi.check(capi.lib().smml_resconv_fwd_f32(capi.fptr(v), capi.fptr(w2), capi.fptr(out), B, H, n, D, w2.shape[1],
                                                   capi.stream()), "resconv_fwd")
        ctx.wshape = w.shape
        ctx.save_for_backward(v, w2)
        return out

    @staticmethod
    def backward(ctx, dout):
        v, w2 = ctx.saved_tensors
        if ctx.det:
            _no_det("resconv backward (res_conv weight gradient)", "the depthwise-convolution weight gradient of the Nystrom block is "
                    "summed with float atomics (smml_resconv_bwd_f32)")
        B, H, n, D = v.shape
        dv = torch.empty_like(v)
        dw = _zeros_like(w2)
        capi.check(capi.lib().smml_resconv_bwd_f32(capi.fptr(_c(dout)), capi.fptr(v), capi.fptr(w2), capi.fptr(dv),
                                                   capi.fptr(dw), B, H, n, D, w2.shape[1], capi.stream()), "resconv_bwd")
        return dv, dw.reshape(ctx.wshape)


def resconv(v, w):
    return _ResConv.apply(v, w)


class _DwConv7(torch.autograd.Function):
    """Depthwise 7x7 convolution (padding 3) on channel-last maps x [B, H, W, C] with weights wm [C, 49], bias [C]."""

    @staticmethod
    def forward(ctx, x, wm, bias):
        x, wm, bias = _c(x), _c(wm), _c(bias)
        B, H, W, Cc = x.shape
        ctx.det = DETERMINISTIC
        y = torch.empty_like(x)
        capi.check(capi.lib().smml_dwconv7_fwd_f32(capi.fptr(x), capi.fptr(wm), capi.fptr(bias), capi.fptr(y), B, H, W, Cc, 0,
                                                   capi.stream()), "dwconv7_fwd")
        ctx.save_for_backward(x, wm)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wm = ctx.saved_tensors
        if ctx.det:
            _no_det("dwconv7 backward (PPEG weight gradient)", "the depthwise-convolution weight and bias gradients are summed with float "
                    "atomics (smml_dwconv7_bwd_weight_f32)")
        B, H, W, Cc = x.shape
        dy = _c(dy)
        dx = torch.empty_like(x)
        L = capi.lib()
        capi.check(L.smml_dwconv7_fwd_f32(capi.fptr(dy), capi.fptr(wm), None, capi.fptr(dx), B, H, W, Cc, 1, capi.stream()),
                   "dwconv7_bwd_data")
        dwm = _zeros_like(wm)
        db = _ZEROS.zeros((Cc,), x.device)
        capi.check(L.smml_dwconv7_bwd_weight_f32(capi.fptr(x), capi.fptr(dy), capi.fptr(dwm), capi.fptr(db), B, H, W, Cc,
                                                 capi.stream()), "dwconv7_bwd_weight")
        return dx, dwm, db


def dwconv7(x, wm, bias):
    return _DwConv7.apply(x, wm, bias)


class _OrthLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, Ph, G, Gh, gamma):
        P, Ph, G, Gh = _c(P), _c(Ph), _c(G), _c(Gh)
        B, D = P.shape
        loss = torch.empty(B, device=P.device, dtype=torch.float32)
        capi.check(capi.lib().smml_orth_loss_f32(capi.fptr(P), capi.fptr(Ph), capi.fptr(G), capi.fptr(Gh), None, capi.fptr(loss),
                                                 None, None, None, None, B, D, float(gamma), capi.stream()), "orth_loss")
        ctx.gamma = float(gamma)
        ctx.save_for_backward(P, Ph, G, Gh)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        P, Ph, G, Gh = ctx.saved_tensors
        B, D = P.shape
        dP, dPh, dG, dGh = (torch.empty_like(t) for t in (P, Ph, G, Gh))
        capi.check(capi.lib().smml_orth_loss_f32(capi.fptr(P), capi.fptr(Ph), capi.fptr(G), capi.fptr(Gh), capi.fptr(_c(dloss)),
                                                 None, capi.fptr(dP), capi.fptr(dPh), capi.fptr(dG), capi.fptr(dGh), B, D,
                                                 ctx.gamma, capi.stream()), "orth_loss_bwd")
        return dP, dPh, dG, dGh, None


def orthogonal_loss(P, Ph, G, Gh, gamma: float = 0.5):
    return _OrthLoss.apply(P, Ph, G, Gh, gamma)
