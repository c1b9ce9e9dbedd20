/* smml.h - C-ABI of the MI355X (gfx950) kernels for the multimodal-MIL attention / fusion hot path.
 *
 * Drop-in boundary for helenypzhang/Subspace-Multimodal-Learning.  The reference has no FFI layer: the
 * path sits behind plain PyTorch nn.Module classes.  This library is what the
 * host-side mirror of those modules (package `subspace-multimodal-learning_amd`) binds through ctypes;
 * each entry point names the reference op sequence (file:line) it replaces.
 *
 * Conventions
 *   - all tensors are fp32, contiguous, token-major (channel-last), and live in HBM of ONE device;
 *     every pointer is a raw device pointer owned by the caller (PyTorch caching allocator on the
 *     Python side); the library never allocates, frees or retains device memory;
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on it and re-entrant;
 *   - return value 0 = ok, negative = error; the message is read with smml_last_error()
 *     (thread-local: the one piece of per-thread state the library keeps); no exception crosses the boundary;
 *   - "accumulated into" outputs must be zeroed (or hold a running sum) by the caller;
 *   - fixed widths of the two fused attention families (no other value is built, the entry points return an error):
 *     head dim 64; position-bias MLP posdim -> 32 -> 32 -> heads / groups (the reference's dim = 128), heads / groups <= 2;
 *   - parameter NAMES are binding, not only types and order: the Python side calls the deformable-attention entry points by them
 *     (_capi.bind), so one meaning keeps one name across entry points (q, tables, logits_t / logits16, H, G, posdim, dtype, ...);
 *     tests/test_named_launch.py fails if a prototype names a parameter the caller's namespace does not hold.
 */
#ifndef SMML_H_
#define SMML_H_

#include <stddef.h>

/* what smml_abi_version() returns.  2: per-call SmmlDeformOpts instead of per-thread setters, region entry points */
#define SMML_ABI_VERSION 2

#ifdef __cplusplus
extern "C" {
#endif

const char* smml_last_error(void);
int smml_abi_version(void);
/* 0 iff `device` is a usable gfx950 device of this process */
int smml_device_check(int device);
/* HIP events as plain handles: time one kernel on the stream it is launched on (bench.py roofline leg) */
void* smml_event_create(void);
int smml_event_destroy(void* ev);
int smml_event_record(void* ev, void* stream);
int smml_event_elapsed_ms(void* start, void* stop, float* ms);

/* ------------------------------------------------------------------------------------------------
 * Strided-batched fp32 GEMM on the f32 matrix cores (exact fp32):
 *   C[b0,b1](m,n) (+)= act(alpha * sum_k A[b0,b1](m,k) B[b0,b1](k,n) + bias) + beta * residual
 * A(m,k) at A + b0*sa0 + b1*sa1 + m*sam + k*sak;  B(k,n) at B + b0*sb0 + b1*sb1 + k*sbk + n*sbn;
 * C(m,n) at C + b0*sc0 + b1*sc1 + m*ldc + n;  residual shares C's batch offsets with row stride ldr.
 * bias_mode 0 none | 1 bias[n] | 2 bias[(m / rows_per_bias) * bias_ld + n];  act 0 none | 1 relu | 2 tanh |
 * 3 sigmoid | 4 tanh on output columns [0, N / 2) and sigmoid on [N / 2, N) (N even: the two gates of a gated attention head in one product); act 3 / 4 always run the exact-fp32 kernels, whatever smml_gemm_set_mode says.
 * splitk > 1 or accumulate != 0: products are atomically added into C (caller zeroes C or keeps a running
 * sum there; no act / residual); batch strides of 0 on C fold a batch dimension into one output.
 * Replaces nn.Linear / 1x1 nn.Conv sites of the path: models/DeformCrossTransMIL.py:35-37,83,93-95,
 * 196; models/DeformableAttention2D.py:218-221; models/DeformableAttention1D.py:150-153;
 * models/NystromAttention.py:60-65,86,122-140 - and their backward products. */
int smml_gemm_f32(const float* A, const float* B, float* C, const float* bias, const float* residual,
                  int M, int N, int K, long long sam, long long sak, long long sbk, long long sbn,
                  long long ldc, long long ldr, int nb0, int nb1, long long sa0, long long sa1,
                  long long sb0, long long sb1, long long sc0, long long sc1, long long sbias0,
                  long long sbias1, int bias_mode, int rows_per_bias, long long bias_ld, int act,
                  int splitk, int accumulate, float alpha, float beta, void* stream);
/* Deterministic form of the split-K / folded-batch products (functional.deterministic): same arguments plus a workspace.  The product
 * kernels store alpha A B of every (batch item, split-K slice) z = (b0 nb1 + b1) splitk + ks densely at workspace[z][m][n]; a second kernel
 * owns one element of C per thread and adds, in ascending z, the splitk slices of its batch item and - for a batch dimension folded onto
 * one C (sc0 / sc1 = 0) - every item of that dimension.  C is overwritten with the sum (accumulate != 0: the sum is added onto what C
 * holds); no float atomics.  bias, residual and act must be NULL / 0.
 * workspace: smml_gemm_f32_det_workspace_bytes = nb0 nb1 splitk M N 4 bytes, 16-byte aligned. */
size_t smml_gemm_f32_det_workspace_bytes(int M, int N, int nb0, int nb1, int splitk);
int smml_gemm_f32_det(const float* A, const float* B, float* C, const float* bias, const float* residual,
                      int M, int N, int K, long long sam, long long sak, long long sbk, long long sbn,
                      long long ldc, long long ldr, int nb0, int nb1, long long sa0, long long sa1,
                      long long sb0, long long sb1, long long sc0, long long sc1, long long sbias0,
                      long long sbias1, int bias_mode, int rows_per_bias, long long bias_ld, int act,
                      int splitk, int accumulate, float alpha, float beta, void* workspace, size_t workspace_bytes,
                      void* stream);
/* test hook: 1 routes every product through the generic (any stride / any K) kernel instead of the tiled
 * fast path (K % 16 == 0, 16-byte aligned operands with a unit stride on k or on the row index). */
void smml_gemm_force_generic(int on);
/* precision / tuning switch of the tiled kernels: 0 automatic (default: exact fp32 on the f32 MFMA, split-bf16 for large
 * square-ish products), 1 fp32-MFMA kernel only, 2 split-bf16 (three terms, fp32-grade) wherever it applies, 3 single-term bf16
 * (operands rounded to bf16 when staged, fp32 accumulation: the 16-bit compute mode of the Nystrom block), 4 single-term fp16 (operands
 * rounded to fp16 when staged - 11 mantissa bits, fp16's exponent range: for forward-range operands; the fp16 compute modes issue their
 * gradient products in mode 3). */
void smml_gemm_set_mode(int mode);
int smml_gemm_get_mode(void);
/* tile-height switch of the tiled kernels: 0 automatic (64-row tiles for launches that the 128-row tiling leaves below two
 * workgroups per CU, e.g. the batched 256^3 products of the Nystrom pseudo-inverse), 1 never, 2 wherever it applies. */
void smml_gemm_set_small_tile(int v);

/* bf16-STORAGE GEMM (16-bit matrix pipe, fp32 accumulation): A and B are bf16 in memory, C is bf16 (out_bf16 = 1) or fp32.
 *   trans = 0   C[M, N] = A[M, K] B[N, K]^T   (row strides lda / ldb >= K, in elements; K % 8 == 0)
 *   trans = 1   C[M, N] = A[K, M]^T B[K, N]   (row strides lda >= M, ldb >= N; M % 8 == 0, N % 8 == 0)
 * bias (fp32 [N] or NULL) is added once.  splitk > 1 (fp32 output only): the K range is cut into slices whose partial products are
 * ADDED to C atomically - the caller zeroes C; splitk = 0: chosen by the library (one round of workgroups; C must then be zeroed too).  Operands 16-byte aligned, lda / ldb multiples of 8.
 * The projections of the Nystrom block's bf16 compute mode (models/NystromAttention.py:88 to_qkv, :147 to_out) and their backward
 * products with bf16 bags (BASELINE configs 2 / 4): activations stay bf16 end to end. */
int smml_gemm_b16(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long long lda, long long ldb,
                  long long ldc, int trans, int out_bf16, int splitk, void* stream);
/* tile selection of the bf16-storage GEMM: 0 automatic (the 256-row, eight-wave tile where its grid still covers the chip), 1 the
 * 128 x 128 tile only, 2 the 256-row tile wherever M >= 256 and N >= 128 (test / measurement switch; SMML_B16_TILE presets it). */
void smml_gemm_b16_set_tile(int mode);
/* measurement switch: 1 (default) places the tiles of one slice of a split reduction on one XCD (they share the slice's operands through one
 * L2), 0 spreads them over the XCDs like any other launch. */
void smml_gemm_b16_set_slice_major(int on);
/* nb problems of that shape at element strides sa / sb / sc (multiples of 8) between them; sc = 0 (fp32 output only): the problems' products
 * are ADDED into the one zeroed output, like split-K slices.  A bag's n real rows are addressed in place as one batch item (the zero rows
 * the reference pads in front of a bag, NystromAttention.py:82, are never multiplied). */
int smml_gemm_b16_batched(const void* A, const void* B, void* C, const float* bias, int M, int N, int K, long long lda, long long ldb,
                          long long ldc, int trans, int out_bf16, int splitk, int nb, long long sa, long long sb, long long sc, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Grouped 1x1 convolution on token-major data (to_q / to_k / to_v, models/DeformableAttention2D.py:218-221, DeformableAttention1D.py:150-153)
 * as three streaming kernels, for the group shapes smml_grouped_pointwise_applies accepts (16 input and 64 output channels per group, any
 * number of groups and rows):   y[m, cout_g g + o] = sum_i x[m, cin_g g + i] w[cout_g g + o, i]
 * x [rows, groups cin_g], w [groups cout_g, cin_g], y / dy [rows, groups cout_g], all dense fp32; x, dy and w 16-byte aligned.
 * fwd and dx give the bits of the same product issued as a batch over the groups through smml_gemm_f32; dw [groups cout_g, cin_g] is
 * OVERWRITTEN with a sum in a fixed order (per-workgroup partials in the workspace, no float atomics): deterministic in every mode. */
int smml_grouped_pointwise_applies(int groups, int cin_g, int cout_g);
int smml_grouped_pointwise_fwd_f32(const float* x, const float* w, float* y, long long rows, int groups, int cin_g, int cout_g, void* stream);
int smml_grouped_pointwise_dx_f32(const float* dy, const float* w, float* dx, long long rows, int groups, int cin_g, int cout_g, void* stream);
/* workspace: W groups cout_g cin_g 4 bytes with W = ceil(rows / rpw) workgroups of rpw = max(64, ceil(rows / 256) rounded up to a multiple
 * of 32) rows, 16-byte aligned. */
size_t smml_grouped_pointwise_dw_workspace_bytes(long long rows, int groups, int cin_g, int cout_g);
int smml_grouped_pointwise_dw_f32(const float* dy, const float* x, float* dw, long long rows, int groups, int cin_g, int cout_g,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm over the last dim C (<= 1024) of x [R, C]; saves mean / rstd per row.
 * Replaces nn.LayerNorm at models/DeformCrossTransMIL.py:44,71,75,90,144 and mil.py:175,187. */
int smml_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, float* mean,
                           float* rstd, long long R, int C, float eps, void* stream);
/* The mean over a bag's tokens of LayerNorm(x) (the path's final norm, DeformCrossTransMIL.py:144 and Pooler's mean :193) in one pass over
 * x [nb, n, C] that never stores the normalised tensor: out[b, c] += (1 / n) sum_r LayerNorm(x)[b, r, c], out [nb, C] accumulated into
 * (the caller zeroes it); mean / rstd [nb n] are smml_layernorm_fwd_f32's, bit for bit.  C = 128 only, x / gamma / beta 16-byte aligned:
 * any other call is an error (compose smml_layernorm_fwd_f32 and smml_colsum_f32 instead). */
int smml_layernorm_fwd_mean_f32(const float* x, const float* gamma, const float* beta, float* mean, float* rstd, float* out, int nb,
                                long long n, int C, float eps, void* stream);
/* Deterministic form: out OVERWRITTEN.  A bag's rows are cut into chunks of rpc = 64 rows (n <= 1024: 512; beyond n = 131 072:
 * ceil(n / 2048) rounded up to a multiple of 32) - a function of n alone, the same in both forms; the chunk sums (scaled) go to
 * workspace[chunk][b][C] and a second kernel adds them in a fixed order.  workspace: ceil(n / rpc) nb C 4 bytes, 16-byte aligned (0 for C != 128). */
size_t smml_layernorm_fwd_mean_det_workspace_bytes(int nb, long long n, int C);
int smml_layernorm_fwd_mean_det_f32(const float* x, const float* gamma, const float* beta, float* mean, float* rstd, float* out, int nb,
                                    long long n, int C, float eps, void* workspace, size_t workspace_bytes, void* stream);
/* dy row for x row i is dy[(i / rows_per_dy) * C + c] * dy_scale (rows_per_dy > 1 broadcasts one
 * gradient row over a token block, e.g. the gradient of Pooler's mean, DeformCrossTransMIL.py:193);
 * dx is overwritten (accumulate_dx = 0) or added to; dgamma / dbeta are accumulated into. */
int smml_layernorm_bwd_f32(const float* x, const float* dy, const float* gamma, const float* mean,
                           const float* rstd, float* dx, float* dgamma, float* dbeta, long long R, int C,
                           long long rows_per_dy, float dy_scale, int accumulate_dx, void* stream);
/* Deterministic form: the workgroups write their dgamma / dbeta rows to workspace[workgroup][2][C] and a second kernel adds them in a
 * fixed order ONTO dgamma / dbeta (the accumulate-into contract above); dx is smml_layernorm_bwd_f32's, bit for bit.
 * workspace: W 2 C 4 bytes with W = min(ceil(R / 16), 768) at C = 128 and min(ceil(R / 4), 1024) otherwise, 16-byte aligned. */
size_t smml_layernorm_bwd_det_workspace_bytes(long long R, int C);
int smml_layernorm_bwd_det_f32(const float* x, const float* dy, const float* gamma, const float* mean,
                               const float* rstd, float* dx, float* dgamma, float* dbeta, long long R, int C,
                               long long rows_per_dy, float dy_scale, int accumulate_dx, void* workspace,
                               size_t workspace_bytes, void* stream);

/* out[b, c] += scale * sum_r x[b, r, c] for x [nb, R, C]; out accumulated into.
 * Pooler mean (DeformCrossTransMIL.py:193) and bias gradients. */
int smml_colsum_f32(const float* x, float* out, int nb, long long R, int C, float scale, void* stream);
/* Deterministic form: out[b, c] = scale * sum_r x[b, r, c], OVERWRITTEN.  The rows are cut into chunks that depend on (R, C) alone; the
 * chunk sums (scaled) go to workspace[chunk][b][C] and a second kernel adds the chunks in a fixed order.
 * workspace: ceil(R / rpc) nb C 4 bytes, 16-byte aligned, with rows per chunk rpc = 256, or - where C % 4 == 0, C <= 1024 and C / 4 divides
 * 256 - max(64 rl, ceil(R / 2048)) rounded up to a multiple of rl = 256 / (C / 4). */
size_t smml_colsum_det_workspace_bytes(int nb, long long R, int C);
int smml_colsum_det_f32(const float* x, float* out, int nb, long long R, int C, float scale, void* workspace,
                        size_t workspace_bytes, void* stream);

/* OrthogonalLoss (models/cmta_utils.py:1212-1228) on rows P, P_hat, G, G_hat [B, D]: loss [B] (nullable) and, when
 * dloss [B] is given, dP / dPh / dG / dGh [B, D]; one wave per sample, wavefront reductions. */
int smml_orth_loss_f32(const float* P, const float* Ph, const float* G, const float* Gh, const float* dloss, float* loss,
                       float* dP, float* dPh, float* dG, float* dGh, int B, int D, float gamma, void* stream);

/* Tail of BatchLoss after its two Gram products (utils/loss.py:26-40): S = go / ||go||_row, V = mean_g gv[g] / ||gv[g]||_row,
 * loss = (S - V)^2 / n_total on [R, R] (dloss NULL), or the gradients dgo [R, R], dgv [nv, R, R] for a given dloss [R, R]; R = batch x world
 * <= 64, nv <= 16 (the reference's 8 offset groups).  One launch per direction instead of ~30 launch-bound elementwise kernels. */
int smml_batchloss_tail_f32(const float* go, const float* gv, const float* dloss, float* loss, float* dgo, float* dgv, int R, int nv,
                            float n_total, void* stream);

/* dx = dy * (y > 0)  (ReLU of _fc1, DeformCrossTransMIL.py:83) */
int smml_relu_bwd_f32(const float* dy, const float* y, float* dx, long long n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Offset network of the deformable attention (DeformableAttention2D.py:207-213,255-266;
 * DeformableAttention1D.py:139-146,176-183): depthwise strided conv (kernel ks, stride r,
 * pad (ks-r)/2) -> GELU -> 1x1 (dg -> posdim) -> tanh -> * offset_scale; vgrid = meshgrid + offsets
 * (returned to the caller's loss un-normalised); vs = 2 vgrid / max(t-1, 1) - 1.
 *   q [B, Hh, Ww, G*dg] (1-D module: Hh = 1)   w0 [dg, 1, ks(, ks)]  b0 [dg]  w2 [posdim, dg]
 *   vgrid [(B G), posdim, th, tw]               vs [(B G), th*tw, posdim] */
int smml_offsets_out_len(int s, int ks, int r);
int smml_offsets_fwd_f32(const float* q, const float* w0, const float* b0, const float* w2, float* vgrid,
                         float* vs, int B, int Hh, int Ww, int G, int dg, int ks, int r, int posdim,
                         float offset_scale, void* stream);
/* upstream gradient = dvgrid (direct, nullable) + 2/max(t-1,1) * dvs (nullable); dw0, db0, dw2 are overwritten (gather formulation, no
 * atomics); dq is overwritten, or - accumulate_dq = 1 - ADDED to: dq then already holds the gradient q received from its other consumer,
 * the fused attention core (one pass over the [B, N, 512] tensor instead of a store plus an elementwise add).
 * workspace: smml_offsets_bwd_workspace_bytes(...) bytes, 16-byte aligned. */
size_t smml_offsets_bwd_workspace_bytes(int B, int Hh, int Ww, int G, int dg, int ks, int r, int posdim);
int smml_offsets_bwd_f32(const float* q, const float* w0, const float* b0, const float* w2,
                         const float* dvgrid, const float* dvs, float* dq, float* dw0, float* db0,
                         float* dw2, void* workspace, size_t workspace_bytes, int B, int Hh, int Ww, int G, int dg,
                         int ks, int r, int posdim, float offset_scale, int accumulate_dq, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Bilinear sampling = F.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=False) of the
 * grouped key/value stream (DeformableAttention2D.py:268-274; DeformableAttention1D.py:36-43,185-190).
 *   x [B, Hh, Ww, G*cg]   vs [(B G), J, posdim]   kv [B, J, G*cg]
 * The 1-D module's degenerate sampling is posdim = 1 with the map laid out [Hh = n, Ww = 1]. */
int smml_bilinear_sample_fwd_f32(const float* x, const float* vs, float* kv, int B, int Hh, int Ww, int G,
                                 int cg, int J, int posdim, void* stream);
/* dx accumulated into (float atomics); dvs accumulated into (+=). */
int smml_bilinear_sample_bwd_f32(const float* x, const float* vs, const float* dkv, float* dx, float* dvs,
                                 int B, int Hh, int Ww, int G, int cg, int J, int posdim, void* stream);
/* Deterministic form: dx is OVERWRITTEN by a gather.  Per (bag, group) the 4 J corner contributions are sorted in LDS by the unique key
 * pixel 2^14 + (4 j + corner) (corners outside the map form a run nobody reads); every (pixel, channel) then adds its pixel's run in sorted
 * order, pixels nobody samples get 0 - no float atomics.  dvs is accumulated into (+=) exactly as above.
 * cg 16 or 32, J <= 4096, Hh Ww <= 262142 (an error otherwise).
 * workspace: B G (4 J + Hh Ww + 1) 4 bytes (the sorted keys and the start of every pixel's run), 16-byte aligned. */
size_t smml_bilinear_sample_bwd_det_workspace_bytes(int B, int Hh, int Ww, int G, int J);
int smml_bilinear_sample_bwd_det_f32(const float* x, const float* vs, const float* dkv, float* dx, float* dvs,
                                     void* workspace, size_t workspace_bytes, int B, int Hh, int Ww, int G, int cg,
                                     int J, int posdim, void* stream);
/* integer path only (bit-exact contract): corner indices cx, cy [n, 4] and in-bounds masks cm [n, 4]
 * in the order (x0,y0) (x1,y0) (x0,y1) (x1,y1) for n sample points vs [n, posdim]. */
int smml_bilinear_corners_f32(const float* vs, int* cx, int* cy, unsigned char* cm, int n, int Hh, int Ww,
                              int posdim, void* stream);

/* Optional behaviour of ONE fused deformable-attention launch (trailing `opts` argument of the entry points below; NULL = all defaults).
 * Passed by the caller with every call: the library keeps no per-thread or global launch state. */
typedef struct SmmlDeformOpts {
  const unsigned long long* seed_offset; /* device-resident offset hashed into dropout_seed when the kernel RUNS (a launch captured in a hipGraph
                                            bakes dropout_seed in; the offset lets every replay draw a new mask), or NULL */
  int raw_distance;                      /* 1: posdim-1 launches feed the bias MLP the raw offset gq - vs (DeformableAttention1D.py:92,
                                            cpb_log_distance = False); 0: its signed log (the reference's default; posdim 2 has no such switch) */
  const unsigned short* mask_table;      /* smml_deform_attn16_bwd with relu_masks == NULL: layer-2 ReLU decisions from this table (filled by
                                            smml_cpb_mask_table with mask_table_pmax), or NULL = recompute layer 2 per pair */
  float mask_table_pmax;
  unsigned short* export_masks;          /* tests: smml_deform_attn16_bwd with relu_masks == NULL also writes the decisions it used here
                                            ([B, H, nst / 32, J, 2, 32] u16, the forward's layout), or NULL */
  int region_lds_cap;                    /* tests: the region entry points keep only regions with an id below this in LDS and take the others from
                                            global memory (the path of parameter sets with more than 2048 linear regions); 0 = the default (2048) */
} SmmlDeformOpts;

/* ------------------------------------------------------------------------------------------------
 * Fused deformable cross-attention core: softmax(scale q k^T + CPB(gq - vs)) v with the continuous
 * position bias MLP posdim -> 32 -> 32 -> heads/groups evaluated on the matrix cores per
 * (query, key) pair and never materialised.
 * Replaces DeformableAttention2D.py:120-157,284-312 and DeformableAttention1D.py:60-102,205-232.
 *   q [B, N, H*64] (unscaled)  k, v [B, J, H*64]  vs [(B G), J, posdim]  gq [N, posdim]
 *   w1 [32, posdim] b1 [32] w2 [32, 32] b2 [32] w3 [H/G, 32] b3 [H/G]
 *   out [B, N, H*64]  lse [B, H, N]  logits_t [B, H, nst / 32, J, 32] and relu_masks [B, H, nst / 32, J, 2, 32] uint16 with
 *   nst = smml_deform_attn_nst(N) (both nullable together: only needed for backward).  Score-shaped tensors are stored per 32-query
 *   tile - the unit one wave owns - so that every pass streams contiguous memory; relu_masks holds the ReLU decisions of the
 *   position bias's second layer, 32 bits per (query, key, head), in the bit order the backward kernel consumes.  Both are
 *   opaque to the caller (scratch it allocates and hands back to the backward).  H/G <= 2.
 * ev_start / ev_stop (nullable, handles of smml_event_create) are recorded on `stream` around the fused
 * forward kernel, resp. around the position-bias backward kernel (the dominant kernel of the step). */
int smml_deform_attn_nst(int N);
int smml_deform_attn_fwd_f32(const float* q, const float* k, const float* v, const float* vs, const float* gq,
                             const float* w1, const float* b1, const float* w2, const float* b2,
                             const float* w3, const float* b3, float* out, float* lse, float* logits_t,
                             unsigned short* relu_masks, int B, int N, int J, int H, int G, int posdim, float scale,
                             float dropout_p, unsigned long long dropout_seed, void* ev_start, void* ev_stop, void* stream, const SmmlDeformOpts* opts);
/* scratch the backward needs: position-bias gradient slabs, the per-wave d vs rows and the query-sliced dK / dV partial sums;
 * 16-byte aligned */
size_t smml_deform_attn_bwd_workspace_bytes(int B, int N, int J, int H);
/* dlogits_t: scratch of logits_t's size and layout (receives d scores); dq / dk / dv / dw* / db* overwritten;
 * dvs overwritten.  Every output is reduced in a fixed order (no float atomics): run-to-run identical results. */
int smml_deform_attn_bwd_f32(const float* q, const float* k, const float* v, const float* vs, const float* gq,
                             const float* w1, const float* b1, const float* w2, const float* b2,
                             const float* w3, const float* b3, const float* out, const float* dout,
                             const float* lse, const float* logits_t, const unsigned short* relu_masks,
                             float* dlogits_t, float* dq, float* dk, float* dv, float* dvs, float* dw1, float* db1, float* dw2, float* db2, float* dw3,
                             float* db3, void* workspace, size_t workspace_bytes, int B, int N, int J, int H,
                             int G, int posdim, float scale, float dropout_p, unsigned long long dropout_seed,
                             void* ev_start, void* ev_stop, void* stream, const SmmlDeformOpts* opts);
/* Wide position-bias family of the fp32-grade core (csrc/deform_attn_wide.hip): the same contract as smml_deform_attn_fwd_f32 / _bwd_f32 for a
 * bias MLP posdim -> W -> W -> H / G with W = 64 or 128 (dim = 256 / 512 of the modules; W is an argument, anything else is refused).
 * w1 [W, posdim], b1 [W], w2 [W, W], b2 [W], w3 [H / G, W], b3 [H / G].  The MLP is evaluated once per (bag, group, query, key) in exact
 * fp32 (layer 2 on v_mfma_f32_32x32x2_f32) into bias tiles of the score layout [B, H, nst / 32, J, 32], which the attention kernel reads:
 *   training:  pass logits_t (the bias tiles are built there and overwritten in place by the scores) and bias_t = NULL;
 *   inference: pass logits_t = NULL and bias_t, caller-allocated scratch of the same size.
 * No ReLU mask is saved: the backward recomputes the MLP with the forward's own evaluator (bit-identical decisions).
 * smml_deform_attn_wide_decisions (tests) exports those decisions: masks [(B G), N, J, 2, W / 32] uint32 - layer 1 then layer 2, hidden
 * channel ch at bit ch % 32 of word ch / 32.  Every output is reduced in a fixed order (no float atomics): run-to-run identical.
 * workspace of the backward: smml_deform_attn_wide_bwd_workspace_bytes, 16-byte aligned (0: unsupported sizes). */
int smml_deform_attn_wide_fwd_f32(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* w1,
                                  const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, float* out, float* lse,
                                  float* logits_t, float* bias_t, int B, int N, int J, int H, int G, int W, int posdim, float scale,
                                  float dropout_p, unsigned long long dropout_seed, void* ev_start, void* ev_stop, void* stream,
                                  const SmmlDeformOpts* opts);
size_t smml_deform_attn_wide_bwd_workspace_bytes(int B, int N, int J, int H, int G, int W);
int smml_deform_attn_wide_bwd_f32(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* w1,
                                  const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, const float* out,
                                  const float* dout, const float* lse, const float* logits_t, float* dlogits_t, float* dq, float* dk, float* dv,
                                  float* dvs, float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, void* workspace,
                                  size_t workspace_bytes, int B, int N, int J, int H, int G, int W, int posdim, float scale, float dropout_p,
                                  unsigned long long dropout_seed, void* ev_start, void* ev_stop, void* stream, const SmmlDeformOpts* opts);
int smml_deform_attn_wide_decisions(const float* vs, const float* gq, const float* w1, const float* b1, const float* w2, const float* b2,
                                    unsigned* masks, int B, int N, int J, int G, int W, int posdim, void* stream, const SmmlDeformOpts* opts);
/* The same fused core with the position bias evaluated EXACTLY PER LINEAR REGION of its MLP (csrc/cpb_regions.h; round 5).  The MLP of
 * models/DeformableAttention2D.py:129-152 is piecewise affine in the signed-log offsets (:148): smml_cpb_regions_build tabulates, for the
 * current parameters, which linear piece every cell of [-pmax, pmax]^2 lies in (cells a ReLU kink crosses carry the kink's line, cells
 * several kinks cross are refined once, what is left evaluates the MLP itself), and the forward / backward below replace the per-pair MLP
 * by a lookup + 2 FMAs, resp. by three fixed-point moment sums per region from which all six parameter gradients follow linearly.
 * Results are those of smml_deform_attn_fwd_f32 / _bwd_f32 to fp32 rounding (no tolerance added: tests/test_gpu_parity.py runs both);
 * posdim = 2, signed-log offsets, one head per offset group (G = H), J <= 16384.
 *   tables: caller-allocated scratch of smml_cpb_regions_bytes() bytes, 256-byte aligned; built per forward call (the parameters change
 *           every step), handed unchanged to the backward of the same call.  pmax >= max |slog(gq - vs)| for speed only: pairs
 *           outside the square evaluate the MLP.
 *   region_ids [B, H, nst / 32, J, 32] uint16: the linear piece of every pair (0xFFFF: none), saved in place of relu_masks.
 *   workspace of the backward: smml_deform_attn_region_bwd_workspace_bytes, 256-byte aligned.
 * Every output is run-to-run identical (slab sums in a fixed order; the region moments are integer sums). */
size_t smml_cpb_regions_bytes(void);
int smml_cpb_regions_build(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                           float pmax, void* tables, size_t tables_bytes, void* stream);
int smml_deform_attn_region_fwd_f32(const float* q, const float* k, const float* v, const float* vs, const float* gq,
                                    const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                                    const float* b3, const void* tables, float* out, float* lse, float* logits_t,
                                    unsigned short* region_ids, int B, int N, int J, int H, float scale, float dropout_p,
                                    unsigned long long dropout_seed, void* ev_start, void* ev_stop, void* stream, const SmmlDeformOpts* opts);
size_t smml_deform_attn_region_bwd_workspace_bytes(int B, int N, int J, int H);
int smml_deform_attn_region_bwd_f32(const float* q, const float* k, const float* v, const float* vs, const float* gq,
                                    const float* w1, const float* b1, const float* w2, const float* b2, const float* w3,
                                    const float* b3, const void* tables, const float* out, const float* dout, const float* lse,
                                    const float* logits_t, const unsigned short* region_ids, float* dlogits_t, float* dq, float* dk,
                                    float* dv, float* dvs, float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3,
                                    void* workspace, size_t workspace_bytes, int B, int N, int J, int H, float scale, float dropout_p,
                                    unsigned long long dropout_seed, void* ev_start, void* ev_stop, void* stream, const SmmlDeformOpts* opts);

/* The 1-D sibling (csrc/cpb_regions1d.h): the MLP of DeformableAttention1D.py:69-98 (Linear(1, 32) - ReLU - Linear(32, 32) - ReLU -
 * Linear(32, H/G)) is piecewise affine in ONE signed-log offset, with at most 1088 breakpoints.  smml_cpb_regions1d_build sorts them and
 * tabulates per piece its ReLU pattern (D1 | D2 << 32) and (a, c) for each of the `outputs` (= H / G, 1 or 2) outputs, plus a uniform index
 * grid over [-pmax, pmax] (pmax = 0: the span of the breakpoints; points outside the grid take an exact binary search - pmax is for speed
 * only).  The forward / backward replace the per-pair MLP by a lookup + 2 FMAs, resp. by two fixed-point moments per piece and output.
 * posdim = 1, signed-log offsets (opts->raw_distance must be 0), H / G in {1, 2}, J <= 16384, the fp32-grade core; no weights are
 * passed: the tables hold them.  Results are those of smml_deform_attn_fwd_f32 / _bwd_f32 (posdim 1) to fp32 rounding.
 *   tables: smml_cpb_regions1d_bytes() bytes, 256-byte aligned, built per forward call and handed unchanged to the backward.
 *   region_ids [B, H, nst / 32, J, 32] uint16: the piece of every pair, per head (the heads of a group share it).
 *   workspace of the backward: smml_deform_attn_region1d_bwd_workspace_bytes, 256-byte aligned.  A non-finite d score makes the six
 *   parameter gradients NaN.  Every output is run-to-run identical. */
size_t smml_cpb_regions1d_bytes(void);
int smml_cpb_regions1d_build(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                             int outputs, float pmax, void* tables, size_t tables_bytes, void* stream);
int smml_deform_attn_region1d_fwd_f32(const float* q, const float* k, const float* v, const float* vs, const float* gq, const void* tables,
                                      float* out, float* lse, float* logits_t, unsigned short* region_ids, int B, int N, int J, int H, int G,
                                      float scale, float dropout_p, unsigned long long dropout_seed, void* ev_start, void* ev_stop,
                                      void* stream, const SmmlDeformOpts* opts);
size_t smml_deform_attn_region1d_bwd_workspace_bytes(int B, int N, int J, int H);
int smml_deform_attn_region1d_bwd_f32(const float* q, const float* k, const float* v, const float* vs, const float* gq, const void* tables,
                                      const float* out, const float* dout, const float* lse, const float* logits_t,
                                      const unsigned short* region_ids, float* dlogits_t, float* dq, float* dk, float* dv, float* dvs,
                                      float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, void* workspace,
                                      size_t workspace_bytes, int B, int N, int J, int H, int G, float scale, float dropout_p,
                                      unsigned long long dropout_seed, void* ev_start, void* ev_stop, void* stream, const SmmlDeformOpts* opts);

/* The same two entry points in the 16-bit compute modes of smml_deform_attn16_fwd / _bwd (dtype 0 = bf16, 1 = fp16: single-term operands on
 * the matrix pipe, scores saved as fp16 [B, H, nst / 32, J, 32], d scores as bf16): the position bias stays the fp32 lookup per linear
 * region, so it is MORE exact than the 16-bit per-pair MLP it replaces, and the launch pair costs about half of it.  Same conditions as
 * above; tables from smml_cpb_regions_build; workspace of the backward: smml_deform_attn_region_bwd_workspace_bytes, 256-byte aligned. */
int smml_deform_attn16_region_fwd(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* w1,
                                  const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, const void* tables,
                                  float* out, float* lse, unsigned short* logits16, unsigned short* region_ids, int B, int N, int J, int H,
                                  float scale, float dropout_p, unsigned long long dropout_seed, int dtype, void* ev_start, void* ev_stop,
                                  void* stream, const SmmlDeformOpts* opts);
int smml_deform_attn16_region_bwd(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* w1,
                                  const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, const void* tables,
                                  const float* out, const float* dout, const float* lse, const unsigned short* logits16,
                                  const unsigned short* region_ids, unsigned short* dlogits16, float* dq, float* dk, float* dv, float* dvs,
                                  float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, void* workspace,
                                  size_t workspace_bytes, int B, int N, int J, int H, float scale, float dropout_p,
                                  unsigned long long dropout_seed, int dtype, void* ev_start, void* ev_stop, void* stream,
                                  const SmmlDeformOpts* opts);

/* The region path with ONE OR TWO heads per offset group (H / G in {1, 2}; the MLP of DeformableAttention2D.py:129-152 then ends in
 * Linear(32, H / G)).  Both outputs share layers 1 and 2, so they share the regions, the lookup and the region ids; only (a, c) differs per
 * output.  smml_cpb_regions_mh_build tabulates the same regions as smml_cpb_regions_build plus, for outputs == 2, the (a, c) of the second
 * output (w3 [outputs, 32], b3 [outputs]; same buffer size, smml_cpb_regions_bytes()).  In the forward and backward, head h belongs to
 * offset group h / (H / G), reads that group's sample positions vs [(B G), J, 2] and takes output h % (H / G); d vs of a group is the sum
 * over its heads.  region_ids [B, H, nst / 32, J, 32]: per head (the heads of a group hold equal ids).  The tables must have been built
 * with outputs = H / G.  Workspace of the backwards: smml_deform_attn_region_mh_bwd_workspace_bytes, 256-byte aligned.  With H == G every
 * output is bit-identical to the one-output entry points above.  A non-finite d score makes the six parameter gradients NaN.  Every
 * output is run-to-run identical. */
int smml_cpb_regions_mh_build(const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, int outputs,
                              float pmax, void* tables, size_t tables_bytes, void* stream);
int smml_deform_attn_region_mh_fwd_f32(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* w1,
                                       const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, const void* tables,
                                       float* out, float* lse, float* logits_t, unsigned short* region_ids, int B, int N, int J, int H, int G,
                                       float scale, float dropout_p, unsigned long long dropout_seed, void* ev_start, void* ev_stop, void* stream,
                                       const SmmlDeformOpts* opts);
size_t smml_deform_attn_region_mh_bwd_workspace_bytes(int B, int N, int J, int H, int G);
int smml_deform_attn_region_mh_bwd_f32(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* w1,
                                       const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, const void* tables,
                                       const float* out, const float* dout, const float* lse, const float* logits_t,
                                       const unsigned short* region_ids, float* dlogits_t, float* dq, float* dk, float* dv, float* dvs, float* dw1,
                                       float* db1, float* dw2, float* db2, float* dw3, float* db3, void* workspace, size_t workspace_bytes, int B,
                                       int N, int J, int H, int G, float scale, float dropout_p, unsigned long long dropout_seed, void* ev_start,
                                       void* ev_stop, void* stream, const SmmlDeformOpts* opts);
int smml_deform_attn16_region_mh_fwd(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* w1,
                                     const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, const void* tables,
                                     float* out, float* lse, unsigned short* logits16, unsigned short* region_ids, int B, int N, int J, int H, int G,
                                     float scale, float dropout_p, unsigned long long dropout_seed, int dtype, void* ev_start, void* ev_stop,
                                     void* stream, const SmmlDeformOpts* opts);
int smml_deform_attn16_region_mh_bwd(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* w1,
                                     const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, const void* tables,
                                     const float* out, const float* dout, const float* lse, const unsigned short* logits16,
                                     const unsigned short* region_ids, unsigned short* dlogits16, float* dq, float* dk, float* dv, float* dvs,
                                     float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, void* workspace,
                                     size_t workspace_bytes, int B, int N, int J, int H, int G, float scale, float dropout_p,
                                     unsigned long long dropout_seed, int dtype, void* ev_start, void* ev_stop, void* stream,
                                     const SmmlDeformOpts* opts);

/* 16-bit compute mode of the same fused core (csrc/deform_attn16.hip; BASELINE config 4 names bf16, config 5 fp16): the op sequence of
 * smml_deform_attn_fwd_f32 / _bwd_f32 (models/DeformableAttention2D.py:120-157,284-312; DeformableAttention1D.py:60-102,205-232) with
 * single-term 16-bit operands on the matrix pipe - dtype 0 = bf16, 1 = fp16 for forward-range operands (q, k, v, probabilities, the
 * hidden layer and W2 of the position-bias MLP); gradient-range operands are always bf16 - and 16-bit score storage:
 *   logits16  [B, H, nst / 32, J, 32] fp16 in BOTH modes (the pre-softmax scores incl. bias are of forward range; in training the forward's
 *             own softmax runs on the rounded values, and with dropout the keep decision rides in the lowest mantissa bit)
 *   dlogits16 [B, H, nst / 32, J, 32] bf16 (scratch of the backward: d scores = d bias)
 * q / k / v / out and every gradient stay fp32 in memory; layer 1 of the position-bias MLP, the softmax statistics and all
 * accumulators are fp32; relu_masks, the workspace (smml_deform_attn_bwd_workspace_bytes) and the decision export
 * (smml_deform_attn_relu1_masks) are shared with the fp32 path.  ev_start / ev_stop as in the fp32 entry points. */
int smml_deform_attn16_fwd(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* w1,
                           const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, float* out,
                           float* lse, unsigned short* logits16, unsigned short* relu_masks, int B, int N, int J, int H, int G,
                           int posdim, float scale, float dropout_p, unsigned long long dropout_seed, int dtype, void* ev_start,
                           void* ev_stop, void* stream, const SmmlDeformOpts* opts);
int smml_deform_attn16_bwd(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* w1,
                           const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, const float* out,
                           const float* dout, const float* lse, const unsigned short* logits16, const unsigned short* relu_masks,
                           unsigned short* dlogits16, float* dq, float* dk, float* dv, float* dvs, float* dw1, float* db1,
                           float* dw2, float* db2, float* dw3, float* db3, void* workspace, size_t workspace_bytes, int B, int N,
                           int J, int H, int G, int posdim, float scale, float dropout_p, unsigned long long dropout_seed,
                           int dtype, void* ev_start, void* ev_stop, void* stream, const SmmlDeformOpts* opts);
/* relu_masks == NULL in smml_deform_attn16_bwd: the forward ran without the MLP (smml_deform_attn_table_fwd below) and saved no ReLU bits -
 * the backward recomputes layer 2 per pair (one bf16 term) and differentiates the per-pair MLP exactly as with saved bits
 * (opts->export_masks: tests read the decisions it used). */
/* Mask table: instead of recomputing layer 2 per pair, a relu_masks == NULL backward can take the layer-2 decisions from a table of the sign
 * pattern of W2 relu(W1 p + b1) + b2 at the centres of cells^posdim cells over [-pmax, pmax]^posdim (cells = smml_cpb_mask_table_cells(posdim):
 * 1024 per axis in 2-D, 16384 in 1-D; `table` = cells^posdim 32-bit words = two u16 lane-half words in relu_masks' bit layout).  A pair's
 * decision then differs from its own pre-activation's sign only where a layer-2 kink crosses its cell (|x2| <= |grad x2| x 1.8e-3), the size of the
 * decision noise of the single-term bf16 product.  Handed to the backward as opts->mask_table / opts->mask_table_pmax. */
int smml_cpb_mask_table_cells(int posdim);
int smml_cpb_mask_table(const float* w1, const float* b1, const float* w2, const float* b2, unsigned short* table, int posdim, float pmax,
                        void* stream);
/* Table mode of the 16-bit core (csrc/deform_attn16.hip, "table mode"): the continuous position bias CPB(slog(gq - vs)) of
 * models/DeformableAttention2D.py:120-157 / DeformableAttention1D.py:60-102 is ONE function of the posdim signed-log offsets for every
 * pair of a launch, so the caller evaluates the MLP once on a grid - `table` [H / G, points^posdim] fp32, point (i0, i1) at index
 * i1 * points + i0 <-> p = -table_pmax + i * 2 table_pmax / (points - 1), points = smml_deform_attn_table_points(posdim) - and the
 * kernels interpolate it (bi)linearly per pair (positions beyond +-table_pmax take the edge value).  The backward returns
 * d table (the interpolation's adjoint: a histogram of d bias over the cells, fp32 atomics in LDS - the one order-dependent sum) in
 * place of the six parameter gradients, which follow from it through the table's own small backward; dq / dk / dv / dvs as in
 * smml_deform_attn16_bwd (fixed-order reductions).  grid_h, grid_w > 0 (posdim 2, grid_h * grid_w = N, both <= 128) assert that the
 * queries sit on a regular grid - gq[y * grid_w + x] = (X[x], Y[y]), as the 2-D module's do: the weight of a pair then factorises over
 * the axes and d table becomes two small dense products per key on the matrix pipe (no atomics: fixed-order sums); 0, 0 = any queries.
 * An additive mode: values differ from the per-pair MLP by the interpolation error
 * (tests/test_gpu_deform_table.py states the bounds); everything else - logits16 / dlogits16 layouts, dtype, dropout, events - as above. */
int smml_deform_attn_table_points(int posdim);
size_t smml_deform_attn_table_bwd_workspace_bytes(int B, int N, int J, int H, int posdim);
int smml_deform_attn_table_fwd(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* table,
                               float* out, float* lse, unsigned short* logits16, int B, int N, int J, int H, int G, int posdim,
                               int table_g, float table_pmax, float scale, float dropout_p, unsigned long long dropout_seed, int dtype,
                               void* ev_start, void* ev_stop, void* stream, const SmmlDeformOpts* opts);
int smml_deform_attn_table_bwd(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* table,
                               const float* out, const float* dout, const float* lse, const unsigned short* logits16,
                               unsigned short* dlogits16, float* dq, float* dk, float* dv, float* dvs, float* dtable, void* workspace,
                               size_t workspace_bytes, int B, int N, int J, int H, int G, int posdim, int table_g, float table_pmax,
                               int grid_h, int grid_w, float scale, float dropout_p, unsigned long long dropout_seed, int dtype,
                               void* ev_start, void* ev_stop, void* stream, const SmmlDeformOpts* opts);


/* attention dropout (nn.Dropout on the probabilities, DeformableAttention2D.py:309 / 1D :229): dropout_p in
 * [0, 1) and a 64-bit seed select a counter-based keep decision per (b, h, query, key); pass the same pair to
 * forward and backward.  The mask itself (0 / 1 floats [B, H, N, J]) is only materialised for tests: */
int smml_deform_attn_dropout_mask_f32(float* mask, int B, int N, int J, int H, float dropout_p,
                                      unsigned long long dropout_seed, void* stream, const SmmlDeformOpts* opts);

/* decision export (parity tests only): the ReLU decisions [W1 p + b1 > 0] of the position bias's FIRST layer
 * (DeformableAttention2D.py:129-131, 1D :69-71) bit for bit as the fused forward and the position-bias backward evaluate them,
 * masks [(B G), J, 2, smml_deform_attn_nst(N)] uint16 in the bit order of relu_masks above.  Together with relu_masks (layer 2)
 * and smml_bilinear_corners_f32 (the sampler's cells) this is every piecewise-linear decision of the module; tests impose
 * them on the fp64 oracle so that gradient comparisons do not depend on rounding-level ties. */
int smml_deform_attn_relu1_masks(const float* vs, const float* gq, const float* w1, const float* b1, unsigned short* masks,
                                 int B, int N, int J, int G, int posdim, void* stream, const SmmlDeformOpts* opts);

/* Attention maps (csrc/attn_maps.hip): where a fused deformable cross-attention call looked, from what its forward saved.  Input: the score
 * tiles logits_t [B, H, nst / 32, J, 32] fp32 and lse [B, H, N] of ANY fp32-grade forward above (pair, wide in its training form, region,
 * region_mh, region1d; not the fp16 tiles of the 16-bit cores).  The probabilities P[b, h, i, j] = exp(logits - lse) (natural base) are the
 * softmax BEFORE dropout (DeformableAttention2D.py:306-308, 1D :226-228); nothing of the forward is recomputed.
 *   key_mass [B, H, J] = (1 / N) sum_i P[b, h, i, j], always written; every row sums to 1
 *   attn     [B, H, N, J] = P, nullable (B H N J floats: small bags and tests)
 * One pass over logits_t (16 bytes per lane); the padding rows N .. nst - 1 of the last tiles never enter a sum.  The column sums go through
 * partial rows [B, H, ceil(ceil(N / 32) / 8), J] in `workspace` (smml_attn_maps_workspace_bytes bytes, 16-byte aligned; 0 for a non-positive
 * size; logits_t 16-byte aligned too) that a second kernel adds in ascending order: no float atomics, run-to-run identical. */
size_t smml_attn_maps_workspace_bytes(int B, int N, int J, int H);
int smml_attn_maps_f32(const float* logits_t, const float* lse, float* key_mass, float* attn, void* workspace, size_t workspace_bytes,
                       int B, int N, int J, int H, void* stream);
/* The mass on the patch grid (csrc/offsets.hip): per (bag, offset group) the mean of key_mass over the group's H / G heads, distributed to
 * the Hh x Ww map the keys were sampled from with the four corner weights and in-bounds masks of smml_bilinear_sample_fwd_f32 (the same
 * integer path: the adjoint of that gather).  Mass at corners outside the map is dropped as the sampler drops their features, so a map sums
 * to at most 1.  2-D positions only: vs [(B G), J, 2]; patch_map [B, G, Hh, Ww] is overwritten.  Additions in a fixed (key, corner) order per
 * pixel: no atomics, run-to-run identical.  Ww <= 8192. */
int smml_attn_splat_f32(const float* key_mass, const float* vs, float* patch_map, int B, int H, int G, int J, int Hh, int Ww, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Nystrom landmark self-attention, HBM-bound pieces (the contractions of models/NystromAttention.py:86,
 * 122-140 and the pinv iteration :20-35 run through smml_gemm_f32 with alpha / beta epilogues).
 * Row softmax over the last dim L of x [rows, L] (:137) and its backward dx = y (dy - sum(dy y)). */
int smml_softmax_fwd_f32(const float* x, float* y, long long rows, int L, void* stream);
int smml_softmax_bwd_f32(const float* y, const float* dy, float* dx, long long rows, int L, void* stream);
/* dst[b, r, c] = scale * src[b, c]: backward of the landmark segment mean (:102-118; the forward is
 * smml_colsum_f32 over [B*h*m, l, d] with scale 1/l). */
int smml_tile_rows_f32(const float* src, float* dst, long long nb, int R, int C, float scale, void* stream);
/* depthwise residual convolution along the tokens (:72,144-145): v [B, H, n, D], w [H, KW] ->
 * out_merged [B, n, H*D] (heads merged, the layout the output projection consumes). */
/* bf16-STORAGE forms of the n'-sized kernels of the block's bf16 compute mode; qkv / dqkv are the token-major bf16 buffers
 * [B, n, 3, H, D] the projection GEMM writes / its backward reads (n = m l).
 *   segment_mean: qmean, kmean fp32 [B, H, m, D] = landmark means of q and of k (models/NystromAttention.py:102-118)
 *   segment_mean_bwd_add: dqkv(q, k parts) += (dqmean, dkmean) broadcast / l
 *   resconv: 33-tap depthwise convolution over tokens (:62-66,144-145); element (b, t, h, d) of in at b i_bs + t i_rs + h D + d (elements),
 *            of out at b o_bs + t o_rs + h D + d; flip = 1 applies the reversed taps (gradient w.r.t. the input)
 *   resconv_wgrad: dw fp32 [H, 33] += sum dout[b, t, h, d] v[b, t + k - 16, h, d] */
int smml_segment_mean_b16(const void* qkv, float* qmean, float* kmean, int B, int n, int l, int H, int D, void* stream);
int smml_segment_mean_bwd_add_b16(void* dqkv, const float* dqmean, const float* dkmean, int B, int n, int l, int H, int D, void* stream);
int smml_resconv_b16(const void* in, const float* w, void* out, int B, int H, int n, int D, int KW, long long i_bs, long long i_rs,
                     long long o_bs, long long o_rs, int flip, void* stream);
int smml_resconv_wgrad_b16(const void* dout, const void* v, float* dw, int B, int H, int n, int D, int KW, long long g_bs, long long g_rs,
                           long long v_bs, long long v_rs, void* stream);

/* Newton-Schulz pseudo-inverse iteration (models/NystromAttention.py:28-33; dup cmta_utils.py:152-157), `iters` times, on NB problems of
 * m x m (row-major, contiguous): z <- 1/4 z (13 I - x z (15 I - x z (7 I - x z))).  One host call issues the whole chain of batched
 * products (4 per iteration forward, 8 + one update backward) on `stream`.  reduced != 0: the caller accepts products with 16-bit
 * mantissas (the block's 16-bit compute mode; m = 256 then runs as two bf16 planes per matrix on the 16-bit matrix pipe); reduced = 0:
 * exact fp32 products.  The forward and the backward of one call take the same `reduced`.
 * fwd: saved (smml_newton_schulz_saved_floats floats) receives what the backward needs of every iteration; z_out [NB, m, m] = the result.
 * bwd: dx, dz0 [NB, m, m] overwritten; scratch = smml_newton_schulz_scratch_floats floats.  All buffers 16-byte aligned. */
size_t smml_newton_schulz_saved_floats(int NB, int m, int iters, int reduced);     /* sizes, in floats, of `saved` and `scratch` below */
size_t smml_newton_schulz_scratch_floats(int NB, int m, int iters, int reduced);
/* measurement / test switch: 0 every product through smml_gemm_f32; 1 the exact-fp32 chain kernel for m = 256 whatever `reduced`; 2 (default) */
void smml_newton_schulz_set_fast(int on);
int smml_newton_schulz_fwd(const float* x, const float* z0, float* saved, float* z_out, int NB, int m, int iters, int reduced, void* stream);
int smml_newton_schulz_bwd(const float* x, const float* z0, const float* saved, const float* dz_in, float* dx, float* dz0,
                           float* scratch, int NB, int m, int iters, int reduced, void* stream);

int smml_resconv_fwd_f32(const float* v, const float* w, float* out_merged, int B, int H, int n, int D, int KW,
                         void* stream);
/* dv [B, H, n, D] overwritten, dw [H, KW] accumulated into */
int smml_resconv_bwd_f32(const float* dout_merged, const float* v, const float* w, float* dv, float* dw, int B, int H,
                         int n, int D, int KW, void* stream);
/* PPEG (models/mil.py:192-206): depthwise 7x7 + 5x5 + 3x3 + identity as ONE merged 7x7 depthwise pass on
 * channel-last maps x [B, H, W, C]; wm [C, 49]; flip = 1 applies the rotated kernel (data gradient). */
int smml_dwconv7_fwd_f32(const float* x, const float* wm, const float* bias, float* y, int B, int H, int W, int C, int flip,
                         void* stream);
/* dwm [C, 49], db [C] accumulated into */
int smml_dwconv7_bwd_weight_f32(const float* x, const float* dy, float* dwm, float* db, int B, int H, int W, int C,
                                void* stream);

/* ------------------------------------------------------------------------------------------------
 * Train-step glue: the gradient-modulation block of the reference's training loop,
 * train_test.py:87-184 (task types diag2021 / grade / subtype; 'survival' below), as one launch with no host synchronisation:
 * per-branch logits feat_x W_x^T + b / 2, score_x = sum_b softmax(.)[label_b], ratio_t = score_t / score_i, and for
 * every class row of classifier.weight.grad [C, 2 hs] whose tumor / immune halves have negative cosine similarity the
 * projection + renormalisation of the weaker branch's half (:158-183), IN PLACE in weight_grad.
 *   feat_t, feat_i [B, hs]   weight [C, 2 hs]   bias [C]   label [B] int64   weight_grad [C, 2 hs]
 *   info (nullable) [4 + 2 C]: score_t, score_i, ratio_t, ratio_i, then (cosine similarity, branch taken 0 / 1 / 2) per row. */
int smml_grad_modulate_f32(const float* feat_t, const float* feat_i, const float* weight, const float* bias,
                           const long long* label, float* weight_grad, float* info, int B, int C, int hs, void* stream);
/* task_type 'survival' of the same block (train_test.py:99-102,121-149): the two branch scores are the concordance indices of
 * risk_b = -sum_t cumprod_t (1 - sigmoid(out_b)) against (censor, survtime) - what the reference obtains on the host from scikit-survival's
 * concordance_index_censored(event = 1 - censor, survtime, risk, tied_tol = 1e-8) (utils/utils.py:315-317): a sample with an event is
 * comparable with every sample of later time and with every sample censored at the same time; concordant if its risk is larger, tied within
 * 1e-8 counts one half.  censor, survtime [B] fp32 (censor 1 = censored).  All samples censored (:127-133) or no comparable pair: no edit.
 * info[0..1] = cindex_t, cindex_i, the rest as above.  scikit-survival is absent from the build image: parity of this entry is unpinned. */
int smml_grad_modulate_survival_f32(const float* feat_t, const float* feat_i, const float* weight, const float* bias,
                                    const float* censor, const float* survtime, float* weight_grad, float* info, int B, int C, int hs,
                                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * Data-format step in front of the path: bags stored as packed bf16 rows, resampled to the fixed
 * instance count on the device by the reference's index rule (data/dataset.py:151-175: i mod n when the bag is short,
 * int(np.around(i * (n / fixdim))) when it is long - IEEE double, round-half-even; bit-exact integer path).
 *   src [n_rows, dim] bf16 (as uint16)   dst [fixdim, dim] fp32 (out_is_f32 != 0) or bf16; dim % 8 == 0, 16-byte aligned.
 * smml_fixdim_indices writes the fixdim source-row indices alone (int64), for the bit-exactness tests. */
int smml_fixdim_indices(long long* out, long long n_rows, long long fixdim, void* stream);
int smml_fixdim_gather_bf16(const unsigned short* src, long long n_rows, void* dst, int out_is_f32, long long fixdim, int dim,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused softmax attention on the 16-bit matrix pipe: O = softmax(scale Q K^T) V with fp32 storage, bf16 (use_fp16 = 0) or
 * fp16 (use_fp16 = 1) operands converted on the fly and fp32 accumulation; the [Lq, Lk] probability matrix is never written
 * (forward keeps one base-2 log-sum-exp per query in lse2, backward recomputes).  Serves the two attention-shaped products of
 * the Nystrom block in its 16-bit compute mode (models/NystromAttention.py:122-140): softmax(q kl^T) (z (attn3 v)) with
 * (Lq, Lk) = (n', m) and softmax(ql k^T) v with (Lq, Lk) = (m, n').
 *   q [BH, Lq, 64]   k, v [BH, Lk, 64]   dq [BH, Lq, 64]   dk, dv [BH, Lk, 64]   lse2 [BH, Lq]   (D must be 64)
 *   out / dout: head-major [BH, Lq, 64] (heads_merged = 0) or heads merged [BH / H, Lq, H * 64] (heads_merged = H: the layout
 *   the block's output projection consumes).  accumulate != 0: out += result (out already holds the residual convolution of
 *   v, :144-145); the backward then takes that residual (same layout, nullable) to recover the attention output.
 * Backward: dq / dk / dv overwritten; workspace of smml_attn16_bwd_workspace_bytes(...) bytes, 16-byte aligned. */
size_t smml_attn16_fwd_workspace_bytes(int BH, int Lq, int Lk);   /* 0 unless the shape runs key-split (few queries, many keys) */
int smml_attn16_fwd_f32(const float* q, const float* k, const float* v, float* out, float* lse2, void* workspace,
                        size_t workspace_bytes, int BH, int Lq, int Lk, int D, float scale, int use_fp16, int heads_merged,
                        int accumulate, void* stream);
/* forward kernel choice for Lk <= 256 (measurement / test hook): 0 (default) = always the online-softmax kernel, 1 = the two-pass
 * kernel with all keys resident in LDS wherever its 256-query workgroups fill the chip, 2 = wherever Lk <= 256.  The two-pass kernel
 * halves the vector instructions per MFMA but the launch is HBM-bound with fp32 storage (csrc/attn16.hip). */
void smml_attn16_set_fewkeys(int mode);
/* queries-long bf16-storage forward (smml_attn16_fwd_b16, long_side 1): 0 = one 32-query block per wave, 1 (default) = two blocks per wave
 * (the K / V fragments of a tile feed two accumulator sets: half the LDS fragment reads, barriers and K / V staging per MFMA) wherever the
 * 256-query workgroups still cover the chip twice over, 2 = always (test / measurement switch). */
void smml_attn16_set_query_blocks(int mode);
/* bf16-STORAGE forms of the two attention-shaped products (bf16 compute mode with bf16 bags): the LONG side (long_side 0: keys / values -
 * softmax(ql k^T) v; 1: queries - softmax(q kl^T) w) is bf16 in memory at element strides (s_bs, s_hs, s_rs) per (bag, head, row) - q / k / v
 * are read in the token-major [b, n', 3, h, 64] buffer the projection wrote - the short (landmark) side is fp32 [B H, L, 64].
 *   long_side 0: q fp32, k / v bf16, out fp32 [B H, Lq, 64]; residual must be NULL
 *   long_side 1: q bf16, k / v fp32, out = attention + residual, both bf16 at strides (o_bs, o_hs, o_rs) (residual may be NULL)
 * Backward: gradients of the long side are bf16 at strides (g_bs, g_hs, g_rs) (e.g. inside the gradient of the qkv buffer), those of the
 * short side fp32.  long_side 0: dout / out fp32, dq fp32, dk written, dv written or added to (dv_accumulate);
 * long_side 1: out / residual / dout bf16 at the o strides, dq bf16 written, dk / dv fp32.  Workspaces as for the fp32-storage entries. */
int smml_attn16_fwd_b16(const void* q, const void* k, const void* v, void* out, const void* residual, float* lse2, void* workspace,
                        size_t workspace_bytes, int B, int H, int Lq, int Lk, float scale, int long_side, long long s_bs, long long s_hs,
                        long long s_rs, long long o_bs, long long o_hs, long long o_rs, void* stream);
int smml_attn16_bwd_b16(const void* q, const void* k, const void* v, const void* out, const void* residual, const void* dout,
                        const float* lse2, void* dq, void* dk, void* dv, void* workspace, size_t workspace_bytes, int B, int H, int Lq,
                        int Lk, float scale, int long_side, long long s_bs, long long s_hs, long long s_rs, long long o_bs, long long o_hs,
                        long long o_rs, long long g_bs, long long g_hs, long long g_rs, int dv_accumulate, void* stream);
size_t smml_attn16_bwd_workspace_bytes(int BH, int Lq, int Lk);
int smml_attn16_bwd_f32(const float* q, const float* k, const float* v, const float* out, const float* residual, const float* dout,
                        const float* lse2, float* dq, float* dk, float* dv, void* workspace, size_t workspace_bytes, int BH, int Lq,
                        int Lk, int D, float scale, int use_fp16, int heads_merged, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Attention pooling of ABMIL (models/mil.py:66-75: the second attention layer, transpose, softmax over the bag, bmm with the raw features):
 *   s[b, n] = h[b, n, :] . w2 + b2      out[b, :] = sum_n softmax_n(s[b, :])[n] x[b, n, :]      lse[b] = log sum_n exp(s[b, n])
 * with h = tanh(x W1^T + b1) formed by smml_gemm_f32 (act 2).  One streaming pass over x and h with an online softmax: the bag's rows are cut
 * into splits, each split leaves one partial (max, sum, accumulator [L]) in the workspace and a second kernel merges a bag's partials in
 * ascending split order - no float atomics, one form, deterministic by construction.
 *   x [B, N, L]   h [B, N, D]   w2 [D]   b2 [1] (in device memory, like w2)   s [B, N]   out [B, L]   lse [B];
 *   any N >= 1, L a multiple of 256 up to 1024, D a multiple of 64 up
 *   to 256 (anything else is an error); x, out, dout and the workspaces 16-byte aligned.
 * splits: rows are cut into ceil(N / ceil(N / splits)) splits; 0 = chosen by the library (about 1024 workgroups over the B bags, no split
 * under 48 rows).  The workspace functions take the same value.
 * Backward, for dout [B, L] and the saved s, lse: t[b, n] = dout . x[b, n, :], p = exp(s - lse) / sum_n exp(s - lse) (the sum is re-formed:
 * lse carries a rounding of |lse| 2^-24), c[b] = sum_n p t (= dout . out; formed from the row dots and kept in fp64 up to t - c, so that sum_n ds
 * cancels to the rounding of its terms), ds = p (t - c); dh [B, N, D] = ds w2 (tanh_grad = 0: the gradient of h) or ds w2 (1 - h^2) (tanh_grad = 1: the gradient of
 * the hidden layer's pre-activation, from which dW1 and db1 follow by smml_gemm_f32 and smml_colsum_f32), dw2 [D] = sum ds h and
 * db2 [1] = sum ds, all overwritten; the row dots and the workgroups' dw2 / db2 partials go to the workspace, the partials are added in a
 * fixed order.  No gradient of x is formed. */
size_t smml_attn_pool_fwd_workspace_bytes(int B, int N, int L, int splits);
int smml_attn_pool_fwd_f32(const float* x, const float* h, const float* w2, const float* b2, float* s, float* out, float* lse, void* workspace,
                           size_t workspace_bytes, int B, int N, int L, int D, int splits, void* stream);
size_t smml_attn_pool_bwd_workspace_bytes(int B, int N, int D, int splits);
int smml_attn_pool_bwd_f32(const float* x, const float* h, const float* w2, const float* s, const float* lse, const float* dout, float* dh,
                           float* dw2, float* db2, void* workspace, size_t workspace_bytes, int B, int N, int L, int D, int splits,
                           int tanh_grad, void* stream);

/* The gated form (GatedABMIL, models/mil.py:102-152; the attention head of CLAM and of MCAT's Attn_Net_Gated):
 *   s[b, n] = sum_d w[d] hv[b, n, d] hu[b, n, d] + b      with hv = tanh(x Wv^T + bv), hu = sigmoid(x Wu^T + bu)
 * and everything after the score - online softmax, partials, merge, row dots, fixed-order reductions - as above.  The two hidden tensors are
 * ONE buffer h2 [B, N, 2 D]: columns [0, D) hold hv and columns [D, 2 D) hold hu, as smml_gemm_f32 writes them with act 4 from the stacked
 * weight [Wv; Wu].  D is the width of ONE half (a multiple of 64 up to 256); w [D], b [1]; the other shapes, the alignment rules, `splits`
 * and the workspaces are those of the plain entry points: size them with smml_attn_pool_fwd_workspace_bytes(B, N, L, splits) and
 * smml_attn_pool_bwd_workspace_bytes(B, N, D, splits).
 * Backward, with ds as above and g = ds w[d]: dh2 [B, N, 2 D] holds g hu | g hv (act_grad = 0: the gradient of h2) or
 * g hu (1 - hv^2) | g hv hu (1 - hu) (act_grad = 1: the gradient of the stacked pre-activation, from which d[Wv; Wu] and d[bv; bu] follow by
 * one smml_gemm_f32 and one smml_colsum_f32), dw [D] = sum ds hv hu, db [1] = sum ds, all overwritten. */
int smml_attn_pool_gated_fwd_f32(const float* x, const float* h2, const float* w, const float* b, float* s, float* out, float* lse,
                                 void* workspace, size_t workspace_bytes, int B, int N, int L, int D, int splits, void* stream);
int smml_attn_pool_gated_bwd_f32(const float* x, const float* h2, const float* w, const float* s, const float* lse, const float* dout,
                                 float* dh2, float* dw, float* db, void* workspace, size_t workspace_bytes, int B, int N, int L, int D,
                                 int splits, int act_grad, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Few-query co-attention (models/MultiheadAttention.py with one head and L <= 8 queries over S keys: CMTA's G_in_P_Att, MCAT's coattn), the
 * bag-sized core of the folded form.  With q^ = (query Wq^T + bq) scaling, u = q^ Wk and c = q^ . bk (formed by the caller, [B, L, E]-sized):
 *   raw[b, l, s] = u[b, l, :] . x[b, s, :] + c[b, l]      z[b, l, :] = sum_s softmax_s(raw[b, l, :])[s] y[b, s, :]      lse[b, l] = log sum_s exp(raw)
 * and the module's output is (z Wv^T + bv) Wo^T + bo.  One streaming pass over x (and y) with one online softmax per query; the bag's rows
 * are cut into splits as for smml_attn_pool_*, one partial (m[L], l[L], acc[L, Ev]) per split, merged in ascending split order - no float
 * atomics, one form, deterministic by construction.
 *   u [B, L, Ek]   c [B, L]   z [B, L, Ev]   raw [B, L, S]   lse [B, L]   dense;
 *   x [B, S, Ek], y [B, S, Ev]: unit column stride, rows *_row_stride and bags *_batch_stride floats apart (multiples of 4; a slice or a
 *   sequence-first tensor is read in place).  y may BE x (same pointer, strides and width, as at every call site of the reference): the rows
 *   are then read once.  key_padding_mask [B, S] bytes (non-zero: the key is masked, its raw score is -inf) or null.
 *   L <= 8, Ek and Ev multiples of 64 up to 512, any S >= 1 (anything else is an error); u, x, y, z, dz, dx, dy and the workspaces 16-byte
 *   aligned.  A bag whose keys are ALL masked gives NaN, as in the reference; that is not checked.
 * splits: as for smml_attn_pool_fwd_f32 (0 = about 1024 workgroups over the B bags, no split under 64 rows).
 * Backward, for dz [B, L, Ev], the saved raw, lse, z and optionally draw [B, L, S] (the gradient of the raw scores) and dlse [B, L] (either
 * may be null): p = exp(raw - lse), t = dz . y_s, kappa = dz . z, ds = p (t - kappa + dlse) + draw (0 at masked keys);
 *   du [B, L, Ek] = sum_s ds x_s   dc [B, L] = sum_s ds   dx [B, S, Ek] = sum_l ds u_l   dy [B, S, Ev] = sum_l p dz_l   all overwritten,
 * dx and dy with strides of their own.  dx and dy may be null (nothing is formed for them); where y is x the one row dx + dy goes to dx and
 * dy must be null.  The workgroups' du / dc partials go to the workspace and are added in ascending split order. */
size_t smml_fewq_attn_fwd_workspace_bytes(int B, int L, int S, int Ev, int splits);
int smml_fewq_attn_fwd_f32(const float* u, const float* c, const float* x, const float* y, const unsigned char* key_padding_mask, float* z,
                           float* raw, float* lse, void* workspace, size_t workspace_bytes, int B, int L, int S, int Ek, int Ev,
                           long long x_batch_stride, long long x_row_stride, long long y_batch_stride, long long y_row_stride, int splits,
                           void* stream);
size_t smml_fewq_attn_bwd_workspace_bytes(int B, int L, int S, int Ek, int splits);
int smml_fewq_attn_bwd_f32(const float* u, const float* x, const float* y, const float* raw, const float* lse, const float* z, const float* dz,
                           const float* draw, const float* dlse, float* du, float* dc, float* dx, float* dy, void* workspace,
                           size_t workspace_bytes, int B, int L, int S, int Ek, int Ev, long long x_batch_stride, long long x_row_stride,
                           long long y_batch_stride, long long y_row_stride, long long dx_batch_stride, long long dx_row_stride,
                           long long dy_batch_stride, long long dy_row_stride, int splits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Few-key co-attention (the same module with a bag of L queries over S <= 8 keys: CMTA's P_in_G_Att), the dual problem: the projections fold
 * onto the keys.  With k^ = key Wk^T + bk and v^ = value Wv^T + bv, u = scaling k^ Wq, c = scaling k^ . bq and w = v^ Wo^T + bo (formed by the
 * caller, [B S, E]-sized):
 *   raw[b, l, j] = x[b, l, :] . u[b, j, :] + c[b, j]      out[b, l, :] = sum_j softmax_j(raw[b, l, :])[j] w[b, j, :]
 * and out IS the module's output (bo folds into w because the weights of a row sum to one).  One streaming pass over the rows of x: S dot
 * products, a softmax over S numbers and a weighted sum of S rows per row; no sum crosses rows in the forward.
 *   x [B, L, Eq]: unit column stride, rows x_row_stride and bags x_batch_stride floats apart (multiples of 4; a slice or a sequence-first
 *   tensor is read in place)   u [B, S, Eq]   c [B, S]   w [B, S, Eo]   out [B, L, Eo]   raw [B, L, S]   dense.
 *   key_padding_mask [B, S] bytes (non-zero: the key is masked, its raw score is -inf) or null; a bag whose keys are ALL masked gives NaN, as
 *   in the reference.  1 <= S <= 8, Eq and Eo multiples of 64 up to 512, any L >= 1 (anything else is an error, nothing is launched); x, u,
 *   w, out, dout, dx and the workspace 16-byte aligned.
 * splits: as for smml_fewq_attn_fwd_f32 (0 = about 1024 workgroups over the B bags, no split under 64 rows, whole tiles of 16 rows); the
 * forward's result does not depend on it and its workspace is empty (the size function and the two arguments mirror the few-query entry).
 * Backward, for dout (rows of width Eo, strides of their own), the saved raw and optionally draw [B, L, S] (the gradient of the raw scores;
 * null: none arrived): p = softmax(raw), dp = dout . w_j, g = p (dp - sum_j p dp) + draw (0 at masked keys);
 *   dx [B, L, Eq] = sum_j g u_j (strides of its own; null: nothing is formed)   du [B, S, Eq] = sum_l g x_l   dc [B, S] = sum_l g
 *   dw [B, S, Eo] = sum_l p dout_l      all overwritten.
 * The workgroups' du / dc / dw partials go to the workspace and are added in ascending split order: no float atomics, the result is a
 * function of the inputs and `splits` alone. */
size_t smml_fewk_attn_fwd_workspace_bytes(int B, int L, int S, int Eo, int splits);
int smml_fewk_attn_fwd_f32(const float* x, const float* u, const float* c, const float* w, const unsigned char* key_padding_mask, float* out,
                           float* raw, void* workspace, size_t workspace_bytes, int B, int L, int S, int Eq, int Eo, long long x_batch_stride,
                           long long x_row_stride, int splits, void* stream);
size_t smml_fewk_attn_bwd_workspace_bytes(int B, int L, int S, int Eq, int Eo, int splits);
int smml_fewk_attn_bwd_f32(const float* x, const float* u, const float* w, const float* raw, const float* dout, const float* draw, float* dx,
                           float* du, float* dc, float* dw, void* workspace, size_t workspace_bytes, int B, int L, int S, int Eq, int Eo,
                           long long x_batch_stride, long long x_row_stride, long long dout_batch_stride, long long dout_row_stride,
                           long long dx_batch_stride, long long dx_row_stride, int splits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sets of at most 8 tokens (MCAT_Surv after its co-attention, models/model.py:589-651: nn.TransformerEncoder with 8 heads over the 4 genomic
 * tokens, then Attn_Net_Gated + softmax + bmm).  A token set is a few KB and its cost is launches: every entry point below is ONE launch, with no
 * workspace and no float atomics - the results are a function of the inputs alone.
 *
 * Self-attention from a packed projection.  qkv holds the rows [q | k | v] of width 3 E of (sample b, token t) at
 * qkv + b qkv_batch_stride + t qkv_token_stride (floats, multiples of 4, tokens at least 3 E apart: the sequence-first [T, B, 3 E] output of one
 * smml_gemm_f32 is read in place, a batch-first one as well); head h of H reads columns [h hd, (h + 1) hd) of each third, hd = E / H.
 *   S = scale Q K^T   P = softmax_rows(S) (the row maximum is subtracted)   O = (P keep) V
 *   o: rows of width E with the heads merged, at o + b o_batch_stride + t o_token_stride   p [B, H, T, T] dense: the softmax BEFORE keep
 *   keep [B, H, T, T] dense or null: float multipliers of attention dropout, 0 or 1 / (1 - rate), drawn by the caller.  A row whose keep is all
 *   zero gives a zero output row and zero score gradients.
 *   1 <= T <= 8, E a multiple of 64 up to 512, hd 32 or 64, any B >= 1 (anything else is an error, nothing is launched); qkv, o, dout, dqkv
 *   16-byte aligned.
 * Backward, for dout (rows of width E, strides of their own), the saved p and the same keep:
 *   dV = (P keep)^T dO   dP = (dO V^T) keep   dS = P (dP - rowsum(dP P))   dQ = scale dS K   dK = scale dS^T Q
 * written as rows [dq | dk | dv] into dqkv (strides of its own, every element overwritten). */
int smml_token_attn_fwd_f32(const float* qkv, const float* keep, float* o, float* p, int B, int T, int E, int H, long long qkv_batch_stride,
                            long long qkv_token_stride, long long o_batch_stride, long long o_token_stride, float scale, void* stream);
int smml_token_attn_bwd_f32(const float* qkv, const float* keep, const float* p, const float* dout, float* dqkv, int B, int T, int E, int H,
                            long long qkv_batch_stride, long long qkv_token_stride, long long dout_batch_stride, long long dout_token_stride,
                            long long dqkv_batch_stride, long long dqkv_token_stride, float scale, void* stream);

/* Gated attention pooling over a token set, WITH the gradient of the pooled rows (smml_attn_pool_gated_* pools a bag of features and forms none).
 *   s[b, t] = sum_d w[d] hv[b, t, d] hu[b, t, d] + b      a[b, :] = softmax_t(s[b, :])      out[b, :] = sum_t a[b, t] x[b, t, :]
 *   x: rows of width E at x + b x_batch_stride + t x_token_stride (as qkv above, tokens at least E apart)   h2 [B, T, 2 D] dense, the layout of
 *   smml_attn_pool_gated_*: columns [0, D) hold hv (tanh), columns [D, 2 D) hold hu (sigmoid)   w [D]   b [1] (device memory)
 *   s [B, T]   a [B, T]   out [B, E]
 *   1 <= T <= 8, E a multiple of 64 up to 512, D a multiple of 64 up to 256, any B >= 1 (anything else is an error, nothing is launched);
 *   x, h2, w, out, dout, dx, dh2 16-byte aligned.
 * Backward, for dout [B, E] and the saved a: tau[b, t] = dout[b] . x[b, t], ds = a (tau - sum_t a tau) (the dots and their mean are kept in
 * fp64 up to the difference: the tokens of a set can lie close together, and tau - sum_t a tau then cancels to a few digits);
 *   dx[b, t, :] = a[b, t] dout[b, :] (strides of its own)   dh2 [B, T, 2 D] = ds w hu | ds w hv (the gradient of h2)
 *   dw [D] = sum_{b, t} ds hv hu   db [1] = sum_{b, t} ds      all overwritten.
 * dw and db are formed by ONE workgroup of the launch, which re-forms ds of every sample and adds in a fixed order (four interleaved ascending
 * runs over the samples, then the four runs in order); the other workgroups own one sample's dx and dh2 each. */
int smml_token_pool_gated_fwd_f32(const float* x, const float* h2, const float* w, const float* b, float* s, float* a, float* out, int B, int T,
                                  int E, int D, long long x_batch_stride, long long x_token_stride, void* stream);
int smml_token_pool_gated_bwd_f32(const float* x, const float* h2, const float* w, const float* a, const float* dout, float* dx, float* dh2,
                                  float* dw, float* db, int B, int T, int E, int D, long long x_batch_stride, long long x_token_stride,
                                  long long dx_batch_stride, long long dx_token_stride, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Self-normalising encoder stacks (SNN_Block, models/mcat_utils.py:81-95: the sig_networks of MCAT_Surv and CMTA; MaxNet's encoder,
 * models/model.py:142-187): G independent networks (1 <= G <= 8) of `depth` layers each (1 <= depth <= 4, the same for every network), all of
 * them in ONE forward launch and TWO backward launches.  Layer l = 1 .. depth of network g:
 *   z_l = a_{l-1} W_l^T + b_l        W_l [N_l, K_l] row-major (nn.Linear's), K_l = N_{l-1}, a_0 = x_g [B, K_0]
 *   e_l = z_l > 0 ? z_l : expm1(z_l)                                                     (ELU, alpha = 1)
 *   a_l = e_l (keep null) or A keep e_l + A alpha' (keep - 1) + A alpha' p               (torch's AlphaDropout for the 0 / 1 tensor keep;
 *                                                                                         alpha' = 1.7580993408473766, A = ((alpha'^2 p + 1)(1 - p))^-1/2)
 *   out_g [B, N_depth] = final_relu ? max(a_depth, 0) : a_depth
 * 1 <= K_0 <= 2048, 1 <= N_l <= 256, any B >= 1, no width needs to be a multiple of anything and no pointer an alignment (anything else is an
 * error, nothing is launched).
 * The per-network and per-layer device addresses travel as HOST arrays of 64-bit addresses, widths, strides and offsets as HOST arrays; the
 * entry point reads them during the call into the kernels' by-value argument - no device allocation, no copy, nothing is retained:
 *   x [G]: the base of network g's input; its rows start x_col_offset[g] floats into rows x_row_stride[g] floats apart (unit column stride): a
 *          column range of a wider [B, sum K] tensor is read in place
 *   W, b [G depth]: entry g depth + l - 1 is W_l, b_l of network g          widths [G (depth + 1)]: K_0, N_1 .. N_depth of network g
 *   out [G]: dense [B, N_depth] each (they may be the slices of one [G, B, N] buffer)
 * acts (device, B sum_{g, l} N_l floats): every e_l, dense [B, N_l] blocks in the order g = 0 .. G - 1, within g l = 1 .. depth; keep (device,
 * the same layout, 0 or 1; required with p > 0, null with p = 0) and the backward's scratch dz (device, the same layout and size, every
 * element written: dz_l = da_l . A keep . (e_l > 0 ? 1 : e_l + 1)) share it.
 * Backward, for dout [G] (dense [B, N_depth] each; 0: no gradient arrived for that network): the final ReLU's mask is taken from out (needed
 * with final_relu only), da_{l-1} = dz_l W_l;
 *   dW [G depth]: dW_l [N_l, K_l] = dz_l^T a_{l-1}      db [G depth]: db_l [N_l] = sum_b dz_l      one separately allocated buffer per parameter,
 *   dx [G] (the table may be null, an entry 0: not formed): dense [B, K_0]
 * all overwritten; each element has one owner, which adds over the rows b = 0 .. B - 1 in that order (dW, db) or over n ascending (da, dx): no
 * float atomics, the results are a function of the inputs alone. */
int smml_snn_stack_fwd_f32(const unsigned long long* x, const long long* x_row_stride, const long long* x_col_offset, const unsigned long long* W,
                           const unsigned long long* b, const int* widths, const float* keep, float* acts, const unsigned long long* out, int G,
                           int depth, int B, float p, int final_relu, void* stream);
int smml_snn_stack_bwd_f32(const unsigned long long* x, const long long* x_row_stride, const long long* x_col_offset, const unsigned long long* W,
                           const int* widths, const float* keep, const float* acts, const unsigned long long* out, const unsigned long long* dout,
                           float* dz, const unsigned long long* dW, const unsigned long long* db, const unsigned long long* dx, int G, int depth,
                           int B, float p, int final_relu, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMML_H_ */
