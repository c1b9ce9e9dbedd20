// Grouped 1x1 convolution on token-major data, 16 input and 64 output channels per group (to_q / to_k / to_v of the deformable
// attention modules at dim 128):   y[m, 64 g + o] = sum_i x[m, 16 g + i] w[64 g + o, i]      x [rows, 16 G], w [64 G, 16], y [rows, 64 G]
// and its two gradients.  Each of the three is a streaming pass: the MFMA work is a few microseconds chip-wide, the operands are
// rows * (16 G + 64 G) * 4 bytes, so the kernels are laid out for HBM pace and nothing else:
//   * one wave owns one group and strides over 32-row tiles; the eight waves of a workgroup together read and write FULL rows
//     (G = 8: 512-byte rows of x, 2 KB rows of y), each row exactly once;
//   * the weight fragment of a wave's group lives in registers for the whole launch (forward 16, dX 32 values per lane): no LDS, no barrier;
//   * the row operand is loaded from global memory directly in MFMA fragment layout (lane (c, hf) = row c, k slot hf reads 32 contiguous
//     bytes of its row per 16 k values), one tile ahead of the MFMAs that consume it.
// Forward and dX reproduce the batched route through smml_gemm_f32 BIT FOR BIT: the same instruction (v_mfma_f32_32x32x2_f32), the same
// k index in the same k slot of the same step (step st of K tile kt multiplies k = 16 kt + 8 hf + st), K tiles ascending, one accumulator
// chain per output element starting from +0.  dX therefore keeps the 32-column instruction with 16 live columns, as the batched route has.
// dW is one pass over dy and x: every workgroup sums its rows into one [G, 64, 16] partial (plain stores into the caller's workspace), a
// second kernel adds the partials in a fixed order.  No zero fill, no float atomics: the result is a fixed function of the operands.
#include "smml_common.h"

namespace {

constexpr int GPW_CIN = 16, GPW_COUT = 64;     // channels per group
constexpr int GPW_WAVES = 8;                   // waves (= groups) per workgroup
constexpr int GPW_GRID = 512;                  // row-striding workgroups per group block: two resident per CU on 256 CUs
constexpr int GPW_DW_STEP = 16;                // rows per dW step (eight 2-row MFMA steps)
constexpr int GPW_DW_GRID = 256;               // dW workgroups (sixteen waves each) per group block: one per CU
constexpr int GPW_SEG = 32;                    // segments of the dW partial sum

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

__global__ __launch_bounds__(512, 4) void grouped_pointwise_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                    float* __restrict__ y, long long rows, int G) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 31, hf = lane >> 5;
  const int g = blockIdx.y * GPW_WAVES + wave;
  if (g >= G) return;                                        // (no barrier anywhere in this kernel)
  const long long Cin = (long long)GPW_CIN * G, Cout = (long long)GPW_COUT * G;
  float bf[2][8];                                            // B fragment: output channel 32 nb + c, k = 8 hf + st
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    const float* p = w + ((long long)g * GPW_COUT + 32 * nb + c) * GPW_CIN + 8 * hf;
    const float4 u = ld4(p), v = ld4(p + 4);
    bf[nb][0] = u.x; bf[nb][1] = u.y; bf[nb][2] = u.z; bf[nb][3] = u.w;
    bf[nb][4] = v.x; bf[nb][5] = v.y; bf[nb][6] = v.z; bf[nb][7] = v.w;
  }
  const long long ntiles = (rows + 31) / 32;
  const float* xg = x + GPW_CIN * g + 8 * hf;
  float* yg = y + GPW_COUT * g + c;
  float4 n0, n1;
  long long t = blockIdx.x;
  if (t < ntiles) { const float* p = xg + min(t * 32 + c, rows - 1) * Cin; n0 = ld4(p); n1 = ld4(p + 4); }
  for (; t < ntiles; t += gridDim.x) {
    const float af[8] = {n0.x, n0.y, n0.z, n0.w, n1.x, n1.y, n1.z, n1.w};
    const long long tn = t + gridDim.x;
    if (tn < ntiles) { const float* p = xg + min(tn * 32 + c, rows - 1) * Cin; n0 = ld4(p); n1 = ld4(p + 4); }   // in flight during the MFMAs
    floatx16 acc0 = {0}, acc1 = {0};
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      acc0 = mfma32(af[st], bf[0][st], acc0);
      acc1 = mfma32(af[st], bf[1][st], acc1);
    }
    const long long mb = t * 32;
    if (mb + 32 <= rows) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float* q = yg + (mb + acc_row(r, hf)) * Cout;
        q[0] = acc0[r];
        q[32] = acc1[r];
      }
    } else {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long m = mb + acc_row(r, hf);
        if (m < rows) { yg[m * Cout] = acc0[r]; yg[m * Cout + 32] = acc1[r]; }
      }
    }
  }
}

__global__ __launch_bounds__(512, 4) void grouped_pointwise_dx_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                   float* __restrict__ dx, long long rows, int G) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, c = lane & 31, hf = lane >> 5;
  const int g = blockIdx.y * GPW_WAVES + wave;
  if (g >= G) return;
  const long long Cin = (long long)GPW_CIN * G, Cout = (long long)GPW_COUT * G;
  float bf[4][8];                                            // B fragment: input channel c (16 live columns), k = output channel 16 kt + 8 hf + st
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int st = 0; st < 8; ++st) {
      const float v = w[((long long)g * GPW_COUT + 16 * kt + 8 * hf + st) * GPW_CIN + (c & 15)];
      bf[kt][st] = c < GPW_CIN ? v : 0.f;
    }
  const long long ntiles = (rows + 31) / 32;
  const float* dyg = dy + GPW_COUT * g + 8 * hf;
  float* dxg = dx + GPW_CIN * g + c;
  float4 nx[8];
  long long t = blockIdx.x;
  auto load = [&](long long tile) {
    const float* p = dyg + min(tile * 32 + c, rows - 1) * Cout;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) { nx[2 * kt] = ld4(p + 16 * kt); nx[2 * kt + 1] = ld4(p + 16 * kt + 4); }
  };
  if (t < ntiles) load(t);
  for (; t < ntiles; t += gridDim.x) {
    // the next tile's K block kt is requested as soon as this tile's MFMAs of that block have read their registers: one tile of dy in
    // flight per wave without a second set of 32 registers (a full double buffer does not fit 4 waves per SIMD)
    const long long tn = t + gridDim.x;
    const bool more = tn < ntiles;
    const float* pn = dyg + min(tn * 32 + c, rows - 1) * Cout;
    floatx16 acc = {0};
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      const float4 u = nx[2 * kt], v = nx[2 * kt + 1];
      const float af[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
#pragma unroll
      for (int st = 0; st < 8; ++st) acc = mfma32(af[st], bf[kt][st], acc);
      if (more) { nx[2 * kt] = ld4(pn + 16 * kt); nx[2 * kt + 1] = ld4(pn + 16 * kt + 4); }
    }
    if (c < GPW_CIN) {
      const long long mb = t * 32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long m = mb + acc_row(r, hf);
        if (m < rows) dxg[m * Cin] = acc[r];
      }
    }
  }
}

// part[blockIdx.x][g][o][i] = sum over the workgroup's rows m of dy[m, 64 g + o] x[m, 16 g + i].  The k slot of the instruction is the row:
// step s of a 16-row block multiplies rows 2 s + hf.  Sixteen waves: waves 0-7 take the first half of the workgroup's rows, waves 8-15 the
// second, one group each; the two halves meet in LDS, so a workgroup of twice the rows leaves ONE partial.  Every address of the row loop is
// a wave-uniform base that advances by 16 rows plus one of 16 fixed per-lane offsets: one vector add per load, no clamps or selects (the
// fp32 MFMA shares its ALUs with them); only the last rows of the launch take the predicated tail.  Columns 16-31 of the instruction repeat columns 0-15 and are dropped.
__global__ __launch_bounds__(1024, 4) void grouped_pointwise_dw_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                      float* __restrict__ part, long long rows, int G, long long rows_per_wg) {
  __shared__ float comb[GPW_WAVES][GPW_COUT * GPW_CIN];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, c = lane & 31, hf = lane >> 5;
  const int gl = wave & (GPW_WAVES - 1), half = wave / GPW_WAVES;
  const int g = blockIdx.y * GPW_WAVES + gl;
  const bool active = g < G;
  const long long Cin = (long long)GPW_CIN * G, Cout = (long long)GPW_COUT * G;
  const long long w0 = blockIdx.x * rows_per_wg, w1 = min(rows, w0 + rows_per_wg), hr = rows_per_wg / 2;   // hr: a multiple of 16
  const long long r0 = min(w1, w0 + half * hr), r1 = min(w1, r0 + hr);
  floatx16 acc0 = {0}, acc1 = {0};
  if (active && r0 < r1) {
    const float* pa = dy + GPW_COUT * g + r0 * Cout;         // wave-uniform
    const float* pb = x + GPW_CIN * g + r0 * Cin;
    unsigned oa[8], ob[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) { oa[s] = (unsigned)((2 * s + hf) * Cout + c); ob[s] = (unsigned)((2 * s + hf) * Cin + (c & 15)); }
    float a0[8], a1[8], b[8];
    const long long nfull = (r1 - r0) / GPW_DW_STEP;
    const int rem = (int)(r1 - r0 - nfull * GPW_DW_STEP);
    auto load = [&]() {
#pragma unroll
      for (int s = 0; s < 8; ++s) { a0[s] = pa[oa[s]]; a1[s] = pa[oa[s] + 32]; b[s] = pb[ob[s]]; }
    };
    if (nfull > 0) load();
    for (long long i = 0; i < nfull; ++i) {
      float ca0[8], ca1[8], cb[8];
#pragma unroll
      for (int s = 0; s < 8; ++s) { ca0[s] = a0[s]; ca1[s] = a1[s]; cb[s] = b[s]; }
      pa += GPW_DW_STEP * Cout; pb += GPW_DW_STEP * Cin;
      if (i + 1 < nfull) load();                             // in flight during the MFMAs
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        acc0 = mfma32(ca0[s], cb[s], acc0);
        acc1 = mfma32(ca1[s], cb[s], acc1);
      }
    }
    if (rem) {                                               // the last rows of the launch: rows past the end contribute zeros
#pragma nounroll
      for (int s = 0; s < (rem + 1) / 2; ++s) {              // (once per launch: kept rolled, it holds no registers of the loop above)
        const bool in = 2 * s + hf < rem;
        const long long row = in ? 2 * s + hf : 0;
        const float u = pa[row * Cout + c], v = pa[row * Cout + c + 32], z = pb[row * Cin + (c & 15)];
        acc0 = mfma32(in ? u : 0.f, in ? z : 0.f, acc0);
        acc1 = mfma32(in ? v : 0.f, in ? z : 0.f, acc1);
      }
    }
  }
  const bool live = active && c < GPW_CIN;
  if (half == 1 && live) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      comb[gl][acc_row(r, hf) * GPW_CIN + c] = acc0[r];
      comb[gl][(32 + acc_row(r, hf)) * GPW_CIN + c] = acc1[r];
    }
  }
  __syncthreads();
  if (half == 0 && live) {
    float* p = part + ((long long)blockIdx.x * G + g) * (GPW_COUT * GPW_CIN) + c;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      p[acc_row(r, hf) * GPW_CIN] = acc0[r] + comb[gl][acc_row(r, hf) * GPW_CIN + c];
      p[(32 + acc_row(r, hf)) * GPW_CIN] = acc1[r] + comb[gl][(32 + acc_row(r, hf)) * GPW_CIN + c];
    }
  }
}

// dw[e] = sum over the np partials of part[p][e], in a fixed order: segment s of GPW_SEG adds its partials p in [s L, (s + 1) L) ascending,
// then one thread adds the segment sums ascending.  32 elements x 32 segments per workgroup; a segment's loads are issued eight at a time
// before they are added (one thread per element walking all partials is np dependent round trips to L2: 14 us for 250 partials).
__global__ __launch_bounds__(32 * GPW_SEG) void grouped_pointwise_dw_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                                                   long long E, int np) {
  __shared__ float seg[GPW_SEG][32];
  const int e = threadIdx.x & 31, s = threadIdx.x >> 5;
  const long long idx = (long long)blockIdx.x * 32 + e;      // E is a multiple of 1024: always in range
  const int L = (np + GPW_SEG - 1) / GPW_SEG, p0 = s * L, p1 = min(np, p0 + L);
  float sum = 0.f;
  for (int p = p0; p < p1; p += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = p + j < p1 ? part[(long long)(p + j) * E + idx] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) sum += v[j];
  }
  seg[s][e] = sum;
  __syncthreads();
  if (s == 0) {
    float v = seg[0][e];
#pragma unroll
    for (int k = 1; k < GPW_SEG; ++k) v += seg[k][e];
    dw[idx] = v;
  }
}

// rows of x / dy per dW workgroup (two halves of whole 16-row steps, at least 32 rows each: a shorter launch is better served by fewer
// workgroups than by more partials) and the number of workgroups, one per CU at most: functions of `rows` alone
long long gpw_dw_rows_per_wg(long long rows) {
  const long long per = (rows + GPW_DW_GRID - 1) / GPW_DW_GRID, rpw = (per + 2 * GPW_DW_STEP - 1) / (2 * GPW_DW_STEP) * (2 * GPW_DW_STEP);
  return rpw < 64 ? 64 : rpw;
}
long long gpw_dw_workgroups(long long rows) { const long long rpw = gpw_dw_rows_per_wg(rows); return (rows + rpw - 1) / rpw; }

bool gpw_al16(const void* p) { return ((size_t)p & 15) == 0; }

}  // namespace

extern "C" {

int smml_grouped_pointwise_applies(int groups, int cin_g, int cout_g) {
  return groups > 0 && cin_g == GPW_CIN && cout_g == GPW_COUT;
}

#define GPW_CHECK_SHAPE(fn)                                                                                                          \
  SMML_REQUIRE(rows > 0 && groups > 0, fn ": non-positive size (rows=%lld groups=%d)", rows, groups);                                 \
  SMML_REQUIRE(smml_grouped_pointwise_applies(groups, cin_g, cout_g), fn ": built for 16 input and 64 output channels per group, got %d and %d", cin_g, cout_g); \
  SMML_REQUIRE(rows <= (1LL << 40) && groups <= 8 * 65535, fn ": problem too large (rows=%lld groups=%d)", rows, groups)

int smml_grouped_pointwise_fwd_f32(const float* x, const float* w, float* y, long long rows, int groups, int cin_g, int cout_g, void* stream) {
  SMML_REQUIRE(x && w && y, "smml_grouped_pointwise_fwd_f32: null operand");
  GPW_CHECK_SHAPE("smml_grouped_pointwise_fwd_f32");
  SMML_REQUIRE(gpw_al16(x) && gpw_al16(w), "smml_grouped_pointwise_fwd_f32: x and w must be 16-byte aligned");
  const long long ntiles = (rows + 31) / 32;
  dim3 grid((unsigned)(ntiles < GPW_GRID ? ntiles : GPW_GRID), (unsigned)((groups + GPW_WAVES - 1) / GPW_WAVES));
  hipLaunchKernelGGL(grouped_pointwise_fwd_kernel, grid, dim3(64 * GPW_WAVES), 0, (hipStream_t)stream, x, w, y, rows, groups);
  SMML_LAUNCH_CHECK("smml_grouped_pointwise_fwd_f32");
  return SMML_OK;
}

int smml_grouped_pointwise_dx_f32(const float* dy, const float* w, float* dx, long long rows, int groups, int cin_g, int cout_g, void* stream) {
  SMML_REQUIRE(dy && w && dx, "smml_grouped_pointwise_dx_f32: null operand");
  GPW_CHECK_SHAPE("smml_grouped_pointwise_dx_f32");
  SMML_REQUIRE(gpw_al16(dy), "smml_grouped_pointwise_dx_f32: dy must be 16-byte aligned");
  const long long ntiles = (rows + 31) / 32;
  dim3 grid((unsigned)(ntiles < GPW_GRID ? ntiles : GPW_GRID), (unsigned)((groups + GPW_WAVES - 1) / GPW_WAVES));
  hipLaunchKernelGGL(grouped_pointwise_dx_kernel, grid, dim3(64 * GPW_WAVES), 0, (hipStream_t)stream, dy, w, dx, rows, groups);
  SMML_LAUNCH_CHECK("smml_grouped_pointwise_dx_f32");
  return SMML_OK;
}

size_t smml_grouped_pointwise_dw_workspace_bytes(long long rows, int groups, int cin_g, int cout_g) {
  if (rows <= 0 || rows > (1LL << 40) || !smml_grouped_pointwise_applies(groups, cin_g, cout_g)) return 0;
  return (size_t)gpw_dw_workgroups(rows) * (size_t)groups * (size_t)(GPW_COUT * GPW_CIN) * sizeof(float);
}

int smml_grouped_pointwise_dw_f32(const float* dy, const float* x, float* dw, long long rows, int groups, int cin_g, int cout_g,
                                  void* workspace, size_t workspace_bytes, void* stream) {
  SMML_REQUIRE(dy && x && dw && workspace, "smml_grouped_pointwise_dw_f32: null operand or workspace");
  GPW_CHECK_SHAPE("smml_grouped_pointwise_dw_f32");
  SMML_REQUIRE(workspace_bytes >= smml_grouped_pointwise_dw_workspace_bytes(rows, groups, cin_g, cout_g),
               "smml_grouped_pointwise_dw_f32: workspace too small");
  const long long rpw = gpw_dw_rows_per_wg(rows), nwg = gpw_dw_workgroups(rows);
  float* part = nwg == 1 ? dw : (float*)workspace;           // a single partial is the result itself: no second pass
  dim3 grid((unsigned)nwg, (unsigned)((groups + GPW_WAVES - 1) / GPW_WAVES));
  hipLaunchKernelGGL(grouped_pointwise_dw_kernel, grid, dim3(128 * GPW_WAVES), 0, (hipStream_t)stream, dy, x, part, rows, groups, rpw);
  SMML_LAUNCH_CHECK("smml_grouped_pointwise_dw_f32");
  if (nwg == 1) return SMML_OK;
  const long long E = (long long)groups * (GPW_COUT * GPW_CIN);
  hipLaunchKernelGGL(grouped_pointwise_dw_reduce_kernel, dim3((unsigned)(E / 32)), dim3(32 * GPW_SEG), 0, (hipStream_t)stream, part, dw, E, (int)nwg);
  SMML_LAUNCH_CHECK("smml_grouped_pointwise_dw_f32/reduce");
  return SMML_OK;
}

#undef GPW_CHECK_SHAPE

}  // extern "C"
