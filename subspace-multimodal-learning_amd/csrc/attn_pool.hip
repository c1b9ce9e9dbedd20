// Attention pooling of ABMIL (models/mil.py:66-75): M_b = sum_n softmax_n(H_bn . w2 + b2) x_bn over one bag of N instances, and its backward.
// A 1-query attention over N keys of width L: through the tiled GEMM it is an M = 1 product, a softmax and another M = 1 product per bag;
// here the bag's rows stream once through registers with an online softmax (running max m, running sum l, L-wide accumulator).
//
//   forward   grid (splits, B), 256 threads.  A workgroup walks its rows in tiles of 16: every wave forms the scores of 4 rows (one wave per
//             row dot, DPP sum), the 16 scores meet in LDS, every wave then forms the tile's max and the 16 weights exp(s - m) in its lanes
//             and hands them out with readlane; thread t owns columns 4 t .. 4 t + 3 of the accumulator, so a row of x is read as one
//             coalesced 4 KB sweep and the tile's 16 row loads are issued before the first is used.  One partial (m, l, acc[L]) per split;
//             a second kernel merges a bag's partials in ascending split order.
//   backward  two streaming kernels on the same grid, one wave per row: the row dots t_n = dM . x_n (x, four rows in flight per wave), then
//             ds_n = softmax_n (t_n - c) with c = sum_n softmax_n t_n, dH_n = ds_n w2 (.) (1 - H_n^2) (H, eight rows in flight) and the
//             per-workgroup partials of dw2 / db2, which a third kernel sums in a fixed order.
//   gated     GatedABMIL (models/mil.py:134-140): the score is sum_d w_d tanh(.)_d sigmoid(.)_d + b, the two hidden tensors are the halves of
//             one buffer h2 [B, N, 2 D].  The forward and the second backward kernel are templated on GATED; merge, row dots and the final
//             reduction are shared.
// Every sum has one owner and a fixed order: no float atomics, the results are a function of the inputs and the split count alone.
#include "smml_common.h"

#include <algorithm>
#include <math.h>

namespace {

constexpr int AP_THREADS = 256;
constexpr int AP_TILE = 16;          // rows per forward tile = x rows in flight per thread (16 float4 registers)
constexpr int AP_MAXL = 1024;        // L <= 4 * AP_THREADS: one float4 of the accumulator per thread
constexpr int AP_MAXD = 256;         // D <= 4 * 64: at most four hidden values per lane
constexpr int AP_MIN_ROWS = 48;      // rows per split the heuristic does not go below (three tiles: the 4 L-byte partial stays under 3 % of the reads)
constexpr int AP_TARGET_WG = 1024;   // workgroups the heuristic aims at: 256 CUs x 4 resident (<= 128 VGPRs, 128 B of LDS)

// max / sum over each aligned group of 16 lanes, valid in every lane of the group (butterfly: both partners add the same two numbers, so the lanes
// agree bit for bit)
__device__ __forceinline__ float group16_max(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
// sum over the 64 lanes in fp64, valid in every lane (butterfly; the lanes agree bit for bit)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float lane_value(float v, int lane) {
  return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), lane));
}
__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); }

// x [B, N, L], h [B, N, D], w2 [D], b2 [1] -> s [B, N], pacc [B, S, L], pml [B, S, 2]; split sp of bag b owns rows [sp rps, min(N, (sp + 1) rps))
// GATED: h is h2 [B, N, 2 D], tanh units in columns [0, D) and sigmoid units in [D, 2 D) of one contiguous row; s_n = sum_d w_d hv_nd hu_nd + b
template <bool GATED>
__global__ __launch_bounds__(AP_THREADS) void attn_pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ h,
                                                                   const float* __restrict__ w2, const float* __restrict__ b2p, float* __restrict__ s,
                                                                   float* __restrict__ pacc, float* __restrict__ pml, const int N, const int L,
                                                                   const int D, const int rps) {
  const int b = blockIdx.y, sp = blockIdx.x, S = gridDim.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = sp * rps, r1 = r0 + min(rps, N - r0);
  const int dj = D >> 6;
  const bool col = 4 * tid < L;
  // every load is unconditional (straight-line code: the loads of a tile are issued back to back): a row past the split's end, a column past
  // L and a hidden panel past D re-read an address that is in range, and meet a weight of zero or are never stored
  const float* xb = x + (size_t)b * N * L + (col ? 4 * tid : 0);
  const int HS = GATED ? 2 * D : D;        // row stride of h
  const float* hb = h + (size_t)b * N * HS + lane;
  __shared__ float sS[2][AP_TILE];       // the tile's scores; two buffers: a wave may fill the next tile's while another still reads this one's

  float w2r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) w2r[j] = j < dj ? w2[j * 64 + lane] : 0.f;
  const float b2 = b2p[0];

  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float m = -INFINITY, l = 0.f;
  int buf = 0;
  for (int t0 = r0; t0 < r1; t0 += AP_TILE, buf ^= 1) {
    // the hidden rows first (the scores wait for them alone), then the tile's 16 rows of x: those stay in flight under the score phase
    float hv[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = min(t0 + wave + 4 * i, r1 - 1);
#pragma unroll
      for (int j = 0; j < 4; ++j) hv[i][j] = hb[(size_t)row * HS + (j < dj ? j * 64 : 0)];      // w2r[j] = 0 for j >= dj
    }
    float hu[GATED ? 4 : 1][4];              // the sigmoid half of the same rows: same clamps, D columns further (D + j 64 + lane < 2 D)
    if constexpr (GATED) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = min(t0 + wave + 4 * i, r1 - 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) hu[i][j] = hb[(size_t)row * HS + D + (j < dj ? j * 64 : 0)];
      }
    }
    float4 xr[AP_TILE];
#pragma unroll
    for (int r = 0; r < AP_TILE; ++r) xr[r] = *reinterpret_cast<const float4*>(xb + (size_t)min(t0 + r, r1 - 1) * L);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) d = fmaf(GATED ? hv[i][j] * hu[i][j] : hv[i][j], w2r[j], d);
      d = wave_sum(d) + b2;
      if (lane == 0) sS[buf][wave + 4 * i] = (t0 + wave + 4 * i < r1) ? d : -INFINITY;     // a row past the end weighs exp(-inf) = 0
    }
    __syncthreads();
    const float sv = sS[buf][lane & 15];
    if (tid < AP_TILE && t0 + tid < r1) s[(size_t)b * N + t0 + tid] = sv;
    // online softmax: every wave forms the same m, l and weights (same inputs, same order)
    const float mn = fmaxf(m, group16_max(sv));          // finite: a tile holds at least one row
    const float scale = expf(m - mn);                    // first tile: exp(-inf) = 0 on a zero accumulator
    const float p = expf(sv - mn);
    l = fmaf(l, scale, group16_sum(p));
    m = mn;
    acc.x *= scale; acc.y *= scale; acc.z *= scale; acc.w *= scale;
#pragma unroll
    for (int r = 0; r < AP_TILE; ++r) {
      const float pr = lane_value(p, r);
      acc.x = fmaf(pr, xr[r].x, acc.x); acc.y = fmaf(pr, xr[r].y, acc.y);
      acc.z = fmaf(pr, xr[r].z, acc.z); acc.w = fmaf(pr, xr[r].w, acc.w);
    }
  }
  const size_t part = (size_t)b * S + sp;
  if (col) *reinterpret_cast<float4*>(pacc + part * L + 4 * tid) = acc;
  if (tid == 0) { pml[part * 2] = m; pml[part * 2 + 1] = l; }
}

// partials of bag b, in ascending split order -> M [B, L], lse [B].  One workgroup per bag walks S partial rows: the rescale weights
// exp(m_i - m) of 256 splits at a time are formed by 256 threads and parked in LDS, and the rows are read 16 at a time (a dependent load per
// split would cost one memory latency each; at 8 x 10 000 that was most of the forward's time)
__global__ __launch_bounds__(AP_THREADS) void attn_pool_merge_kernel(const float* __restrict__ pacc, const float* __restrict__ pml,
                                                                     float* __restrict__ out, float* __restrict__ lse, const int S, const int L) {
  const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool col = 4 * tid < L;
  const float* ml = pml + (size_t)b * S * 2;
  const float* pa = pacc + (size_t)b * S * L + (col ? 4 * tid : 0);
  __shared__ float mred[4], wS[AP_THREADS], lwS[AP_THREADS];
  float m = -INFINITY;
  for (int i = tid; i < S; i += AP_THREADS) m = fmaxf(m, ml[2 * i]);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
  if (lane == 0) mred[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(mred[0], mred[1]), fmaxf(mred[2], mred[3]));
  float l = 0.f;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int c0 = 0; c0 < S; c0 += AP_THREADS) {
    const int cn = min(AP_THREADS, S - c0);
    __syncthreads();                                   // the previous chunk's weights have been read
    if (tid < cn) {
      const float w = expf(ml[2 * (c0 + tid)] - m);
      wS[tid] = w;
      lwS[tid] = ml[2 * (c0 + tid) + 1] * w;
    }
    __syncthreads();
    for (int i0 = 0; i0 < cn; i0 += 16) {
      float4 a[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) a[k] = *reinterpret_cast<const float4*>(pa + (size_t)(c0 + min(i0 + k, cn - 1)) * L);
#pragma unroll
      for (int k = 0; k < 16; ++k) {
        const bool ok = i0 + k < cn;
        const float w = ok ? wS[min(i0 + k, cn - 1)] : 0.f;
        l += ok ? lwS[min(i0 + k, cn - 1)] : 0.f;
        acc.x = fmaf(w, a[k].x, acc.x); acc.y = fmaf(w, a[k].y, acc.y); acc.z = fmaf(w, a[k].z, acc.z); acc.w = fmaf(w, a[k].w, acc.w);
      }
    }
  }
  const float inv = 1.f / l;
  if (col) *reinterpret_cast<float4*>(out + (size_t)b * L + 4 * tid) = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
  if (tid == 0) lse[b] = m + logf(l);
}

// row stride of the backward partials: dw2 in columns [0, D), db2 in column D
__host__ __device__ constexpr int bwd_part_ld(int D) { return D + 64; }

// t[b, n] = dM[b, :] . x[b, n, :]: one wave per row, four rows (16 KB) in flight per wave; and per split zc = (sum e_n, sum e_n t_n) with
// e_n = exp(s_n - lse) over the split's rows (wave order, then the four waves in order), in fp64: see attn_pool_bwd_kernel
__global__ __launch_bounds__(AP_THREADS) void attn_pool_bwd_rowdot_kernel(const float* __restrict__ x, const float* __restrict__ dM,
                                                                          const float* __restrict__ s, const float* __restrict__ lse,
                                                                          float* __restrict__ t, double* __restrict__ zc, const int N, const int L,
                                                                          const int rps) {
  const int b = blockIdx.y, sp = blockIdx.x, S = gridDim.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r0 = sp * rps, r1 = r0 + min(rps, N - r0);
  const int lj = L >> 8;
  const float* xb = x + (size_t)b * N * L + 4 * lane;       // loads are unconditional, as in the forward kernel
  // this lane's columns of dM: 4 lane .. 4 lane + 3 of every 256-column panel
  float4 g[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    g[j] = j < lj ? *reinterpret_cast<const float4*>(dM + (size_t)b * L + j * 256 + 4 * lane) : make_float4(0.f, 0.f, 0.f, 0.f);
  const float lseb = lse[b];
  double ez = 0., ec = 0.;
  for (int row = r0 + 4 * wave; row < r1; row += 16) {
    float4 xv[4][4];
    float sv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const size_t ri = (size_t)min(row + i, r1 - 1);
#pragma unroll
      for (int j = 0; j < 4; ++j) xv[i][j] = *reinterpret_cast<const float4*>(xb + ri * L + (j < lj ? j * 256 : 0));   // g[j] = 0 for j >= lj
      sv[i] = s[(size_t)b * N + ri];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) d += dot4(g[j], xv[i][j]);
      d = wave_sum(d);
      const bool ok = row + i < r1;
      if (lane == 0 && ok) t[(size_t)b * N + row + i] = d;
      const float e = ok ? expf(sv[i] - lseb) : 0.f;
      ez += (double)e;
      ec = fma((double)e, (double)d, ec);
    }
  }
  __shared__ double red[2][4];
  if (lane == 0) { red[0][wave] = ez; red[1][wave] = ec; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = zc + ((size_t)b * S + sp) * 2;
    o[0] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    o[1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  }
}

// saved h, s, lse and the row dots t -> dh [B, N, D] (times 1 - h^2 if tanh_grad) and part [B S, D + 64]
// GATED: h is h2 [B, N, 2 D] = (hv | hu) and dh has its shape.  With g = ds w_d: tanh_grad writes the pre-activation gradients
// g hu (1 - hv^2) | g hv hu (1 - hu), otherwise the gradients of h2 itself, g hu | g hv; dw_d = sum_n ds hv hu
template <bool GATED>
__global__ __launch_bounds__(AP_THREADS) void attn_pool_bwd_kernel(const float* __restrict__ h, const float* __restrict__ w2,
                                                                   const float* __restrict__ s, const float* __restrict__ lse,
                                                                   const float* __restrict__ t, const double* __restrict__ zc,
                                                                   float* __restrict__ dh, float* __restrict__ part, const int N, const int D,
                                                                   const int rps, const int tanh_grad) {
  const int b = blockIdx.y, sp = blockIdx.x, S = gridDim.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = sp * rps, r1 = r0 + min(rps, N - r0);
  const int dj = D >> 6;
  const int HS = GATED ? 2 * D : D;                          // row stride of h and dh
  const float* hb = h + (size_t)b * N * HS + lane;          // loads are unconditional, as in the forward kernel
  float* dhb = dh + (size_t)b * N * HS + lane;
  const float* sb = s + (size_t)b * N;
  const float* tb = t + (size_t)b * N;

  // ds_n = p_n (t_n - c) with p_n = e_n / z, e_n = exp(s_n - lse), z = sum_n e_n (1 only to the rounding of lse, |lse| 2^-24 absolute) and
  // c = sum_n e_n t_n / z: every workgroup adds the S per-split sums of the row-dot kernel in a fixed order.  c is formed from the SAME e_n
  // and t_n that ds uses, and it is kept in fp64 up to the difference t_n - c: sum_n ds_n, zero in exact arithmetic, then cancels to the
  // rounding of its terms.  db1 = w2 (.) sum_n ds_n (1 - h_n^2) needs that: with a peaked softmax half an fp32 ulp of c (5e-8 of it) moves db1
  // by 1e-4 of its scale - an fp32 c, from dM . M or from the row dots, left db1 5 x further from fp64 than an fp32 evaluation by torch.
  const float lseb = lse[b];
  __shared__ double zred[2][4];
  double z = 0., cz = 0.;
  for (int i = tid; i < S; i += AP_THREADS) {
    z += zc[((size_t)b * S + i) * 2];
    cz += zc[((size_t)b * S + i) * 2 + 1];
  }
  z = wave_sum_f64(z);
  cz = wave_sum_f64(cz);
  if (lane == 0) { zred[0][wave] = z; zred[1][wave] = cz; }
  __syncthreads();
  z = ((zred[0][0] + zred[0][1]) + zred[0][2]) + zred[0][3];
  const double c = (((zred[1][0] + zred[1][1]) + zred[1][2]) + zred[1][3]) / z;
  const float rz = (float)(1. / z);
  float w2r[4], dw[4] = {0.f, 0.f, 0.f, 0.f}, db = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) w2r[j] = j < dj ? w2[j * 64 + lane] : 0.f;

  // one wave per row, eight rows in flight per wave
  for (int row = r0 + 8 * wave; row < r1; row += 32) {
    float hv[8][4], sv[8], tv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const size_t ri = (size_t)min(row + i, r1 - 1);
#pragma unroll
      for (int j = 0; j < 4; ++j) hv[i][j] = hb[ri * HS + (j < dj ? j * 64 : 0)];
      sv[i] = sb[ri];
      tv[i] = tb[ri];
    }
    float hu[GATED ? 8 : 1][4];              // the sigmoid half: same clamps, D columns further
    if constexpr (GATED) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const size_t ri = (size_t)min(row + i, r1 - 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) hu[i][j] = hb[ri * HS + D + (j < dj ? j * 64 : 0)];
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const bool ok = row + i < r1;
      const float ds = ok ? expf(sv[i] - lseb) * rz * (float)((double)tv[i] - c) : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < dj) {
          const float hh = hv[i][j];
          if constexpr (GATED) {
            const float uu = hu[i][j], g = ds * w2r[j];
            float ov = g * uu, ou = g * hh;
            if (tanh_grad) { ov *= fmaf(-hh, hh, 1.f); ou *= uu * (1.f - uu); }
            if (ok) {
              dhb[(size_t)(row + i) * HS + j * 64] = ov;
              dhb[(size_t)(row + i) * HS + D + j * 64] = ou;
            }
            dw[j] = fmaf(ds, hh * uu, dw[j]);
          } else {
            float o = ds * w2r[j];
            if (tanh_grad) o *= fmaf(-hh, hh, 1.f);
            if (ok) dhb[(size_t)(row + i) * D + j * 64] = o;
            dw[j] = fmaf(ds, hh, dw[j]);
          }
        }
      }
      db += ds;
    }
  }
  // the four waves' sums, added in wave order
  __shared__ float red[4][AP_MAXD + 1];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < dj) red[wave][j * 64 + lane] = dw[j];
  if (lane == 0) red[wave][D] = db;
  __syncthreads();
  float* pr = part + ((size_t)b * S + sp) * bwd_part_ld(D);
  for (int k = tid; k <= D; k += AP_THREADS) pr[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// part [P, D + 64] -> dw2 [D], db2 [1]: wave w of 16 adds rows w, w + 16, ... in ascending order (eight loads in flight), the waves' sums are
// added in wave order
constexpr int AP_REDUCE_WAVES = 16;
__global__ __launch_bounds__(64 * AP_REDUCE_WAVES) void attn_pool_bwd_reduce_kernel(const float* __restrict__ part, const long long P, const int D,
                                                                                   float* __restrict__ dw2, float* __restrict__ db2) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int k = blockIdx.x * 64 + lane;
  const int ld = bwd_part_ld(D);
  __shared__ float red[AP_REDUCE_WAVES][64];
  float a = 0.f;
  if (k <= D)
    for (long long p = wave; p < P; p += 8 * AP_REDUCE_WAVES) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p + u * AP_REDUCE_WAVES < P ? part[(p + u * AP_REDUCE_WAVES) * ld + k] : 0.f;
#pragma unroll
      for (int u = 0; u < 8; ++u) a += v[u];
    }
  red[wave][lane] = a;
  __syncthreads();
  if (wave == 0 && k <= D) {
    float v = red[0][lane];
#pragma unroll
    for (int w = 1; w < AP_REDUCE_WAVES; ++w) v += red[w][lane];
    if (k < D) dw2[k] = v; else db2[0] = v;
  }
}

bool pool_shape_ok(int B, int N, int L, int D) {
  return B > 0 && B <= 65535 && N > 0 && N <= (1 << 30) && L > 0 && L <= AP_MAXL && L % 256 == 0 && D > 0 && D <= AP_MAXD && D % 64 == 0;
}

// rows per split: `splits` as asked for (tests), or - splits <= 0 - enough splits for AP_TARGET_WG workgroups, none under AP_MIN_ROWS rows
int pool_rows_per_split(int B, int N, int splits) {
  if (splits > 0) return (int)(((long long)N + splits - 1) / splits);
  const int want = std::max(1, (AP_TARGET_WG + B - 1) / B);
  return std::max((N + want - 1) / want, std::min(N, AP_MIN_ROWS));
}
// the splits that hold a row
int pool_splits(int N, int rps) { return (int)(((long long)N + rps - 1) / rps); }

bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// floats of the backward's row dots t [B, N], padded so that what follows them in the workspace stays 16-byte aligned
size_t bwd_rowdot_floats(int B, int N) { return ((size_t)B * (size_t)N + 3) / 4 * 4; }

// the plain and the gated entry points differ in the hidden tensor's row (D or 2 D floats) and in the kernel instantiation alone
template <bool GATED>
int pool_fwd(const char* fn, const float* x, const float* h, const float* w2, const float* b2, float* s, float* out, float* lse,
             void* workspace, size_t workspace_bytes, int B, int N, int L, int D, int splits, void* stream) {
  SMML_REQUIRE(x && h && w2 && b2 && s && out && lse && workspace, "%s: null pointer", fn);
  SMML_REQUIRE(pool_shape_ok(B, N, L, D), "%s: need L a multiple of 256 up to %d and D a multiple of 64 up to %d, N >= 1, "
               "B <= 65535 (got B %d, N %d, L %d, D %d)", fn, AP_MAXL, AP_MAXD, B, N, L, D);
  SMML_REQUIRE(aligned16(x) && aligned16(out) && aligned16(workspace), "%s: x, out and workspace must be 16-byte aligned", fn);
  SMML_REQUIRE(workspace_bytes >= smml_attn_pool_fwd_workspace_bytes(B, N, L, splits), "%s: workspace too small", fn);
  const int rps = pool_rows_per_split(B, N, splits), S = pool_splits(N, rps);
  float* pacc = (float*)workspace;
  float* pml = pacc + (size_t)B * S * L;
  hipLaunchKernelGGL(attn_pool_fwd_kernel<GATED>, dim3((unsigned)S, (unsigned)B), dim3(AP_THREADS), 0, (hipStream_t)stream, x, h, w2, b2, s, pacc,
                     pml, N, L, D, rps);
  SMML_LAUNCH_CHECK(fn);
  hipLaunchKernelGGL(attn_pool_merge_kernel, dim3((unsigned)B), dim3(AP_THREADS), 0, (hipStream_t)stream, pacc, pml, out, lse, S, L);
  SMML_LAUNCH_CHECK(fn);
  return SMML_OK;
}

template <bool GATED>
int pool_bwd(const char* fn, const float* x, const float* h, const float* w2, const float* s, const float* lse, const float* dout,
             float* dh, float* dw2, float* db2, void* workspace, size_t workspace_bytes, int B, int N, int L, int D, int splits,
             int tanh_grad, void* stream) {
  SMML_REQUIRE(x && h && w2 && s && lse && dout && dh && dw2 && db2 && workspace, "%s: null pointer", fn);
  SMML_REQUIRE(pool_shape_ok(B, N, L, D), "%s: need L a multiple of 256 up to %d and D a multiple of 64 up to %d, N >= 1, "
               "B <= 65535 (got B %d, N %d, L %d, D %d)", fn, AP_MAXL, AP_MAXD, B, N, L, D);
  SMML_REQUIRE(aligned16(x) && aligned16(dout) && aligned16(workspace), "%s: x, dout and workspace must be 16-byte aligned", fn);
  SMML_REQUIRE(workspace_bytes >= smml_attn_pool_bwd_workspace_bytes(B, N, D, splits), "%s: workspace too small", fn);
  const int rps = pool_rows_per_split(B, N, splits), S = pool_splits(N, rps);
  float* t = (float*)workspace;
  double* zc = (double*)(t + bwd_rowdot_floats(B, N));
  float* part = (float*)(zc + (size_t)B * S * 2);
  hipLaunchKernelGGL(attn_pool_bwd_rowdot_kernel, dim3((unsigned)S, (unsigned)B), dim3(AP_THREADS), 0, (hipStream_t)stream, x, dout, s, lse, t, zc,
                     N, L, rps);
  SMML_LAUNCH_CHECK(fn);
  hipLaunchKernelGGL(attn_pool_bwd_kernel<GATED>, dim3((unsigned)S, (unsigned)B), dim3(AP_THREADS), 0, (hipStream_t)stream, h, w2, s, lse, t, zc,
                     dh, part, N, D, rps, tanh_grad);
  SMML_LAUNCH_CHECK(fn);
  hipLaunchKernelGGL(attn_pool_bwd_reduce_kernel, dim3((unsigned)(bwd_part_ld(D) / 64)), dim3(64 * AP_REDUCE_WAVES), 0, (hipStream_t)stream, part,
                     (long long)B * S, D, dw2, db2);
  SMML_LAUNCH_CHECK(fn);
  return SMML_OK;
}

}  // namespace

extern "C" {

size_t smml_attn_pool_fwd_workspace_bytes(int B, int N, int L, int splits) {
  if (B <= 0 || N <= 0 || L <= 0) return 0;
  const size_t S = (size_t)pool_splits(N, pool_rows_per_split(B, N, splits));
  return (size_t)B * S * ((size_t)L + 4) * sizeof(float);       // acc [B, S, L], then (m, l) [B, S, 2] (padded to 4: the next user stays aligned)
}

int smml_attn_pool_fwd_f32(const float* x, const float* h, const float* w2, const float* b2, float* s, float* out, float* lse, void* workspace,
                           size_t workspace_bytes, int B, int N, int L, int D, int splits, void* stream) {
  return pool_fwd<false>("smml_attn_pool_fwd_f32", x, h, w2, b2, s, out, lse, workspace, workspace_bytes, B, N, L, D, splits, stream);
}

int smml_attn_pool_gated_fwd_f32(const float* x, const float* h2, const float* w, const float* b, float* s, float* out, float* lse,
                                 void* workspace, size_t workspace_bytes, int B, int N, int L, int D, int splits, void* stream) {
  return pool_fwd<true>("smml_attn_pool_gated_fwd_f32", x, h2, w, b, s, out, lse, workspace, workspace_bytes, B, N, L, D, splits, stream);
}

size_t smml_attn_pool_bwd_workspace_bytes(int B, int N, int D, int splits) {
  if (B <= 0 || N <= 0 || D <= 0) return 0;
  const size_t S = (size_t)pool_splits(N, pool_rows_per_split(B, N, splits));
  return (bwd_rowdot_floats(B, N) + (size_t)B * S * (size_t)(bwd_part_ld(D) + 4)) * sizeof(float);     // t [B, N], zc [B S, 2] fp64, part [B S, D + 64]
}

int smml_attn_pool_bwd_f32(const float* x, const float* h, const float* w2, const float* s, const float* lse, const float* dout, float* dh,
                           float* dw2, float* db2, void* workspace, size_t workspace_bytes, int B, int N, int L, int D, int splits,
                           int tanh_grad, void* stream) {
  return pool_bwd<false>("smml_attn_pool_bwd_f32", x, h, w2, s, lse, dout, dh, dw2, db2, workspace, workspace_bytes, B, N, L, D, splits,
                         tanh_grad, stream);
}

int smml_attn_pool_gated_bwd_f32(const float* x, const float* h2, const float* w, const float* s, const float* lse, const float* dout,
                                 float* dh2, float* dw, float* db, void* workspace, size_t workspace_bytes, int B, int N, int L, int D,
                                 int splits, int act_grad, void* stream) {
  return pool_bwd<true>("smml_attn_pool_gated_bwd_f32", x, h2, w, s, lse, dout, dh2, dw, db, workspace, workspace_bytes, B, N, L, D, splits,
                        act_grad, stream);
}

}  // extern "C"
