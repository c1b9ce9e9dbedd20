// Row-wise / column-wise HBM-bound pieces of the path for gfx950 (wavefront reductions, no matrix cores):
//   LayerNorm forward / backward          (models/DeformCrossTransMIL.py:44,71,75,90,144; mil.py:175,187)
//   column sums / means over tokens       (Pooler mean, DeformCrossTransMIL.py:193; bias gradients)
//   ReLU backward                         (_fc1, DeformCrossTransMIL.py:83)
//   LayerNorm + mean over tokens          (the path's final norm: one pass over x, the normalised tensor is never stored)
// LayerNorm: the generic kernels put one wave on one row (lane l owns columns l, l + 64, ...; C <= 1024); at C = 128 - the path's token
// width - that is one 512-byte row in flight per wave and latency-bound, so both directions have a 128-column kernel: a half-wave per
// row, one float4 per lane, several rows of loads in flight per wave, grid-stride loop.  Partial column sums leave a workgroup
// through float atomics, or - the deterministic entry points - as a row of a partial slab that is summed in a fixed order.
#include <algorithm>
#include "smml_common.h"

namespace {

constexpr int MAXV = 16;   // per-lane elements: supports C <= 1024

// y = (x - mean) * rstd * gamma + beta ; saves mean / rstd per row
__global__ __launch_bounds__(256) void layernorm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ y,
                                                            float* __restrict__ mean, float* __restrict__ rstd, long long R,
                                                            int C, float eps) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const float* xr = x + row * C;
  float v[MAXV];
  float s = 0.f;
  const int nv = (C + 63) >> 6;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    if (i < nv) {
      const int c = lane + 64 * i;
      v[i] = (c < C) ? xr[c] : 0.f;
      s += v[i];
    }
  }
  const float mu = wave_sum(s) / (float)C;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    if (i < nv) {
      const int c = lane + 64 * i;
      const float d = (c < C) ? v[i] - mu : 0.f;
      ss += d * d;
    }
  }
  const float rs = rsqrtf(wave_sum(ss) / (float)C + eps);
  float* yr = y + row * C;
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    if (i < nv) {
      const int c = lane + 64 * i;
      if (c < C) yr[c] = (v[i] - mu) * rs * gamma[c] + beta[c];
    }
  }
  if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
}

// sum over the 128 columns of a row held by a half-wave (lane hl: columns 4 hl .. 4 hl + 3), IN THE ORDER OF wave_sum() OVER THE GENERIC
// KERNEL'S LAYOUT, so that the 128-column kernel returns the generic kernel's bits: there lane l first adds columns l and l + 64 (the
// "leaf" t), then neighbouring lanes are added pairwise at distances 1, 2, 4, 8 inside each row of 16 lanes, then the four rows from
// left to right.  t0..t3: the leaves of columns 4 (hl & 15) + 0..3 - lanes hl and hl ^ 16 hold the same four
__device__ __forceinline__ float row128_sum(float t0, float t1, float t2, float t3) {
  float v = (t0 + t1) + (t2 + t3);
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);                                        // lanes 4 k .. 4 k + 3: columns 16 k .. 16 k + 15 (and + 64)
  const float r0 = __shfl(v, 0, 32), r1 = __shfl(v, 4, 32), r2 = __shfl(v, 8, 32), r3 = __shfl(v, 12, 32);
  return ((r0 + r1) + r2) + r3;
}

// C = 128 (the path's token width), the forward sibling of layernorm_bwd128_kernel: a half-wave per row, one float4 per lane,
// LN128_RPT rows per half-wave and trip - eight rows of loads in flight per wave instead of one.  Two-pass (mean, then the centred sum
// of squares) with every sum and product in the generic kernel's order (row128_sum; leaf of the squares = fma(d_hi, d_hi, d_lo d_lo);
// y = fma(d rstd, gamma, beta)): y, mean and rstd are bit-identical to layernorm_fwd_kernel's.
constexpr int LN128_RPT = 4;
__global__ __launch_bounds__(256) void layernorm_fwd128_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float* __restrict__ y,
                                                               float* __restrict__ mean, float* __restrict__ rstd, long long R,
                                                               float eps) {
  constexpr int C = 128, U = LN128_RPT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hl = lane & 31, half = lane >> 5;
  const bool low = hl < 16;                                     // this lane's columns are the c (not the c + 64) of their leaves
  const float4 gm = *reinterpret_cast<const float4*>(gamma + 4 * hl), bt = *reinterpret_cast<const float4*>(beta + 4 * hl);
  const long long stride = (long long)gridDim.x * (8 * U);     // rows per trip of the whole grid: 4 waves x 2 halves x U
  for (long long base = ((long long)blockIdx.x * 4 + wave) * (2 * U); base < R; base += stride) {
    float4 xv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long row = base + 2 * u + half;
      xv[u] = *reinterpret_cast<const float4*>(x + (row < R ? row : R - 1) * C + 4 * hl);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long row = base + 2 * u + half;
      const float4 own = xv[u];
      const float4 oth = make_float4(__shfl_xor(own.x, 16), __shfl_xor(own.y, 16), __shfl_xor(own.z, 16), __shfl_xor(own.w, 16));
      const float4 lo = low ? own : oth, hi = low ? oth : own;
      const float mu = row128_sum((0.f + lo.x) + hi.x, (0.f + lo.y) + hi.y, (0.f + lo.z) + hi.z, (0.f + lo.w) + hi.w) / (float)C;
      const float4 dl = make_float4(lo.x - mu, lo.y - mu, lo.z - mu, lo.w - mu);
      const float4 dh = make_float4(hi.x - mu, hi.y - mu, hi.z - mu, hi.w - mu);
      const float ss = row128_sum(fmaf(dh.x, dh.x, dl.x * dl.x), fmaf(dh.y, dh.y, dl.y * dl.y), fmaf(dh.z, dh.z, dl.z * dl.z),
                                  fmaf(dh.w, dh.w, dl.w * dl.w));
      const float rs = rsqrtf(ss / (float)C + eps);
      if (row < R) {
        const float4 d = low ? dl : dh;
        *reinterpret_cast<float4*>(y + row * C + 4 * hl) = make_float4(fmaf(d.x * rs, gm.x, bt.x), fmaf(d.y * rs, gm.y, bt.y),
                                                                       fmaf(d.z * rs, gm.z, bt.z), fmaf(d.w * rs, gm.w, bt.w));
        if (hl == 0) { mean[row] = mu; rstd[row] = rs; }
      }
    }
  }
}

// The mean over a bag's tokens of LayerNorm(x) without y in memory (the final norm of the path: y was written, then read back once by the
// column sums): x [nb, n, 128]; workgroup (chunk, b) takes rows [chunk rows_per_chunk, ...) of bag b, forms each row's mean, rstd and y in
// registers exactly as layernorm_fwd128_kernel does (mean / rstd: its bits), adds y per lane over the rows a half-wave meets, the eight
// half-waves in ascending order, times scale (1 / n) - then out[b, c] += that (float atomics) or part[chunk][b][c] = that (deterministic form)
__global__ __launch_bounds__(256) void layernorm_fwd128_mean_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float* __restrict__ mean,
                                                                    float* __restrict__ rstd, float* __restrict__ out, long long n,
                                                                    float eps, float scale, int rows_per_chunk, float* __restrict__ part) {
  constexpr int C = 128, U = LN128_RPT;
  __shared__ float red[8][C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hl = lane & 31, half = lane >> 5;
  const int b = blockIdx.y;
  const bool low = hl < 16;
  const float4 gm = *reinterpret_cast<const float4*>(gamma + 4 * hl), bt = *reinterpret_cast<const float4*>(beta + 4 * hl);
  const long long lo_row = (long long)blockIdx.x * rows_per_chunk, hi_row = min(n, lo_row + rows_per_chunk);   // lo_row < n: the host's grid
  const float* xb = x + (long long)b * n * C;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long long base = lo_row + wave * (2 * U); base < hi_row; base += 8 * U) {
    float4 xv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long row = base + 2 * u + half;
      xv[u] = *reinterpret_cast<const float4*>(xb + (row < hi_row ? row : hi_row - 1) * C + 4 * hl);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long row = base + 2 * u + half;
      const float4 own = xv[u];
      const float4 oth = make_float4(__shfl_xor(own.x, 16), __shfl_xor(own.y, 16), __shfl_xor(own.z, 16), __shfl_xor(own.w, 16));
      const float4 lo = low ? own : oth, hi = low ? oth : own;
      const float mu = row128_sum((0.f + lo.x) + hi.x, (0.f + lo.y) + hi.y, (0.f + lo.z) + hi.z, (0.f + lo.w) + hi.w) / (float)C;
      const float4 dl = make_float4(lo.x - mu, lo.y - mu, lo.z - mu, lo.w - mu);
      const float4 dh = make_float4(hi.x - mu, hi.y - mu, hi.z - mu, hi.w - mu);
      const float ss = row128_sum(fmaf(dh.x, dh.x, dl.x * dl.x), fmaf(dh.y, dh.y, dl.y * dl.y), fmaf(dh.z, dh.z, dl.z * dl.z),
                                  fmaf(dh.w, dh.w, dl.w * dl.w));
      const float rs = rsqrtf(ss / (float)C + eps);
      if (row < hi_row) {
        const float4 d = low ? dl : dh;
        acc.x += fmaf(d.x * rs, gm.x, bt.x); acc.y += fmaf(d.y * rs, gm.y, bt.y);
        acc.z += fmaf(d.z * rs, gm.z, bt.z); acc.w += fmaf(d.w * rs, gm.w, bt.w);
        if (hl == 0) { mean[(long long)b * n + row] = mu; rstd[(long long)b * n + row] = rs; }
      }
    }
  }
  *reinterpret_cast<float4*>(&red[wave * 2 + half][4 * hl]) = acc;
  __syncthreads();
  if (threadIdx.x < C) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += red[i][threadIdx.x];
    t *= scale;
    if (part) part[((size_t)blockIdx.x * gridDim.y + b) * C + threadIdx.x] = t;
    else atomicAdd(&out[(long long)b * C + threadIdx.x], t);
  }
}

// a + b rounded once, never contracted with a product that feeds it (the compiler fuses a * b + c across statements by default, and
// HIP's __fadd_rn is a plain +): what accumulate_dx adds must be the bits of a separate elementwise add
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

// dx (+)= rstd * (g dy - mean(g dy) - xhat * mean(g dy xhat)); dgamma += sum dy xhat; dbeta += sum dy
// dy row for x row i is dy[(i / rows_per_dy) * C ...] * dy_scale  (rows_per_dy > 1: broadcast rows, e.g. the
// gradient of a mean over tokens).
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                            const float* __restrict__ gamma, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, float* __restrict__ dx,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            long long R, int C, long long rows_per_dy, float dy_scale,
                                                            int accumulate_dx, float* __restrict__ part) {
  __shared__ float red[2][4][64 * MAXV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int nv = (C + 63) >> 6;
  float ag[MAXV], ab[MAXV], gm[MAXV];
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    ag[i] = 0.f; ab[i] = 0.f;
    const int c = lane + 64 * i;
    gm[i] = (i < nv && c < C) ? gamma[c] : 0.f;
  }
  for (long long row = (long long)blockIdx.x * 4 + wave; row < R; row += (long long)gridDim.x * 4) {
    const float* xr = x + row * C;
    const float* dr = dy + (row / rows_per_dy) * C;
    const float mu = mean[row], rs = rstd[row];
    float xh[MAXV], gd[MAXV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      if (i < nv) {
        const int c = lane + 64 * i;
        const bool ok = c < C;
        const float d = ok ? dr[c] * dy_scale : 0.f;
        xh[i] = ok ? (xr[c] - mu) * rs : 0.f;
        gd[i] = d * gm[i];
        s1 += gd[i];
        s2 += gd[i] * xh[i];
        ag[i] += d * xh[i];
        ab[i] += d;
      }
    }
    s1 = wave_sum(s1) / (float)C;
    s2 = wave_sum(s2) / (float)C;
    float* dxr = dx + row * C;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
      if (i < nv) {
        const int c = lane + 64 * i;
        if (c < C) {
          const float v = rs * (gd[i] - s1 - xh[i] * s2);
          dxr[c] = accumulate_dx ? add_rn(dxr[c], v) : v;       // a separate add's bits (no contraction with the product)
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < MAXV; ++i) {
    if (i < nv) { red[0][wave][lane + 64 * i] = ag[i]; red[1][wave][lane + 64 * i] = ab[i]; }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    const float g = red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c];
    const float b = red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c];
    if (part) {        // deterministic mode: this workgroup's row of the slab [workgroup][2][C]; slab_reduce_kernel adds the rows in a fixed order
      part[((size_t)blockIdx.x * 2 + 0) * C + c] = g;
      part[((size_t)blockIdx.x * 2 + 1) * C + c] = b;
    } else {
      atomicAdd(&dgamma[c], g);
      atomicAdd(&dbeta[c], b);
    }
  }
}

// sum over the 32 lanes of a half-wave (both halves independently)
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// C = 128 (the path's token width): a half-wave per row, one float4 per lane, LN128_BWD_RPT = two row pairs per trip - four rows of
// loads (x and dy) in flight per wave instead of one (the generic kernel is latency-bound at 128 columns).  Four row pairs per trip, as
// in the forward sibling (122 registers, no scratch), were measured inside the training step at 80 000 rows and are no faster: 42.6 /
// 41.7 -> 42.5 us per plain call - the kernel is not short of loads in flight.  The arithmetic of a row does not
// depend on the trip it falls into: dx is the same bits for any U and grid.
// accumulate_dx: the old dx of all the trip's rows is loaded before the first store, and added with a non-contracted +.
constexpr int LN128_BWD_RPT = 2;
__global__ __launch_bounds__(256) void layernorm_bwd128_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               const float* __restrict__ gamma, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, float* __restrict__ dx,
                                                               float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                               long long R, long long rows_per_dy, float dy_scale,
                                                               int accumulate_dx, float* __restrict__ part) {
  constexpr int C = 128, U = LN128_BWD_RPT;
  __shared__ float red[2][8][C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hl = lane & 31, half = lane >> 5;
  const float4 gm = *reinterpret_cast<const float4*>(gamma + 4 * hl);
  float4 ag = make_float4(0.f, 0.f, 0.f, 0.f), ab = ag;
  const long long stride = (long long)gridDim.x * (8 * U);     // rows per trip of the whole grid: 4 waves x 2 halves x U
  for (long long r0 = ((long long)blockIdx.x * 4 + wave) * (2 * U) + half; r0 < R; r0 += stride) {
    float4 xv[U], dv[U];
    float mu[U], rs[U];
    bool ok[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long row = r0 + 2 * u;
      ok[u] = row < R;
      const long long rr = ok[u] ? row : R - 1;
      xv[u] = *reinterpret_cast<const float4*>(x + rr * C + 4 * hl);
      dv[u] = *reinterpret_cast<const float4*>(dy + (rr / rows_per_dy) * C + 4 * hl);
      mu[u] = mean[rr]; rs[u] = rstd[rr];
    }
    float4 ov[U];
    if (accumulate_dx) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        ov[u] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[u]) ov[u] = *reinterpret_cast<const float4*>(dx + (r0 + 2 * u) * C + 4 * hl);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const float sc = ok[u] ? dy_scale : 0.f;
      const float4 d = make_float4(dv[u].x * sc, dv[u].y * sc, dv[u].z * sc, dv[u].w * sc);
      const float4 xh = make_float4((xv[u].x - mu[u]) * rs[u], (xv[u].y - mu[u]) * rs[u], (xv[u].z - mu[u]) * rs[u],
                                    (xv[u].w - mu[u]) * rs[u]);
      const float4 gd = make_float4(d.x * gm.x, d.y * gm.y, d.z * gm.z, d.w * gm.w);
      float s1 = (gd.x + gd.y) + (gd.z + gd.w);
      float s2 = (gd.x * xh.x + gd.y * xh.y) + (gd.z * xh.z + gd.w * xh.w);
      ag.x += d.x * xh.x; ag.y += d.y * xh.y; ag.z += d.z * xh.z; ag.w += d.w * xh.w;
      ab.x += d.x; ab.y += d.y; ab.z += d.z; ab.w += d.w;
      s1 = half_sum(s1) * (1.f / C);
      s2 = half_sum(s2) * (1.f / C);
      if (ok[u]) {
        float4* dxr = reinterpret_cast<float4*>(dx + (r0 + 2 * u) * C + 4 * hl);
        float4 v = make_float4(rs[u] * (gd.x - s1 - xh.x * s2), rs[u] * (gd.y - s1 - xh.y * s2),
                               rs[u] * (gd.z - s1 - xh.z * s2), rs[u] * (gd.w - s1 - xh.w * s2));
        if (accumulate_dx) {        // one rounding of old + new (no contraction with the product above): the bits of a separate add
          const float4 o = ov[u];
          v = make_float4(add_rn(v.x, o.x), add_rn(v.y, o.y), add_rn(v.z, o.z), add_rn(v.w, o.w));
        }
        *dxr = v;
      }
    }
  }
  *reinterpret_cast<float4*>(&red[0][wave * 2 + half][4 * hl]) = ag;
  *reinterpret_cast<float4*>(&red[1][wave * 2 + half][4 * hl]) = ab;
  __syncthreads();
  if (threadIdx.x < C) {
    float g = 0.f, bsum = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) { g += red[0][i][threadIdx.x]; bsum += red[1][i][threadIdx.x]; }
    if (part) {        // deterministic mode (see layernorm_bwd_kernel)
      part[((size_t)blockIdx.x * 2 + 0) * C + threadIdx.x] = g;
      part[((size_t)blockIdx.x * 2 + 1) * C + threadIdx.x] = bsum;
    } else {
      atomicAdd(&dgamma[threadIdx.x], g);
      atomicAdd(&dbeta[threadIdx.x], bsum);
    }
  }
}

// out[b, c] += scale * sum_{r in chunk} x[b, r, c]   (x [nb, R, C] contiguous; out zeroed by the caller)
// part != NULL (deterministic mode): the chunk's scaled sums are stored to part[chunk][b][C] instead; slab_reduce_kernel adds the chunks
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ x, float* __restrict__ out, long long R,
                                                     int C, float scale, int rows_per_block, float* __restrict__ part) {
  __shared__ float red[256];
  const int b = blockIdx.y;
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r1 = min(R, r0 + rows_per_block);
  // thread -> (column group, row lane): C <= 256 columns handled per pass
  for (int cb = 0; cb < C; cb += 256) {
    const int ncol = min(256, C - cb);
    // rows interleaved over 256 / ncol_pow2 row lanes
    int cp = 1;
    while (cp < ncol) cp <<= 1;
    const int rl = 256 / cp;
    const int col = threadIdx.x % cp, rlane = threadIdx.x / cp;
    float s = 0.f;
    if (col < ncol && rlane < rl) {
      const float* xb = x + ((long long)b * R) * C + cb + col;
      for (long long r = r0 + rlane; r < r1; r += rl) s += xb[r * C];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < cp && threadIdx.x < ncol) {
      float t = 0.f;
      for (int k = 0; k < rl; ++k) t += red[k * cp + threadIdx.x];
      if (part) part[((size_t)blockIdx.x * gridDim.y + b) * C + cb + threadIdx.x] = t * scale;
      else atomicAdd(&out[(long long)b * C + cb + threadIdx.x], t * scale);
    }
    __syncthreads();
  }
}

// the same for C % 4 == 0 and C <= 1024 (every bias gradient of the path: C = 128 / 512): 16-byte loads, a thread owns four columns and
// every (256 / (C / 4))-th row of its block's chunk, eight loads in flight per thread (the scalar form above read 41 MB in 26 us
// = 1.6 TB/s; this one is HBM-paced)
__global__ __launch_bounds__(256) void colsum4_kernel(const float* __restrict__ x, float* __restrict__ out, long long R, int C,
                                                      float scale, int rows_per_block, float* __restrict__ part) {
  __shared__ float4 red[256];
  const int b = blockIdx.y;
  const int cq = C >> 2;                               // float4 columns (<= 256)
  const int rl = 256 / cq;                             // row lanes
  const int col = threadIdx.x % cq, rlane = threadIdx.x / cq;
  const long long r0 = (long long)blockIdx.x * rows_per_block, r1 = min(R, r0 + rows_per_block);
  float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0, s3 = s0;
  if (rlane < rl) {
    const float4* xb = reinterpret_cast<const float4*>(x + ((long long)b * R) * C) + col;
    long long r = r0 + rlane;
    for (; r + 7LL * rl < r1; r += 8LL * rl) {
      const float4 a0 = xb[r * cq], a1 = xb[(r + rl) * cq], a2 = xb[(r + 2LL * rl) * cq], a3 = xb[(r + 3LL * rl) * cq];
      const float4 a4 = xb[(r + 4LL * rl) * cq], a5 = xb[(r + 5LL * rl) * cq], a6 = xb[(r + 6LL * rl) * cq], a7 = xb[(r + 7LL * rl) * cq];
      s0.x += a0.x + a4.x; s0.y += a0.y + a4.y; s0.z += a0.z + a4.z; s0.w += a0.w + a4.w;
      s1.x += a1.x + a5.x; s1.y += a1.y + a5.y; s1.z += a1.z + a5.z; s1.w += a1.w + a5.w;
      s2.x += a2.x + a6.x; s2.y += a2.y + a6.y; s2.z += a2.z + a6.z; s2.w += a2.w + a6.w;
      s3.x += a3.x + a7.x; s3.y += a3.y + a7.y; s3.z += a3.z + a7.z; s3.w += a3.w + a7.w;
    }
    for (; r < r1; r += rl) { const float4 a = xb[r * cq]; s0.x += a.x; s0.y += a.y; s0.z += a.z; s0.w += a.w; }
  }
  red[threadIdx.x] = make_float4((s0.x + s1.x) + (s2.x + s3.x), (s0.y + s1.y) + (s2.y + s3.y), (s0.z + s1.z) + (s2.z + s3.z),
                                 (s0.w + s1.w) + (s2.w + s3.w));
  __syncthreads();
  if (threadIdx.x < cq) {
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k < rl; ++k) { const float4 v = red[k * cq + threadIdx.x]; t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w; }
    if (part) {
      *reinterpret_cast<float4*>(part + ((size_t)blockIdx.x * gridDim.y + b) * C + 4 * threadIdx.x) =
          make_float4(t.x * scale, t.y * scale, t.z * scale, t.w * scale);
    } else {
      float* o = out + (long long)b * C + 4 * threadIdx.x;
      atomicAdd(o, t.x * scale); atomicAdd(o + 1, t.y * scale); atomicAdd(o + 2, t.z * scale); atomicAdd(o + 3, t.w * scale);
    }
  }
}

// Fixed-order column sums of a partial slab [nrows][ncols] (the deterministic forms of the LayerNorm backward and of the column sums): a
// workgroup owns 32 columns; row lane l of 8 adds rows l, l + 8, ... in ascending order, then one thread per column adds the eight lane sums,
// lane 0 first.  Column c goes to out0[c] (c < split) or out1[c - split]; add: the sum is added onto what is there (dgamma / dbeta are
// accumulated into), else it is stored.
__global__ __launch_bounds__(256) void slab_reduce_kernel(const float* __restrict__ part, long long nrows, long long ncols,
                                                          float* __restrict__ out0, float* __restrict__ out1, long long split, int add) {
  __shared__ float red[8][32];
  const int cl = threadIdx.x & 31, rl = threadIdx.x >> 5;
  const long long c = (long long)blockIdx.x * 32 + cl;
  float s = 0.f;
  if (c < ncols)
    for (long long r = rl; r < nrows; r += 8) s += part[r * ncols + c];
  red[rl][cl] = s;
  __syncthreads();
  if (rl == 0 && c < ncols) {
    float t = red[0][cl];
#pragma unroll
    for (int k = 1; k < 8; ++k) t += red[k][cl];
    float* o = c < split ? out0 + c : out1 + (c - split);
    *o = add ? *o + t : t;
  }
}

__global__ void relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ y, float* __restrict__ dx,
                                long long n) {
  const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 3 < n) {
    const float4 d = *reinterpret_cast<const float4*>(dy + i), v = *reinterpret_cast<const float4*>(y + i);
    *reinterpret_cast<float4*>(dx + i) =
        make_float4(v.x > 0.f ? d.x : 0.f, v.y > 0.f ? d.y : 0.f, v.z > 0.f ? d.z : 0.f, v.w > 0.f ? d.w : 0.f);
  } else {
    for (long long k = i; k < n; ++k) dx[k] = y[k] > 0.f ? dy[k] : 0.f;
  }
}


// OrthogonalLoss (models/cmta_utils.py:1217-1228): one wave per sample, five |cosine similarities| of the
// Tail of BatchLoss (utils/loss.py:26-40) after the two Gram products: S = G_o / ||G_o||_row, V = mean_g G_v[g] / ||G_v[g]||_row,
// L = (S - V)^2 / N - and its backward - on [R, R] / [nv, R, R] matrices with R = batch x world <= 64: one workgroup, one thread per row.
// (In torch this tail is ~30 launch-bound ATen kernels per loss and direction: norm, div, stack, mean, sub, pow, div and their autograd twins.)
//   dL given:  dS = 2 (S - V) dL / N;  d G_o row i = (dS_i - S_i (S_i . dS_i)) / ||G_o,i||;  the same through each G_v[g] with -dS / nv
__global__ __launch_bounds__(64) void batchloss_tail_kernel(const float* __restrict__ Go, const float* __restrict__ Gv,
                                                            const float* __restrict__ dL, float* __restrict__ L,
                                                            float* __restrict__ dGo, float* __restrict__ dGv, int R, int nv, float Nf) {
  const int i = threadIdx.x;
  if (i >= R) return;
  const float* go = Go + (size_t)i * R;
  float no = 0.f;
  for (int j = 0; j < R; ++j) no = fmaf(go[j], go[j], no);
  no = sqrtf(no);
  float nvn[16];
  for (int g = 0; g < nv; ++g) {
    const float* gv = Gv + ((size_t)g * R + i) * R;
    float t = 0.f;
    for (int j = 0; j < R; ++j) t = fmaf(gv[j], gv[j], t);
    nvn[g] = sqrtf(t);
  }
  const float invn = 1.f / (float)nv;
  if (!dL) {
    for (int j = 0; j < R; ++j) {
      float v = 0.f;
      for (int g = 0; g < nv; ++g) v += Gv[((size_t)g * R + i) * R + j] / nvn[g];
      const float d = go[j] / no - v * invn;
      L[(size_t)i * R + j] = d * d / Nf;
    }
    return;
  }
  // backward: dS row, its projection on S, then the same per vgrid group
  float sdot = 0.f;
  float vdot[16];
  for (int g = 0; g < nv; ++g) vdot[g] = 0.f;
  for (int j = 0; j < R; ++j) {
    float v = 0.f;
    for (int g = 0; g < nv; ++g) v += Gv[((size_t)g * R + i) * R + j] / nvn[g];
    const float s = go[j] / no;
    const float ds = 2.f * (s - v * invn) * dL[(size_t)i * R + j] / Nf;
    sdot = fmaf(s, ds, sdot);
    for (int g = 0; g < nv; ++g) vdot[g] = fmaf(Gv[((size_t)g * R + i) * R + j] / nvn[g], -ds * invn, vdot[g]);
  }
  for (int j = 0; j < R; ++j) {
    float v = 0.f;
    for (int g = 0; g < nv; ++g) v += Gv[((size_t)g * R + i) * R + j] / nvn[g];
    const float s = go[j] / no;
    const float ds = 2.f * (s - v * invn) * dL[(size_t)i * R + j] / Nf;
    dGo[(size_t)i * R + j] = (ds - s * sdot) / no;
    for (int g = 0; g < nv; ++g) {
      const float y = Gv[((size_t)g * R + i) * R + j] / nvn[g];
      dGv[((size_t)g * R + i) * R + j] = (-ds * invn - y * vdot[g]) / nvn[g];
    }
  }
}

// rows P, P_hat, G, G_hat [B, D] by wavefront reductions:
//   loss = (1 - |cos(sg P, Ph)|) + (1 - |cos(sg G, Gh)|) + gamma (|cos(P, G)| + |cos(sg P, Gh)| + |cos(sg G, Ph)|)
// (sg = stop-gradient / .detach()).  Backward in the same kernel family: d cos(a,b)/da = b/(|a||b|) - cos a/|a|^2.
__global__ __launch_bounds__(64) void orth_loss_kernel(const float* __restrict__ P, const float* __restrict__ Ph,
                                                       const float* __restrict__ G, const float* __restrict__ Gh,
                                                       const float* __restrict__ dloss, float* __restrict__ loss,
                                                       float* __restrict__ dP, float* __restrict__ dPh, float* __restrict__ dG,
                                                       float* __restrict__ dGh, int D, float gamma, float eps) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const float *p = P + (long long)b * D, *ph = Ph + (long long)b * D, *g = G + (long long)b * D, *gh = Gh + (long long)b * D;
  float pp = 0, hh = 0, gg = 0, kk = 0, p_ph = 0, g_gh = 0, p_g = 0, p_gh = 0, g_ph = 0;
  for (int i = lane; i < D; i += 64) {
    const float a = p[i], c = ph[i], e = g[i], f = gh[i];
    pp = fmaf(a, a, pp); hh = fmaf(c, c, hh); gg = fmaf(e, e, gg); kk = fmaf(f, f, kk);
    p_ph = fmaf(a, c, p_ph); g_gh = fmaf(e, f, g_gh); p_g = fmaf(a, e, p_g); p_gh = fmaf(a, f, p_gh); g_ph = fmaf(e, c, g_ph);
  }
  pp = wave_sum(pp); hh = wave_sum(hh); gg = wave_sum(gg); kk = wave_sum(kk);
  p_ph = wave_sum(p_ph); g_gh = wave_sum(g_gh); p_g = wave_sum(p_g); p_gh = wave_sum(p_gh); g_ph = wave_sum(g_ph);
  const float np = fmaxf(sqrtf(pp), eps), nh = fmaxf(sqrtf(hh), eps), ng = fmaxf(sqrtf(gg), eps), nk = fmaxf(sqrtf(kk), eps);
  const float c1 = p_ph / (np * nh), c2 = g_gh / (ng * nk), c3 = p_g / (np * ng), c4 = p_gh / (np * nk), c5 = g_ph / (ng * nh);
  if (loss && lane == 0) loss[b] = (1.f - fabsf(c1)) + (1.f - fabsf(c2)) + gamma * (fabsf(c3) + fabsf(c4) + fabsf(c5));
  if (!dloss) return;
  const float go = dloss[b];
  const float s1 = -copysignf(1.f, c1) * go, s2 = -copysignf(1.f, c2) * go;                       // pos pairs
  const float s3 = gamma * copysignf(1.f, c3) * go, s4 = gamma * copysignf(1.f, c4) * go, s5 = gamma * copysignf(1.f, c5) * go;
  for (int i = lane; i < D; i += 64) {
    const float a = p[i], c = ph[i], e = g[i], f = gh[i];
    // d cos(x, y) / dy = x / (|x||y|) - cos * y / |y|^2
    dPh[(long long)b * D + i] = s1 * (a / (np * nh) - c1 * c / (nh * nh)) + s5 * (e / (ng * nh) - c5 * c / (nh * nh));
    dGh[(long long)b * D + i] = s2 * (e / (ng * nk) - c2 * f / (nk * nk)) + s4 * (a / (np * nk) - c4 * f / (nk * nk));
    dP[(long long)b * D + i] = s3 * (e / (np * ng) - c3 * a / (np * np));                       // only cos(P, G) carries grad to P
    dG[(long long)b * D + i] = s3 * (a / (np * ng) - c3 * e / (ng * ng));
  }
}

}  // namespace

extern "C" {

int smml_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd,
                           long long R, int C, float eps, void* stream) {
  SMML_REQUIRE(x && gamma && beta && y && mean && rstd, "smml_layernorm_fwd_f32: null pointer");
  SMML_REQUIRE(R > 0 && C > 0 && C <= 64 * MAXV, "smml_layernorm_fwd_f32: need 0 < C <= %d (got %d)", 64 * MAXV, C);
  const bool aligned = ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(y) | reinterpret_cast<size_t>(gamma) |
                         reinterpret_cast<size_t>(beta)) & 15) == 0;
  if (C == 128 && aligned) {
    const long long nb = (R + 8 * LN128_RPT - 1) / (8 * LN128_RPT);
    hipLaunchKernelGGL(layernorm_fwd128_kernel, dim3((unsigned)(nb < 2048 ? nb : 2048)), dim3(256), 0, (hipStream_t)stream, x, gamma,
                       beta, y, mean, rstd, R, eps);
  } else
  hipLaunchKernelGGL(layernorm_fwd_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, gamma,
                     beta, y, mean, rstd, R, C, eps);
  SMML_LAUNCH_CHECK("smml_layernorm_fwd_f32");
  return SMML_OK;
}

// rows per chunk of layernorm_fwd128_mean_kernel - a function of the bag length alone, the same in both forms: two trips of a workgroup
// (64 rows), more only for bags beyond 131 072 tokens (at most 2048 chunks per bag); a multiple of the 32 rows of a trip.  Bags of up to
// 1024 tokens keep the 512-row chunks of the column sums this kernel replaces: at most two chunks, and two atomic adds onto zero commute,
// so small bags stay run-to-run identical in the default form as they were.
static long long layernorm_mean_rows_per_chunk(long long n) {
  if (n <= 1024) return 512;
  const long long want = (n + 2047) / 2048;
  return want <= 64 ? 64 : (want + 31) / 32 * 32;
}

static int layernorm_mean_launch(const char* fn, const float* x, const float* gamma, const float* beta, float* mean, float* rstd,
                                 float* out, int nb, long long n, int C, float eps, float* part, void* stream) {
  SMML_REQUIRE(x && gamma && beta && mean && rstd && out, "%s: null pointer", fn);
  SMML_REQUIRE(nb > 0 && nb <= 65535 && n > 0, "%s: need 0 < nb <= 65535 bags of n > 0 rows", fn);
  SMML_REQUIRE(C == 128, "%s: the fused token mean has a 128-column kernel only (got C = %d)", fn, C);
  SMML_REQUIRE(((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(gamma) | reinterpret_cast<size_t>(beta)) & 15) == 0,
               "%s: x, gamma and beta must be 16-byte aligned", fn);
  const long long rpc = layernorm_mean_rows_per_chunk(n), chunks = (n + rpc - 1) / rpc;
  SMML_REQUIRE(rpc <= 2147483647LL && chunks <= 2147483647LL, "%s: too many rows", fn);
  hipLaunchKernelGGL(layernorm_fwd128_mean_kernel, dim3((unsigned)chunks, (unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, gamma, beta,
                     mean, rstd, out, n, eps, 1.f / (float)n, (int)rpc, part);
  return SMML_OK;
}

// out [nb, C] must be zeroed by the caller; out[b, c] += (1 / n) sum_r LayerNorm(x)[b, r, c]; mean / rstd [nb n] as smml_layernorm_fwd_f32 saves them
int smml_layernorm_fwd_mean_f32(const float* x, const float* gamma, const float* beta, float* mean, float* rstd, float* out, int nb,
                                long long n, int C, float eps, void* stream) {
  if (int rc = layernorm_mean_launch("smml_layernorm_fwd_mean_f32", x, gamma, beta, mean, rstd, out, nb, n, C, eps, nullptr, stream)) return rc;
  SMML_LAUNCH_CHECK("smml_layernorm_fwd_mean_f32");
  return SMML_OK;
}

size_t smml_layernorm_fwd_mean_det_workspace_bytes(int nb, long long n, int C) {
  if (nb <= 0 || n <= 0 || C != 128) return 0;
  const long long rpc = layernorm_mean_rows_per_chunk(n);
  return (size_t)((n + rpc - 1) / rpc) * (size_t)nb * (size_t)C * sizeof(float);
}

// the same with out OVERWRITTEN by a fixed-order sum: chunk sums to workspace[chunk][nb][C], then slab_reduce_kernel over the chunks
int smml_layernorm_fwd_mean_det_f32(const float* x, const float* gamma, const float* beta, float* mean, float* rstd, float* out, int nb,
                                    long long n, int C, float eps, void* workspace, size_t workspace_bytes, void* stream) {
  SMML_REQUIRE(workspace && out, "smml_layernorm_fwd_mean_det_f32: null pointer");
  SMML_REQUIRE(nb > 0 && n > 0 && C == 128, "smml_layernorm_fwd_mean_det_f32: need nb > 0, n > 0 and C = 128");
  SMML_REQUIRE(workspace_bytes >= smml_layernorm_fwd_mean_det_workspace_bytes(nb, n, C), "smml_layernorm_fwd_mean_det_f32: workspace too small");
  const long long rpc = layernorm_mean_rows_per_chunk(n), chunks = (n + rpc - 1) / rpc;
  float* part = chunks == 1 ? out : (float*)workspace;      // a single chunk is the result itself ([1][nb][C]): no second pass
  if (int rc = layernorm_mean_launch("smml_layernorm_fwd_mean_det_f32", x, gamma, beta, mean, rstd, out, nb, n, C, eps, part, stream)) return rc;
  SMML_LAUNCH_CHECK("smml_layernorm_fwd_mean_det_f32");
  if (chunks == 1) return SMML_OK;
  const long long ncols = (long long)nb * C;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((ncols + 31) / 32)), dim3(256), 0, (hipStream_t)stream, part, chunks, ncols, out,
                     out, ncols, 0);
  SMML_LAUNCH_CHECK("smml_layernorm_fwd_mean_det_f32/reduce");
  return SMML_OK;
}

// grid of layernorm_bwd128_kernel: a workgroup takes 8 LN128_BWD_RPT = 16 rows per trip; at most 768 workgroups (the slab rows of the
// deterministic form's workspace formula in include/smml.h)
static long long layernorm_bwd128_workgroups(long long R) {
  const long long nb = (R + 8 * LN128_BWD_RPT - 1) / (8 * LN128_BWD_RPT);
  return nb < 768 ? nb : 768;
}

// dgamma / dbeta are accumulated into (callers zero them once; the shared LayerNorm of the two streams adds twice)
int smml_layernorm_bwd_f32(const float* x, const float* dy, const float* gamma, const float* mean, const float* rstd,
                           float* dx, float* dgamma, float* dbeta, long long R, int C, long long rows_per_dy,
                           float dy_scale, int accumulate_dx, void* stream) {
  SMML_REQUIRE(x && dy && gamma && mean && rstd && dx && dgamma && dbeta, "smml_layernorm_bwd_f32: null pointer");
  SMML_REQUIRE(R > 0 && C > 0 && C <= 64 * MAXV, "smml_layernorm_bwd_f32: need 0 < C <= %d (got %d)", 64 * MAXV, C);
  SMML_REQUIRE(rows_per_dy >= 1, "smml_layernorm_bwd_f32: rows_per_dy must be >= 1");
  const long long nblk = (R + 3) / 4;
  const bool aligned = ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(dy) | reinterpret_cast<size_t>(dx) |
                         reinterpret_cast<size_t>(gamma)) & 15) == 0;
  if (C == 128 && aligned) {
    hipLaunchKernelGGL(layernorm_bwd128_kernel, dim3((unsigned)layernorm_bwd128_workgroups(R)), dim3(256), 0, (hipStream_t)stream,
                       x, dy, gamma, mean, rstd, dx, dgamma, dbeta, R, rows_per_dy, dy_scale, accumulate_dx, (float*)nullptr);
  } else
  hipLaunchKernelGGL(layernorm_bwd_kernel, dim3((unsigned)(nblk < 1024 ? nblk : 1024)), dim3(256), 0, (hipStream_t)stream,
                     x, dy, gamma, mean, rstd, dx, dgamma, dbeta, R, C, rows_per_dy, dy_scale, accumulate_dx, (float*)nullptr);
  SMML_LAUNCH_CHECK("smml_layernorm_bwd_f32");
  return SMML_OK;
}

// out [nb, C] must be zeroed by the caller; out[b, c] += scale * sum_r x[b, r, c]
int smml_colsum_f32(const float* x, float* out, int nb, long long R, int C, float scale, void* stream) {
  SMML_REQUIRE(x && out && nb > 0 && R > 0 && C > 0, "smml_colsum_f32: bad argument");
  SMML_REQUIRE(nb <= 65535, "smml_colsum_f32: too many batches");
  if ((C & 3) == 0 && C <= 1024 && 256 % (C >> 2) == 0 && ((reinterpret_cast<size_t>(x) & 15) == 0)) {
    // enough blocks to fill the chip a few times, at least 64 rows per row lane
    const int rl = 256 / (C >> 2);
    long long rpb = std::max<long long>(64LL * rl, (R * nb + 2047) / 2048);
    rpb = (rpb + rl - 1) / rl * rl;
    const long long nb4 = (R + rpb - 1) / rpb;
    hipLaunchKernelGGL(colsum4_kernel, dim3((unsigned)nb4, (unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, out, R, C, scale, (int)rpb, (float*)nullptr);
    SMML_LAUNCH_CHECK("smml_colsum_f32/4");
    return SMML_OK;
  }
  int rows_per_block = 256;
  long long nblk = (R + rows_per_block - 1) / rows_per_block;
  hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)nblk, (unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, out, R, C,
                     scale, rows_per_block, (float*)nullptr);
  SMML_LAUNCH_CHECK("smml_colsum_f32");
  return SMML_OK;
}

// ---- deterministic forms: partial rows to a caller-allocated workspace with plain stores, then slab_reduce_kernel (no float atomics)
// workgroups of the LayerNorm backward - a function of (R, C) alone: the 128-column kernel's grid at C = 128, else the generic kernel's
static long long layernorm_bwd_det_workgroups(long long R, int C) {
  if (C == 128) return layernorm_bwd128_workgroups(R);
  const long long nblk = (R + 3) / 4;
  return nblk < 1024 ? nblk : 1024;
}

size_t smml_layernorm_bwd_det_workspace_bytes(long long R, int C) {
  if (R <= 0 || C <= 0 || C > 64 * MAXV) return 0;
  return (size_t)layernorm_bwd_det_workgroups(R, C) * 2 * (size_t)C * sizeof(float);
}

// smml_layernorm_bwd_f32 with dgamma / dbeta summed in a fixed order (added onto what they hold, as there); dx is that entry point's, bit for bit
int smml_layernorm_bwd_det_f32(const float* x, const float* dy, const float* gamma, const float* mean, const float* rstd,
                               float* dx, float* dgamma, float* dbeta, long long R, int C, long long rows_per_dy,
                               float dy_scale, int accumulate_dx, void* workspace, size_t workspace_bytes, void* stream) {
  SMML_REQUIRE(x && dy && gamma && mean && rstd && dx && dgamma && dbeta && workspace, "smml_layernorm_bwd_det_f32: null pointer");
  SMML_REQUIRE(R > 0 && C > 0 && C <= 64 * MAXV, "smml_layernorm_bwd_det_f32: need 0 < C <= %d (got %d)", 64 * MAXV, C);
  SMML_REQUIRE(rows_per_dy >= 1, "smml_layernorm_bwd_det_f32: rows_per_dy must be >= 1");
  SMML_REQUIRE(workspace_bytes >= smml_layernorm_bwd_det_workspace_bytes(R, C), "smml_layernorm_bwd_det_f32: workspace too small");
  const long long nwg = layernorm_bwd_det_workgroups(R, C);
  float* part = (float*)workspace;
  const bool aligned = ((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(dy) | reinterpret_cast<size_t>(dx) |
                         reinterpret_cast<size_t>(gamma)) & 15) == 0;
  if (C == 128 && aligned)
    hipLaunchKernelGGL(layernorm_bwd128_kernel, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream,
                       x, dy, gamma, mean, rstd, dx, dgamma, dbeta, R, rows_per_dy, dy_scale, accumulate_dx, part);
  else
    hipLaunchKernelGGL(layernorm_bwd_kernel, dim3((unsigned)nwg), dim3(256), 0, (hipStream_t)stream,
                       x, dy, gamma, mean, rstd, dx, dgamma, dbeta, R, C, rows_per_dy, dy_scale, accumulate_dx, part);
  SMML_LAUNCH_CHECK("smml_layernorm_bwd_det_f32");
  hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((2 * C + 31) / 32)), dim3(256), 0, (hipStream_t)stream, part, nwg, (long long)2 * C,
                     dgamma, dbeta, (long long)C, 1);
  SMML_LAUNCH_CHECK("smml_layernorm_bwd_det_f32/reduce");
  return SMML_OK;
}

// rows per chunk of the deterministic column sums - a function of (R, C) alone (smml_colsum_f32 also looks at the batch count): the
// float4 kernel's chunk where C allows it (at least 64 rows per row lane, at most ~2048 chunks), else 256 rows
static long long colsum_det_rows_per_chunk(long long R, int C) {
  if ((C & 3) == 0 && C <= 1024 && 256 % (C >> 2) == 0) {
    const int rl = 256 / (C >> 2);
    const long long rpb = std::max<long long>(64LL * rl, (R + 2047) / 2048);
    return (rpb + rl - 1) / rl * rl;
  }
  return 256;
}

size_t smml_colsum_det_workspace_bytes(int nb, long long R, int C) {
  if (nb <= 0 || R <= 0 || C <= 0) return 0;
  const long long rpc = colsum_det_rows_per_chunk(R, C);
  return (size_t)((R + rpc - 1) / rpc) * (size_t)nb * (size_t)C * sizeof(float);
}

// out[b, c] = scale * sum_r x[b, r, c], overwritten: chunk sums to the workspace [chunks][nb][C], then a fixed-order sum over the chunks
int smml_colsum_det_f32(const float* x, float* out, int nb, long long R, int C, float scale, void* workspace, size_t workspace_bytes,
                        void* stream) {
  SMML_REQUIRE(x && out && workspace && nb > 0 && R > 0 && C > 0, "smml_colsum_det_f32: bad argument");
  SMML_REQUIRE(nb <= 65535, "smml_colsum_det_f32: too many batches");
  SMML_REQUIRE(workspace_bytes >= smml_colsum_det_workspace_bytes(nb, R, C), "smml_colsum_det_f32: workspace too small");
  const long long rpc = colsum_det_rows_per_chunk(R, C), chunks = (R + rpc - 1) / rpc;
  SMML_REQUIRE(rpc <= 2147483647LL && chunks <= 2147483647LL, "smml_colsum_det_f32: too many rows");
  float* part = chunks == 1 ? out : (float*)workspace;      // a single chunk is the result itself ([1][nb][C]): no second pass
  if ((C & 3) == 0 && C <= 1024 && 256 % (C >> 2) == 0 && (((reinterpret_cast<size_t>(x) | reinterpret_cast<size_t>(part)) & 15) == 0))
    hipLaunchKernelGGL(colsum4_kernel, dim3((unsigned)chunks, (unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, out, R, C, scale, (int)rpc, part);
  else
    hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)chunks, (unsigned)nb), dim3(256), 0, (hipStream_t)stream, x, out, R, C, scale, (int)rpc, part);
  SMML_LAUNCH_CHECK("smml_colsum_det_f32");
  if (chunks == 1) return SMML_OK;
  const long long ncols = (long long)nb * C;
  hipLaunchKernelGGL(slab_reduce_kernel, dim3((unsigned)((ncols + 31) / 32)), dim3(256), 0, (hipStream_t)stream, part, chunks, ncols, out,
                     out, ncols, 0);
  SMML_LAUNCH_CHECK("smml_colsum_det_f32/reduce");
  return SMML_OK;
}

// loss [B] (nullable) and, when dloss [B] is given, the four gradients [B, D]
int smml_orth_loss_f32(const float* P, const float* Ph, const float* G, const float* Gh, const float* dloss, float* loss,
                       float* dP, float* dPh, float* dG, float* dGh, int B, int D, float gamma, void* stream) {
  SMML_REQUIRE(P && Ph && G && Gh && B > 0 && D > 0, "smml_orth_loss_f32: bad argument");
  SMML_REQUIRE(loss || dloss, "smml_orth_loss_f32: nothing to compute");
  SMML_REQUIRE(!dloss || (dP && dPh && dG && dGh), "smml_orth_loss_f32: gradient outputs missing");
  hipLaunchKernelGGL(orth_loss_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, P, Ph, G, Gh, dloss, loss, dP, dPh, dG,
                     dGh, D, gamma, 1e-8f);
  SMML_LAUNCH_CHECK("smml_orth_loss_f32");
  return SMML_OK;
}

// BatchLoss tail (utils/loss.py:26-40): go [R, R], gv [nv, R, R] -> loss [R, R] (dloss == NULL) or dgo, dgv (dloss given); R <= 64, nv <= 16
int smml_batchloss_tail_f32(const float* go, const float* gv, const float* dloss, float* loss, float* dgo, float* dgv, int R, int nv,
                            float n_total, void* stream) {
  SMML_REQUIRE(go && gv && R > 0 && R <= 64 && nv > 0 && nv <= 16 && n_total > 0.f, "smml_batchloss_tail_f32: need 0 < R <= 64, 0 < nv <= 16");
  SMML_REQUIRE(dloss ? (dgo && dgv) : (loss != nullptr), "smml_batchloss_tail_f32: outputs missing");
  hipLaunchKernelGGL(batchloss_tail_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, go, gv, dloss, loss, dgo, dgv, R, nv, n_total);
  SMML_LAUNCH_CHECK("smml_batchloss_tail_f32");
  return SMML_OK;
}

int smml_relu_bwd_f32(const float* dy, const float* y, float* dx, long long n, void* stream) {
  SMML_REQUIRE(dy && y && dx && n > 0, "smml_relu_bwd_f32: bad argument");
  const long long nthr = (n + 3) / 4;
  hipLaunchKernelGGL(relu_bwd_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, y, dx, n);
  SMML_LAUNCH_CHECK("smml_relu_bwd_f32");
  return SMML_OK;
}

}  // extern "C"
