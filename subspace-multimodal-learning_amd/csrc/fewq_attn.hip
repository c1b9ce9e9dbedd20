// Few-query co-attention (models/MultiheadAttention.py with L <= 8 queries over a bag of S keys; CMTA's G_in_P_Att, MCAT's coattn): the
// bag-sized core of the folded form
//     raw[b, l, s] = u[b, l] . x[b, s] + c[b, l]        z[b, l] = sum_s softmax_s(raw[b, l, :]) y[b, s]
// with u = q^ Wk, c = q^ . bk formed outside ([B, L, E]-sized GEMMs): the key and value projections never touch the bag, x (= y at every call
// site of the reference) streams once through registers with one online softmax (m_l, l_l, acc_l) per query.
//
//   forward   grid (splits, B), 256 threads.  A workgroup walks its rows in tiles of 16; wave w owns rows 4 w .. 4 w + 3 of a tile: one
//             float4 per lane and 256-column panel, u in registers, L wave-reduced dots per row, the wave's own online softmax.  The four
//             waves' states meet in LDS at the end of the split and are merged in wave order into ONE partial (m[L], l[L], acc[L, Ev]) per
//             split; a second kernel merges a bag's partials in ascending split order into z and lse.  raw is written on the way (masked
//             keys: -inf).
//   backward  the same grid and row ownership, one pass: p = exp(raw - lse), t_l = dz_l . y_s, ds_l = p_l (t_l - kappa_l) + draw_l with
//             kappa_l = dz_l . z_l (from the saved z), the row's gradient sum_l ds_l u_l + sum_l p_l dz_l written once (x is y) or as two rows,
//             du_l / dc_l accumulated per wave, merged in wave order per workgroup, and summed over the splits in ascending order by a third
//             kernel.
// A piece of a bag whose keys are all masked keeps m = -inf and takes 0 as the reference point of its exponentials: it weighs 0, never
// exp(-inf + inf).  A bag whose keys are ALL masked is NaN here as in the reference (precondition of the entry points).
// Every sum has one owner and a fixed order: no float atomics, the results are a function of the inputs and the split count alone.
// Several heads would fold as h L effective queries (u and dz per head on their own column slices of x); the kernels are one-head.
#include "smml_common.h"

#include <algorithm>
#include <math.h>

namespace {

constexpr int FQ_THREADS = 256;
constexpr int FQ_TILE = 16;          // rows per tile: four per wave, in flight together
constexpr int FQ_MAXL = 8;
constexpr int FQ_MAXE = 512;         // two 256-column panels: at most two float4 per lane and row
constexpr int FQ_MIN_ROWS = 64;      // rows per split the heuristic does not go below (the L (Ev + 2) partial stays a few per cent of the reads)
constexpr int FQ_TARGET_WG = 1024;   // workgroups the heuristic aims at: 256 CUs x 4 resident

__device__ __forceinline__ float lane_value(float v, int lane) {
  return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), lane));
}
__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); }
__device__ __forceinline__ void axpy4(float4& a, const float s, const float4 v) {
  a.x = fmaf(s, v.x, a.x); a.y = fmaf(s, v.y, a.y); a.z = fmaf(s, v.z, a.z); a.w = fmaf(s, v.w, a.w);
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// the reference point of a piece's exponentials: its max, or 0 while every key seen so far is masked
__device__ __forceinline__ float finite_ref(float m) { return m == -INFINITY ? 0.f : m; }

// u [B, L, Ek], c [B, L], x [B, S, Ek] (strides xbs, xrs), y [B, S, Ev] (SAME: y is x), mask [B, S] bytes or null
//   -> raw [B, L, S], pacc [B, NS, L, Ev], pml [B, NS, L, 2]; split sp of bag b owns rows [sp rps, min(S, (sp + 1) rps))
// LQ: the queries the registers are laid out for (l >= L: skipped); P: 256-column panels of max(Ek, Ev)
template <int LQ, int P, bool SAME>
__global__ __launch_bounds__(FQ_THREADS) void fewq_fwd_kernel(const float* __restrict__ u, const float* __restrict__ c, const float* __restrict__ x,
                                                              const float* __restrict__ y, const unsigned char* __restrict__ mask,
                                                              float* __restrict__ raw, float* __restrict__ pacc, float* __restrict__ pml,
                                                              const int L, const int S, const int Ek, const int Ev, const long long xbs,
                                                              const long long xrs, const long long ybs, const long long yrs, const int rps) {
  const int b = blockIdx.y, sp = blockIdx.x, NS = gridDim.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = sp * rps, r1 = r0 + min(rps, S - r0);
  // every load is unconditional: a row past the split's end and a column past the width re-read an address that is in range and meet a
  // weight of zero (u = 0, p = 0) or are never stored
  bool kc[P], vc[P];
  int ko[P], vo[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    kc[j] = j * 256 + 4 * lane < Ek; ko[j] = kc[j] ? j * 256 + 4 * lane : 0;
    vc[j] = j * 256 + 4 * lane < Ev; vo[j] = vc[j] ? j * 256 + 4 * lane : 0;
  }
  const float* xb = x + (size_t)b * xbs;
  const float* yb = SAME ? xb : y + (size_t)b * ybs;
  const long long vrs = SAME ? xrs : yrs;

  float4 ur[LQ][P];
  float cr[LQ];
#pragma unroll
  for (int l = 0; l < LQ; ++l) {
    const int lc = min(l, L - 1);
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float4 v = ld4(u + ((size_t)b * L + lc) * Ek + ko[j]);
      ur[l][j] = (l < L && kc[j]) ? v : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    cr[l] = c[(size_t)b * L + lc];
  }
  float m[LQ], ls[LQ];
  float4 acc[LQ][P];
#pragma unroll
  for (int l = 0; l < LQ; ++l) {
    m[l] = -INFINITY; ls[l] = 0.f;
#pragma unroll
    for (int j = 0; j < P; ++j) acc[l][j] = make_float4(0.f, 0.f, 0.f, 0.f);
  }

  for (int t0 = r0; t0 < r1; t0 += FQ_TILE) {
    const int rw = t0 + 4 * wave;
    float4 xr[4][P], yr[SAME ? 1 : 4][SAME ? 1 : P];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const size_t ri = (size_t)min(rw + i, r1 - 1);
#pragma unroll
      for (int j = 0; j < P; ++j) {
        xr[i][j] = ld4(xb + ri * xrs + ko[j]);
        if constexpr (!SAME) yr[i][j] = ld4(yb + ri * vrs + vo[j]);
      }
    }
    // lane 4 l + i speaks for (query l, row rw + i): the mask byte of its row, later the score it stores
    const int li = lane & 3, lq = lane >> 2;
    const bool row_ok = rw + li < r1;
    const unsigned mk = mask ? (unsigned)mask[(size_t)b * S + min(rw + li, r1 - 1)] : 0u;
    const bool keep = row_ok && mk == 0u;                      // lanes 0 .. 3 decide for the tile's four rows
    const unsigned long long keep_bits = __ballot(keep);
    float sv = -INFINITY;
    float s[4][LQ];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = (keep_bits >> i) & 1ull;                 // a masked key and a row past the end score -inf: weight exp(-inf - ref) = 0
#pragma unroll
      for (int l = 0; l < LQ; ++l) {
        if (l < L) {
          float d = 0.f;
#pragma unroll
          for (int j = 0; j < P; ++j) d += dot4(ur[l][j], xr[i][j]);
          d = ok ? wave_sum(d) + cr[l] : -INFINITY;
          s[i][l] = d;
          sv = lane == 4 * l + i ? d : sv;
        } else {
          s[i][l] = -INFINITY;
        }
      }
    }
    if (lq < L && row_ok) raw[((size_t)b * L + lq) * S + rw + li] = sv;
#pragma unroll
    for (int l = 0; l < LQ; ++l) {
      if (l < L) {
        const float mn = fmaxf(m[l], fmaxf(fmaxf(s[0][l], s[1][l]), fmaxf(s[2][l], s[3][l])));
        const float ref = finite_ref(mn);
        const float scale = expf(m[l] - ref);                  // m = -inf: 0 on a zero accumulator
        float p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) p[i] = expf(s[i][l] - ref);
        ls[l] = fmaf(ls[l], scale, (p[0] + p[1]) + (p[2] + p[3]));
        m[l] = mn;
#pragma unroll
        for (int j = 0; j < P; ++j) {
          float4 a = acc[l][j];
          a.x *= scale; a.y *= scale; a.z *= scale; a.w *= scale;
#pragma unroll
          for (int i = 0; i < 4; ++i) axpy4(a, p[i], SAME ? xr[i][j] : yr[SAME ? 0 : i][SAME ? 0 : j]);
          acc[l][j] = a;
        }
      }
    }
  }

  // the four waves' states, merged in wave order, one query at a time (8 KB of LDS)
  __shared__ __attribute__((aligned(16))) float sAcc[4][FQ_MAXE];
  __shared__ float sM[4], sL[4];
  const size_t part = (size_t)b * NS + sp;
#pragma unroll
  for (int l = 0; l < LQ; ++l) {
    if (l < L) {
      __syncthreads();                                         // the previous query's columns have been read
#pragma unroll
      for (int j = 0; j < P; ++j)
        if (vc[j]) *reinterpret_cast<float4*>(&sAcc[wave][vo[j]]) = acc[l][j];
      if (lane == 0) { sM[wave] = m[l]; sL[wave] = ls[l]; }
      __syncthreads();
      const float M = fmaxf(fmaxf(sM[0], sM[1]), fmaxf(sM[2], sM[3]));
      const float ref = finite_ref(M);
      const float w0 = expf(sM[0] - ref), w1 = expf(sM[1] - ref), w2 = expf(sM[2] - ref), w3 = expf(sM[3] - ref);
      float* pa = pacc + (part * L + l) * Ev;
      for (int col = tid; col < Ev; col += FQ_THREADS)
        pa[col] = fmaf(w3, sAcc[3][col], fmaf(w2, sAcc[2][col], fmaf(w1, sAcc[1][col], w0 * sAcc[0][col])));
      if (tid == 0) {
        pml[(part * L + l) * 2] = M;
        pml[(part * L + l) * 2 + 1] = fmaf(w3, sL[3], fmaf(w2, sL[2], fmaf(w1, sL[1], w0 * sL[0])));
      }
    }
  }
}

// partials of (bag b, query l), in ascending split order -> z [B, L, Ev], lse [B, L].  grid (L, B); the split weights exp(m_i - m) of 256
// splits at a time are formed by 256 threads and parked in LDS, the partial rows are read eight at a time
__global__ __launch_bounds__(FQ_THREADS) void fewq_merge_kernel(const float* __restrict__ pacc, const float* __restrict__ pml, float* __restrict__ z,
                                                                float* __restrict__ lse, const int NS, const int L, const int Ev) {
  const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t rs = (size_t)L * Ev;                            // from one split's row of this query to the next split's
  const float* pa = pacc + ((size_t)b * NS * L + l) * Ev;
  const float* ml = pml + ((size_t)b * NS * L + l) * 2;
  __shared__ float mred[4], wS[FQ_THREADS], lwS[FQ_THREADS];
  float m = -INFINITY;
  for (int i = tid; i < NS; i += FQ_THREADS) m = fmaxf(m, ml[(size_t)i * L * 2]);
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
  if (lane == 0) mred[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(mred[0], mred[1]), fmaxf(mred[2], mred[3]));
  const float ref = finite_ref(m);
  const int c0 = min(tid, Ev - 1), c1 = min(tid + FQ_THREADS, Ev - 1);
  float a0 = 0.f, a1 = 0.f, lsum = 0.f;
  for (int s0 = 0; s0 < NS; s0 += FQ_THREADS) {
    const int sn = min(FQ_THREADS, NS - s0);
    __syncthreads();                                           // the previous chunk's weights have been read
    if (tid < sn) {
      const float w = expf(ml[(size_t)(s0 + tid) * L * 2] - ref);      // a split whose keys are all masked: exp(-inf) = 0
      wS[tid] = w;
      lwS[tid] = ml[(size_t)(s0 + tid) * L * 2 + 1] * w;
    }
    __syncthreads();
    for (int i0 = 0; i0 < sn; i0 += 8) {
      float v0[8], v1[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float* row = pa + (size_t)(s0 + min(i0 + k, sn - 1)) * rs;
        v0[k] = row[c0];
        v1[k] = row[c1];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const bool ok = i0 + k < sn;
        const float w = ok ? wS[min(i0 + k, sn - 1)] : 0.f;
        lsum += ok ? lwS[min(i0 + k, sn - 1)] : 0.f;
        a0 = fmaf(w, v0[k], a0);
        a1 = fmaf(w, v1[k], a1);
      }
    }
  }
  const float inv = 1.f / lsum;
  float* zr = z + ((size_t)b * L + l) * Ev;
  if (tid < Ev) zr[tid] = a0 * inv;
  if (tid + FQ_THREADS < Ev) zr[tid + FQ_THREADS] = a1 * inv;
  if (tid == 0) lse[(size_t)b * L + l] = m + logf(lsum);
}

// row stride of the backward partials: du in columns [0, Ek), dc in column Ek
__host__ __device__ constexpr int bwd_part_ld(int Ek) { return Ek + 4; }

// saved raw, lse, z and dz (draw, dlse: optional) -> dx, dy (either may be null: nothing is formed for it; SAME: dx receives dx + dy) and
// part [B, NS, L, Ek + 4]
template <int LQ, int P, bool SAME>
__global__ __launch_bounds__(FQ_THREADS) void fewq_bwd_kernel(const float* __restrict__ u, const float* __restrict__ x, const float* __restrict__ y,
                                                              const float* __restrict__ raw, const float* __restrict__ lse,
                                                              const float* __restrict__ z, const float* __restrict__ dz,
                                                              const float* __restrict__ draw, const float* __restrict__ dlse,
                                                              float* __restrict__ dx, float* __restrict__ dy, float* __restrict__ part, const int L,
                                                              const int S, const int Ek, const int Ev, const long long xbs, const long long xrs,
                                                              const long long ybs, const long long yrs, const long long dxbs,
                                                              const long long dxrs, const long long dybs, const long long dyrs, const int rps) {
  const int b = blockIdx.y, sp = blockIdx.x, NS = gridDim.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int r0 = sp * rps, r1 = r0 + min(rps, S - r0);
  bool kc[P], vc[P];                                           // loads are unconditional, as in the forward kernel
  int ko[P], vo[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    kc[j] = j * 256 + 4 * lane < Ek; ko[j] = kc[j] ? j * 256 + 4 * lane : 0;
    vc[j] = j * 256 + 4 * lane < Ev; vo[j] = vc[j] ? j * 256 + 4 * lane : 0;
  }
  const float* xb = x + (size_t)b * xbs;
  const float* yb = SAME ? xb : y + (size_t)b * ybs;
  const long long vrs = SAME ? xrs : yrs;
  const bool want_dx = dx != nullptr, want_dy = !SAME && dy != nullptr;

  float4 ur[LQ][P], gz[LQ][P], du[LQ][P];
  float kap[LQ], dcl[LQ];
#pragma unroll
  for (int l = 0; l < LQ; ++l) {
    const int lc = min(l, L - 1);
    float d = 0.f;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const float4 uv = ld4(u + ((size_t)b * L + lc) * Ek + ko[j]);
      const float4 gv = ld4(dz + ((size_t)b * L + lc) * Ev + vo[j]);
      const float4 zv = ld4(z + ((size_t)b * L + lc) * Ev + vo[j]);
      ur[l][j] = (l < L && kc[j]) ? uv : make_float4(0.f, 0.f, 0.f, 0.f);
      gz[l][j] = (l < L && vc[j]) ? gv : make_float4(0.f, 0.f, 0.f, 0.f);
      d += dot4(gz[l][j], zv);
      du[l][j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    kap[l] = wave_sum(d) - (dlse ? dlse[(size_t)b * L + lc] : 0.f);      // d lse_l enters as ds += dlse_l p
    dcl[l] = 0.f;
  }
  // lane 4 l + i speaks for (query l, row rw + i): it reads raw and draw there and forms p
  const int li = lane & 3, lq = min(lane >> 2, L - 1);
  const bool lane_q = (lane >> 2) < L;
  const float lse_l = lse[(size_t)b * L + lq];
  const float* rawl = raw + ((size_t)b * L + lq) * S;
  const float* drawl = draw ? draw + ((size_t)b * L + lq) * S : rawl;

  for (int t0 = r0; t0 < r1; t0 += FQ_TILE) {
    const int rw = t0 + 4 * wave;
    float4 xr[4][P], yr[SAME ? 1 : 4][SAME ? 1 : P];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const size_t ri = (size_t)min(rw + i, r1 - 1);
#pragma unroll
      for (int j = 0; j < P; ++j) {
        xr[i][j] = ld4(xb + ri * xrs + ko[j]);
        if constexpr (!SAME) yr[i][j] = ld4(yb + ri * vrs + vo[j]);
      }
    }
    const int rl = min(rw + li, r1 - 1);
    const float rv = rawl[rl], dv = drawl[rl];
    const bool live = lane_q && rw + li < r1 && rv != -INFINITY;        // a masked key: p = 0 and no gradient through its score
    const float pe = live ? expf(rv - lse_l) : 0.f;
    const float de = (live && draw) ? dv : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float ds[LQ], pp[LQ];
#pragma unroll
      for (int l = 0; l < LQ; ++l) {
        ds[l] = 0.f; pp[l] = 0.f;
        if (l < L) {
          float t = 0.f;
#pragma unroll
          for (int j = 0; j < P; ++j) t += dot4(gz[l][j], SAME ? xr[i][j] : yr[SAME ? 0 : i][SAME ? 0 : j]);
          t = wave_sum(t);
          pp[l] = lane_value(pe, 4 * l + i);
          ds[l] = fmaf(pp[l], t - kap[l], lane_value(de, 4 * l + i));
          dcl[l] += ds[l];
#pragma unroll
          for (int j = 0; j < P; ++j) axpy4(du[l][j], ds[l], xr[i][j]);
        }
      }
      if (rw + i < r1 && (want_dx || want_dy)) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
          float4 gx = make_float4(0.f, 0.f, 0.f, 0.f), gy = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
          for (int l = 0; l < LQ; ++l) {
            if (l < L) {
              if (SAME || want_dx) axpy4(SAME ? gy : gx, ds[l], ur[l][j]);
              if (SAME || want_dy) axpy4(gy, pp[l], gz[l][j]);
            }
          }
          if constexpr (SAME) {
            if (kc[j]) *reinterpret_cast<float4*>(dx + (size_t)b * dxbs + (size_t)(rw + i) * dxrs + ko[j]) = gy;
          } else {
            if (want_dx && kc[j]) *reinterpret_cast<float4*>(dx + (size_t)b * dxbs + (size_t)(rw + i) * dxrs + ko[j]) = gx;
            if (want_dy && vc[j]) *reinterpret_cast<float4*>(dy + (size_t)b * dybs + (size_t)(rw + i) * dyrs + vo[j]) = gy;
          }
        }
      }
    }
  }

  // the four waves' sums, added in wave order, one query at a time
  __shared__ __attribute__((aligned(16))) float sDu[4][FQ_MAXE];
  __shared__ float sDc[4];
  const size_t prow = ((size_t)b * NS + sp) * L;
#pragma unroll
  for (int l = 0; l < LQ; ++l) {
    if (l < L) {
      __syncthreads();
#pragma unroll
      for (int j = 0; j < P; ++j)
        if (kc[j]) *reinterpret_cast<float4*>(&sDu[wave][ko[j]]) = du[l][j];
      if (lane == 0) sDc[wave] = dcl[l];
      __syncthreads();
      float* pr = part + (prow + l) * bwd_part_ld(Ek);
      for (int col = tid; col < Ek; col += FQ_THREADS) pr[col] = ((sDu[0][col] + sDu[1][col]) + sDu[2][col]) + sDu[3][col];
      if (tid == 0) pr[Ek] = ((sDc[0] + sDc[1]) + sDc[2]) + sDc[3];
    }
  }
}

// part [B, NS, L, Ek + 4] -> du [B, L, Ek], dc [B, L]: grid (L, B), the splits in ascending order, eight loads in flight
__global__ __launch_bounds__(FQ_THREADS) void fewq_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ du, float* __restrict__ dc,
                                                                     const int NS, const int L, const int Ek) {
  const int l = blockIdx.x, b = blockIdx.y;
  const int ld = bwd_part_ld(Ek);
  const float* p = part + ((size_t)b * NS * L + l) * ld;
  const size_t rs = (size_t)L * ld;
  for (int col = threadIdx.x; col <= Ek; col += FQ_THREADS) {
    float a = 0.f;
    for (int i0 = 0; i0 < NS; i0 += 8) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = i0 + k < NS ? p[(size_t)(i0 + k) * rs + col] : 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) a += v[k];
    }
    if (col < Ek) du[((size_t)b * L + l) * Ek + col] = a; else dc[(size_t)b * L + l] = a;
  }
}

bool fewq_shape_ok(int B, int L, int S, int Ek, int Ev) {
  return B > 0 && B <= 65535 && L > 0 && L <= FQ_MAXL && S > 0 && S <= (1 << 30) && Ek > 0 && Ek <= FQ_MAXE && Ek % 64 == 0 && Ev > 0 &&
         Ev <= FQ_MAXE && Ev % 64 == 0;
}

// rows per split: `splits` as asked for (tests), or - splits <= 0 - enough splits for FQ_TARGET_WG workgroups, none under FQ_MIN_ROWS rows
int fewq_rows_per_split(int B, int S, int splits) {
  if (splits > 0) return (int)(((long long)S + splits - 1) / splits);
  const int want = std::max(1, (FQ_TARGET_WG + B - 1) / B);
  return std::max((S + want - 1) / want, std::min(S, FQ_MIN_ROWS));
}
// the splits that hold a row
int fewq_splits(int S, int rps) { return (int)(((long long)S + rps - 1) / rps); }

bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }
// a [B, S, E] view with unit column stride: rows and bags a multiple of four floats apart, rows at least E apart
bool strides_ok(long long bs, long long rs, int E) { return bs >= 0 && rs >= E && bs % 4 == 0 && rs % 4 == 0; }
// x and y name the same rows
bool same_rows(const float* x, const float* y, long long xbs, long long xrs, long long ybs, long long yrs, int Ek, int Ev) {
  return x == y && xbs == ybs && xrs == yrs && Ek == Ev;
}

#define FQ_DISPATCH(KERNEL, LQ, P, SAME, ...)                                                                      \
  do {                                                                                                            \
    if (SAME) hipLaunchKernelGGL((KERNEL<LQ, P, true>), grid, dim3(FQ_THREADS), 0, (hipStream_t)stream, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<LQ, P, false>), grid, dim3(FQ_THREADS), 0, (hipStream_t)stream, __VA_ARGS__);    \
  } while (0)
#define FQ_LAUNCH(KERNEL, ...)                                                   \
  do {                                                                           \
    if (L <= 4 && wide <= 256) FQ_DISPATCH(KERNEL, 4, 1, same, __VA_ARGS__);     \
    else if (L <= 4) FQ_DISPATCH(KERNEL, 4, 2, same, __VA_ARGS__);               \
    else if (wide <= 256) FQ_DISPATCH(KERNEL, 8, 1, same, __VA_ARGS__);          \
    else FQ_DISPATCH(KERNEL, 8, 2, same, __VA_ARGS__);                           \
  } while (0)

}  // namespace

extern "C" {

size_t smml_fewq_attn_fwd_workspace_bytes(int B, int L, int S, int Ev, int splits) {
  if (B <= 0 || L <= 0 || S <= 0 || Ev <= 0) return 0;
  const size_t NS = (size_t)fewq_splits(S, fewq_rows_per_split(B, S, splits));
  return (size_t)B * NS * (size_t)L * ((size_t)Ev + 4) * sizeof(float);     // acc [B, NS, L, Ev], then (m, l) [B, NS, L, 2] (padded to 4)
}

int smml_fewq_attn_fwd_f32(const float* u, const float* c, const float* x, const float* y, const unsigned char* key_padding_mask, float* z,
                           float* raw, float* lse, void* workspace, size_t workspace_bytes, int B, int L, int S, int Ek, int Ev,
                           long long x_batch_stride, long long x_row_stride, long long y_batch_stride, long long y_row_stride, int splits,
                           void* stream) {
  const char* fn = "smml_fewq_attn_fwd_f32";
  SMML_REQUIRE(u && c && x && y && z && raw && lse && workspace, "%s: null pointer", fn);
  SMML_REQUIRE(fewq_shape_ok(B, L, S, Ek, Ev), "%s: need L <= %d queries, Ek and Ev multiples of 64 up to %d, S >= 1, B <= 65535 "
               "(got B %d, L %d, S %d, Ek %d, Ev %d)", fn, FQ_MAXL, FQ_MAXE, B, L, S, Ek, Ev);
  SMML_REQUIRE(strides_ok(x_batch_stride, x_row_stride, Ek) && strides_ok(y_batch_stride, y_row_stride, Ev),
               "%s: row and batch strides must be multiples of 4 floats, rows at least their width apart", fn);
  SMML_REQUIRE(aligned16(u) && aligned16(x) && aligned16(y) && aligned16(workspace), "%s: u, x, y and workspace must be 16-byte aligned", fn);
  SMML_REQUIRE(workspace_bytes >= smml_fewq_attn_fwd_workspace_bytes(B, L, S, Ev, splits), "%s: workspace too small", fn);
  const int rps = fewq_rows_per_split(B, S, splits), NS = fewq_splits(S, rps), wide = std::max(Ek, Ev);
  const bool same = same_rows(x, y, x_batch_stride, x_row_stride, y_batch_stride, y_row_stride, Ek, Ev);
  float* pacc = (float*)workspace;
  float* pml = pacc + (size_t)B * NS * L * Ev;
  const dim3 grid((unsigned)NS, (unsigned)B);
  FQ_LAUNCH(fewq_fwd_kernel, u, c, x, y, key_padding_mask, raw, pacc, pml, L, S, Ek, Ev, x_batch_stride, x_row_stride, y_batch_stride,
            y_row_stride, rps);
  SMML_LAUNCH_CHECK(fn);
  hipLaunchKernelGGL(fewq_merge_kernel, dim3((unsigned)L, (unsigned)B), dim3(FQ_THREADS), 0, (hipStream_t)stream, pacc, pml, z, lse, NS, L, Ev);
  SMML_LAUNCH_CHECK(fn);
  return SMML_OK;
}

size_t smml_fewq_attn_bwd_workspace_bytes(int B, int L, int S, int Ek, int splits) {
  if (B <= 0 || L <= 0 || S <= 0 || Ek <= 0) return 0;
  const size_t NS = (size_t)fewq_splits(S, fewq_rows_per_split(B, S, splits));
  return (size_t)B * NS * (size_t)L * (size_t)bwd_part_ld(Ek) * sizeof(float);     // part [B, NS, L, Ek + 4]
}

int smml_fewq_attn_bwd_f32(const float* u, const float* x, const float* y, const float* raw, const float* lse, const float* z, const float* dz,
                           const float* draw, const float* dlse, float* du, float* dc, float* dx, float* dy, void* workspace,
                           size_t workspace_bytes, int B, int L, int S, int Ek, int Ev, long long x_batch_stride, long long x_row_stride,
                           long long y_batch_stride, long long y_row_stride, long long dx_batch_stride, long long dx_row_stride,
                           long long dy_batch_stride, long long dy_row_stride, int splits, void* stream) {
  const char* fn = "smml_fewq_attn_bwd_f32";
  SMML_REQUIRE(u && x && y && raw && lse && z && dz && du && dc && workspace, "%s: null pointer", fn);
  SMML_REQUIRE(fewq_shape_ok(B, L, S, Ek, Ev), "%s: need L <= %d queries, Ek and Ev multiples of 64 up to %d, S >= 1, B <= 65535 "
               "(got B %d, L %d, S %d, Ek %d, Ev %d)", fn, FQ_MAXL, FQ_MAXE, B, L, S, Ek, Ev);
  SMML_REQUIRE(strides_ok(x_batch_stride, x_row_stride, Ek) && strides_ok(y_batch_stride, y_row_stride, Ev) &&
               (!dx || strides_ok(dx_batch_stride, dx_row_stride, Ek)) && (!dy || strides_ok(dy_batch_stride, dy_row_stride, Ev)),
               "%s: row and batch strides must be multiples of 4 floats, rows at least their width apart", fn);
  SMML_REQUIRE(aligned16(u) && aligned16(x) && aligned16(y) && aligned16(z) && aligned16(dz) && aligned16(dx) && aligned16(dy) &&
               aligned16(workspace), "%s: u, x, y, z, dz, dx, dy and workspace must be 16-byte aligned", fn);
  SMML_REQUIRE(workspace_bytes >= smml_fewq_attn_bwd_workspace_bytes(B, L, S, Ek, splits), "%s: workspace too small", fn);
  const bool same = same_rows(x, y, x_batch_stride, x_row_stride, y_batch_stride, y_row_stride, Ek, Ev);
  SMML_REQUIRE(!same || !dy, "%s: x and y are the same rows: their one gradient row dx + dy goes to dx, dy must be null", fn);
  const int rps = fewq_rows_per_split(B, S, splits), NS = fewq_splits(S, rps), wide = std::max(Ek, Ev);
  float* part = (float*)workspace;
  const dim3 grid((unsigned)NS, (unsigned)B);
  FQ_LAUNCH(fewq_bwd_kernel, u, x, y, raw, lse, z, dz, draw, dlse, dx, dy, part, L, S, Ek, Ev, x_batch_stride, x_row_stride, y_batch_stride,
            y_row_stride, dx_batch_stride, dx_row_stride, dy_batch_stride, dy_row_stride, rps);
  SMML_LAUNCH_CHECK(fn);
  hipLaunchKernelGGL(fewq_bwd_reduce_kernel, dim3((unsigned)L, (unsigned)B), dim3(FQ_THREADS), 0, (hipStream_t)stream, part, du, dc, NS, L, Ek);
  SMML_LAUNCH_CHECK(fn);
  return SMML_OK;
}

}  // extern "C"
