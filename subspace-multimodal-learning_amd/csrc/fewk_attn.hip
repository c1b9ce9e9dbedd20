// Few-key co-attention (models/MultiheadAttention.py with one head and a bag of L queries over S <= 8 keys: CMTA's P_in_G_Att), the dual of
// fewq_attn.hip: with k^ = Wk key + bk and v^ = Wv value + bv the projections fold onto the KEYS,
//     raw[b, l, j] = x[b, l] . u[b, j] + c[b, j]        out[b, l] = sum_j softmax_j(raw[b, l, :]) w[b, j]
// for u = s k^ Wq, c = s k^ . bq, w = v^ Wo^T + bo (formed outside, [B S, E]-sized GEMMs): the query and out projections never touch the bag,
// every row of x is read once and every row of out written once.
//
//   forward   grid (splits, B), 256 threads.  u, c and w of the bag live in LDS for the life of the workgroup, which walks its rows in tiles
//             of 16: a row belongs to ONE 16-lane DPP row of a wave (four rows per wave), a lane holds float4 x Eq/64 of it.  The S dot
//             products close with four DPP steps inside the 16 lanes (quad_perm, quad_perm, row_half_mirror, row_mirror: an all-reduce
//             whose result is the same bits in every lane), the softmax over S numbers is formed by every lane, the output row is
//             sum_j p_j w_j with w read from LDS (the four rows of a wave read the same addresses: a broadcast).  No sum crosses rows.
//   backward  the same grid and row ownership, one pass: p recomputed from raw, dp_j = dout . w_j, g_j = p_j (dp_j - sum p dp) + draw_j,
//             dx = sum_j g_j u_j written once; du_j += g_j x, dc_j += g_j, dw_j += p_j dout accumulate in registers per lane, meet in LDS at
//             the end of the split - the 16 (wave, DPP row) owners added in ascending order - and go to ONE partial per split; a second
//             kernel adds a bag's partials in ascending split order.  S x (Eq + Eo) / 64 float4 accumulators per lane: past 32 of them the
//             pass is launched twice, once for dx / du / dc and once for dw (which needs raw and dout alone).
// A masked key scores -inf, weighs exp(-inf - m) = 0 and receives no gradient; a row whose keys are ALL masked is NaN here as in the reference.
// Every sum has one owner and a fixed order: no float atomics, the results are a function of the inputs and the split count alone.
// Several heads would fold as h S virtual keys with a softmax per group of S; the kernels are one-head.
#include "smml_common.h"

#include <algorithm>
#include <math.h>

namespace {

constexpr int FK_THREADS = 256;
constexpr int FK_TILE = 16;          // rows per tile: one per 16-lane DPP row, four per wave
constexpr int FK_OWNERS = 16;        // (wave, DPP row) pairs of a workgroup: the owners of the backward's per-lane sums
constexpr int FK_MAXS = 8;
constexpr int FK_MAXE = 512;
constexpr int FK_MIN_ROWS = 64;      // rows per split the heuristic does not go below (the S (Eq + Eo) reload of u and w stays a few per cent)
constexpr int FK_TARGET_WG = 1024;   // workgroups the heuristic aims at: 256 CUs x 4 resident

template <int CTRL>
__device__ __forceinline__ float dpp_move(float v) {
  return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), CTRL, 0xf, 0xf, false));
}
// sum over the 16 lanes of a DPP row, the same bits in each of them: xor 1 and xor 2 inside the quads, then the mirrored half row and the
// mirrored row (after each step the partner holds the sum this lane lacks, and a + b is b + a)
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_move<0xB1>(v);            // quad_perm [1, 0, 3, 2]
  v += dpp_move<0x4E>(v);            // quad_perm [2, 3, 0, 1]
  v += dpp_move<0x141>(v);           // row_half_mirror
  v += dpp_move<0x140>(v);           // row_mirror
  return v;
}
__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); }
__device__ __forceinline__ void axpy4(float4& a, const float s, const float4 v) {
  a.x = fmaf(s, v.x, a.x); a.y = fmaf(s, v.y, a.y); a.z = fmaf(s, v.z, a.z); a.w = fmaf(s, v.w, a.w);
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, const float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// rows [S, E] of a bag -> LDS rows of P * 64 floats
template <int P>
__device__ __forceinline__ void stage_rows(float (*dst)[P * 64], const float* __restrict__ src, const int S, const int E) {
  const int e4 = E >> 2;
  for (int i = threadIdx.x; i < S * e4; i += FK_THREADS) {
    const int j = i / e4, q = i - j * e4;
    st4(&dst[j][4 * q], ld4(src + (size_t)j * E + 4 * q));
  }
}

// x [B, L, Eq] (strides xbs, xrs), u [B, S, Eq], c [B, S], w [B, S, Eo], mask [B, S] bytes or null -> out [B, L, Eo], raw [B, L, S];
// split sp of bag b owns rows [sp rps, min(L, (sp + 1) rps)).  SK: the keys the registers are laid out for (j >= S: skipped);
// P: 64-column chunks of max(Eq, Eo) (chunks past a width: skipped - a width is a multiple of 64, so a chunk is whole or absent)
template <int SK, int P>
__global__ __launch_bounds__(FK_THREADS) void fewk_fwd_kernel(const float* __restrict__ x, const float* __restrict__ u, const float* __restrict__ c,
                                                              const float* __restrict__ w, const unsigned char* __restrict__ mask,
                                                              float* __restrict__ out, float* __restrict__ raw, const int L, const int S,
                                                              const int Eq, const int Eo, const long long xbs, const long long xrs,
                                                              const int rps) {
  const int b = blockIdx.y, sp = blockIdx.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane & 15, rg = lane >> 4;
  const int r0 = sp * rps, r1 = r0 + min(rps, L - r0);
  const int nq = Eq >> 6, no = Eo >> 6;
  __shared__ __attribute__((aligned(16))) float sU[SK][P * 64];
  __shared__ __attribute__((aligned(16))) float sW[SK][P * 64];
  stage_rows<P>(sU, u + (size_t)b * S * Eq, S, Eq);
  stage_rows<P>(sW, w + (size_t)b * S * Eo, S, Eo);
  float cj[SK];
  bool live[SK];                                               // the key exists and is not masked
#pragma unroll
  for (int j = 0; j < SK; ++j) {
    const int jc = min(j, S - 1);
    cj[j] = c[(size_t)b * S + jc];
    live[j] = j < S && !(mask && mask[(size_t)b * S + jc]);
  }
  __syncthreads();
  const float* xb = x + (size_t)b * xbs;

  for (int t0 = r0; t0 < r1; t0 += FK_TILE) {
    // every lane stays active (the DPP steps read their neighbours): a row past the split's end re-reads the last row and stores nothing
    const int row = t0 + 4 * wave + rg;
    const bool ok = row < r1;
    const size_t rc = (size_t)min(row, r1 - 1);
    float4 xr[P];
#pragma unroll
    for (int k = 0; k < P; ++k)
      if (k < nq) xr[k] = ld4(xb + rc * xrs + 64 * k + 4 * g);
    float s[SK], sv = 0.f, m = -INFINITY;
#pragma unroll
    for (int j = 0; j < SK; ++j) {
      s[j] = -INFINITY;
      if (j < S) {
        float d = 0.f;
#pragma unroll
        for (int k = 0; k < P; ++k)
          if (k < nq) d += dot4(xr[k], ld4(&sU[j][64 * k + 4 * g]));
        d = row16_sum(d) + cj[j];
        s[j] = live[j] ? d : -INFINITY;
        sv = g == j ? s[j] : sv;
        m = fmaxf(m, s[j]);
      }
    }
    float p[SK], sum = 0.f;
#pragma unroll
    for (int j = 0; j < SK; ++j) {
      p[j] = expf(s[j] - m);                                   // every key masked: -inf - -inf, NaN as in the reference
      sum += p[j];
    }
    const float inv = 1.f / sum;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      if (k < no) {
        float4 a = zero4();
#pragma unroll
        for (int j = 0; j < SK; ++j)
          if (j < S) axpy4(a, p[j] * inv, ld4(&sW[j][64 * k + 4 * g]));
        if (ok) st4(out + ((size_t)b * L + rc) * Eo + 64 * k + 4 * g, a);
      }
    }
    if (ok && g < S) raw[((size_t)b * L + rc) * S + g] = sv;
  }
}

// row stride of the backward partials: du in columns [0, Eq), dw in [Eq, Eq + Eo), dc in column Eq + Eo
__host__ __device__ constexpr int bwd_part_ld(int Eq, int Eo) { return Eq + Eo + 4; }

// the 16 owners' vectors of one key, added in ascending owner order -> dst[0 .. E)
template <int P>
__device__ __forceinline__ void merge_owners(float (*sAcc)[P * 64], const float4 (&acc)[P], const int chunks, const int slot, const int g,
                                             float* __restrict__ dst, const int E) {
  __syncthreads();                                             // the previous vector has been read
#pragma unroll
  for (int k = 0; k < P; ++k)
    if (k < chunks) st4(&sAcc[slot][64 * k + 4 * g], acc[k]);
  __syncthreads();
  for (int col = threadIdx.x; col < E; col += FK_THREADS) {
    float a = sAcc[0][col];
#pragma unroll
    for (int o = 1; o < FK_OWNERS; ++o) a += sAcc[o][col];
    dst[col] = a;
  }
}

// saved raw and dout (draw: optional) -> dx (may be null: nothing is formed for it) and part [B, NS, S, Eq + Eo + 4].  DU: this launch forms
// dx, du and dc; DW: it forms dw.  dout and dx carry strides of their own.
template <int SK, int P, bool DU, bool DW>
__global__ __launch_bounds__(FK_THREADS) void fewk_bwd_kernel(const float* __restrict__ x, const float* __restrict__ u, const float* __restrict__ w,
                                                              const float* __restrict__ raw, const float* __restrict__ dout,
                                                              const float* __restrict__ draw, float* __restrict__ dx, float* __restrict__ part,
                                                              const int L, const int S, const int Eq, const int Eo, const long long xbs,
                                                              const long long xrs, const long long gbs, const long long grs,
                                                              const long long dxbs, const long long dxrs, const int rps) {
  const int b = blockIdx.y, sp = blockIdx.x, NS = gridDim.x;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane & 15, rg = lane >> 4;
  const int r0 = sp * rps, r1 = r0 + min(rps, L - r0);
  const int nq = Eq >> 6, no = Eo >> 6;
  // u and w while the rows stream, the owners' vectors afterwards: one buffer (merge_owners opens with a barrier)
  constexpr int UW = DU ? 2 * SK : 0;
  __shared__ __attribute__((aligned(16))) float sBuf[UW > FK_OWNERS ? UW : FK_OWNERS][P * 64];
  __shared__ float sDc[SK][FK_OWNERS];
  float (*sU)[P * 64] = sBuf;
  float (*sW)[P * 64] = sBuf + (DU ? SK : 0);
  float (*sAcc)[P * 64] = sBuf;
  if constexpr (DU) {
    stage_rows<P>(sU, u + (size_t)b * S * Eq, S, Eq);
    stage_rows<P>(sW, w + (size_t)b * S * Eo, S, Eo);
    __syncthreads();
  }
  const float* xb = x + (size_t)b * xbs;
  const float* gb = dout + (size_t)b * gbs;
  const bool want_dx = DU && dx != nullptr;

  float4 du[DU ? SK : 1][P], dw[DW ? SK : 1][P];
  float dcl[SK];
#pragma unroll
  for (int j = 0; j < SK; ++j) {
    dcl[j] = 0.f;
#pragma unroll
    for (int k = 0; k < P; ++k) {
      if constexpr (DU) du[j][k] = zero4();
      if constexpr (DW) dw[j][k] = zero4();
    }
  }

  // the operands of one tile: this lane's chunks of its row of x and dout, the row's S scores and their gradients.  A row past the split's
  // end re-reads the last row (every lane stays active, as in the forward kernel) and weighs 0
  auto load_tile = [&](const int t0, float4 (&xr)[DU ? P : 1], float4 (&gr)[P], float (&s)[SK], float (&de)[SK]) {
    const size_t rc = (size_t)min(t0 + 4 * wave + rg, r1 - 1);
#pragma unroll
    for (int k = 0; k < P; ++k) {
      if constexpr (DU)
        if (k < nq) xr[k] = ld4(xb + rc * xrs + 64 * k + 4 * g);
      if (k < no) gr[k] = ld4(gb + rc * grs + 64 * k + 4 * g);
    }
    const float* rr = raw + ((size_t)b * L + rc) * S;
    const float* dr = draw ? draw + ((size_t)b * L + rc) * S : rr;
#pragma unroll
    for (int j = 0; j < SK; ++j) {
      s[j] = -INFINITY; de[j] = 0.f;
      if (j < S) {
        s[j] = rr[j];
        if constexpr (DU) de[j] = draw ? dr[j] : 0.f;
      }
    }
  };
  // where the registers allow it the next tile's loads are issued before this tile's arithmetic (two waves per SIMD hide little)
  constexpr bool PRE = SK * P <= 16;
  float4 xr[DU ? P : 1], gr[P], xn[DU ? P : 1], gn[P];
  float s[SK], de[SK], sn[SK], dn[SK];
  if constexpr (PRE) load_tile(r0, xr, gr, s, de);

  for (int t0 = r0; t0 < r1; t0 += FK_TILE) {
    const int row = t0 + 4 * wave + rg;
    const bool ok = row < r1;
    const size_t rc = (size_t)min(row, r1 - 1);
    if constexpr (PRE) load_tile(t0 + FK_TILE, xn, gn, sn, dn);
    else load_tile(t0, xr, gr, s, de);
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < SK; ++j) {
      if (s[j] == -INFINITY) de[j] = 0.f;                      // no gradient through a masked key's score
      m = fmaxf(m, s[j]);
    }
    float p[SK], sum = 0.f;
#pragma unroll
    for (int j = 0; j < SK; ++j) {
      p[j] = expf(s[j] - m);
      sum += p[j];
    }
    const float inv = ok ? 1.f / sum : 0.f;
#pragma unroll
    for (int j = 0; j < SK; ++j) p[j] *= inv;
    if constexpr (DW) {
#pragma unroll
      for (int j = 0; j < SK; ++j)
        if (j < S) {
#pragma unroll
          for (int k = 0; k < P; ++k)
            if (k < no) axpy4(dw[j][k], p[j], gr[k]);
        }
    }
    if constexpr (DU) {
      float gs[SK], kap = 0.f;
#pragma unroll
      for (int j = 0; j < SK; ++j) {
        gs[j] = 0.f;
        if (j < S) {
          float d = 0.f;
#pragma unroll
          for (int k = 0; k < P; ++k)
            if (k < no) d += dot4(gr[k], ld4(&sW[j][64 * k + 4 * g]));
          gs[j] = row16_sum(d);
          kap = fmaf(p[j], gs[j], kap);
        }
      }
#pragma unroll
      for (int j = 0; j < SK; ++j) {
        if (j < S) {
          gs[j] = ok ? fmaf(p[j], gs[j] - kap, de[j]) : 0.f;
          dcl[j] += gs[j];
#pragma unroll
          for (int k = 0; k < P; ++k)
            if (k < nq) axpy4(du[j][k], gs[j], xr[k]);
        }
      }
      if (want_dx) {
#pragma unroll
        for (int k = 0; k < P; ++k) {
          if (k < nq) {
            float4 a = zero4();
#pragma unroll
            for (int j = 0; j < SK; ++j)
              if (j < S) axpy4(a, gs[j], ld4(&sU[j][64 * k + 4 * g]));
            if (ok) st4(dx + (size_t)b * dxbs + rc * dxrs + 64 * k + 4 * g, a);
          }
        }
      }
    }
    if constexpr (PRE) {
#pragma unroll
      for (int k = 0; k < P; ++k) {
        if constexpr (DU)
          if (k < nq) xr[k] = xn[k];
        if (k < no) gr[k] = gn[k];
      }
#pragma unroll
      for (int j = 0; j < SK; ++j) { s[j] = sn[j]; de[j] = dn[j]; }
    }
  }

  const int slot = 4 * wave + rg;
  const size_t prow = ((size_t)b * NS + sp) * S;
  const int ld = bwd_part_ld(Eq, Eo);
#pragma unroll
  for (int j = 0; j < SK; ++j) {
    if (j < S) {
      float* pr = part + (prow + j) * ld;
      if constexpr (DU) {
        if (g == 0) sDc[j][slot] = dcl[j];                     // a row of its own per key: read after merge_owners' barriers
        merge_owners<P>(sAcc, du[j], nq, slot, g, pr, Eq);
        if (tid == 0) {
          float a = sDc[j][0];
#pragma unroll
          for (int o = 1; o < FK_OWNERS; ++o) a += sDc[j][o];
          pr[Eq + Eo] = a;
        }
      }
      if constexpr (DW) merge_owners<P>(sAcc, dw[j], no, slot, g, pr + Eq, Eo);
    }
  }
}

// part [B, NS, S, Eq + Eo + 4] -> du [B, S, Eq], dw [B, S, Eo], dc [B, S]: grid (S, B), the splits in ascending order, eight loads in flight
__global__ __launch_bounds__(FK_THREADS) void fewk_bwd_reduce_kernel(const float* __restrict__ part, float* __restrict__ du, float* __restrict__ dc,
                                                                     float* __restrict__ dw, const int NS, const int S, const int Eq,
                                                                     const int Eo) {
  const int j = blockIdx.x, b = blockIdx.y;
  const int ld = bwd_part_ld(Eq, Eo);
  const float* p = part + ((size_t)b * NS * S + j) * ld;
  const size_t rs = (size_t)S * ld;
  for (int col = threadIdx.x; col <= Eq + Eo; col += FK_THREADS) {
    float a = 0.f;
    for (int i0 = 0; i0 < NS; i0 += 8) {
      float v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = i0 + k < NS ? p[(size_t)(i0 + k) * rs + col] : 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) a += v[k];
    }
    if (col < Eq) du[((size_t)b * S + j) * Eq + col] = a;
    else if (col < Eq + Eo) dw[((size_t)b * S + j) * Eo + col - Eq] = a;
    else dc[(size_t)b * S + j] = a;
  }
}

bool fewk_shape_ok(int B, int L, int S, int Eq, int Eo) {
  return B > 0 && B <= 65535 && S > 0 && S <= FK_MAXS && L > 0 && L <= (1 << 30) && Eq > 0 && Eq <= FK_MAXE && Eq % 64 == 0 && Eo > 0 &&
         Eo <= FK_MAXE && Eo % 64 == 0;
}

// rows per split: `splits` as asked for (tests), or - splits <= 0 - enough splits for FK_TARGET_WG workgroups, none under FK_MIN_ROWS rows,
// whole tiles
int fewk_rows_per_split(int B, int L, int splits) {
  if (splits > 0) return (int)(((long long)L + splits - 1) / splits);
  const int want = std::max(1, (FK_TARGET_WG + B - 1) / B);
  const int rps = std::max((L + want - 1) / want, std::min(L, FK_MIN_ROWS));
  return (rps + FK_TILE - 1) / FK_TILE * FK_TILE;
}
// the splits that hold a row
int fewk_splits(int L, int rps) { return (int)(((long long)L + rps - 1) / rps); }

bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }
// a [B, L, E] view with unit column stride: rows and bags a multiple of four floats apart, rows at least E apart
bool strides_ok(long long bs, long long rs, int E) { return bs >= 0 && rs >= E && bs % 4 == 0 && rs % 4 == 0; }

// accumulators per lane past which the backward pass is launched once per half of its sums (float4 each: 128 VGPRs at the limit)
constexpr int FK_MAX_ACC = 32;

// one launch while the accumulators fit, else one for dx / du / dc and one for dw
template <int SK, int P, typename... Args>
void fewk_bwd_launch(const dim3 grid, hipStream_t stream, Args... args) {
  if constexpr (2 * SK * P <= FK_MAX_ACC) {
    hipLaunchKernelGGL((fewk_bwd_kernel<SK, P, true, true>), grid, dim3(FK_THREADS), 0, stream, args...);
  } else {
    hipLaunchKernelGGL((fewk_bwd_kernel<SK, P, true, false>), grid, dim3(FK_THREADS), 0, stream, args...);
    hipLaunchKernelGGL((fewk_bwd_kernel<SK, P, false, true>), grid, dim3(FK_THREADS), 0, stream, args...);
  }
}

#define FK_DISPATCH(LAUNCH)                                   \
  do {                                                        \
    if (S <= 4 && wide <= 256) LAUNCH(4, 4);                  \
    else if (S <= 4) LAUNCH(4, 8);                            \
    else if (wide <= 256) LAUNCH(8, 4);                       \
    else LAUNCH(8, 8);                                        \
  } while (0)

}  // namespace

extern "C" {

size_t smml_fewk_attn_fwd_workspace_bytes(int B, int L, int S, int Eo, int splits) {
  (void)B; (void)L; (void)S; (void)Eo; (void)splits;
  return 0;                                                    // no sum crosses rows in the forward: nothing to park
}

int smml_fewk_attn_fwd_f32(const float* x, const float* u, const float* c, const float* w, const unsigned char* key_padding_mask, float* out,
                           float* raw, void* workspace, size_t workspace_bytes, int B, int L, int S, int Eq, int Eo, long long x_batch_stride,
                           long long x_row_stride, int splits, void* stream) {
  const char* fn = "smml_fewk_attn_fwd_f32";
  (void)workspace; (void)workspace_bytes;
  SMML_REQUIRE(x && u && c && w && out && raw, "%s: null pointer", fn);
  SMML_REQUIRE(fewk_shape_ok(B, L, S, Eq, Eo), "%s: need 1 <= S <= %d keys, Eq and Eo multiples of 64 up to %d, L >= 1, B <= 65535 "
               "(got B %d, L %d, S %d, Eq %d, Eo %d)", fn, FK_MAXS, FK_MAXE, B, L, S, Eq, Eo);
  SMML_REQUIRE(strides_ok(x_batch_stride, x_row_stride, Eq), "%s: row and batch strides must be multiples of 4 floats, rows at least their "
               "width apart", fn);
  SMML_REQUIRE(aligned16(x) && aligned16(u) && aligned16(w) && aligned16(out), "%s: x, u, w and out must be 16-byte aligned", fn);
  const int rps = fewk_rows_per_split(B, L, splits), NS = fewk_splits(L, rps), wide = std::max(Eq, Eo);
  const dim3 grid((unsigned)NS, (unsigned)B);
#define FK_FWD(SK, P)                                                                                                                  \
  hipLaunchKernelGGL((fewk_fwd_kernel<SK, P>), grid, dim3(FK_THREADS), 0, (hipStream_t)stream, x, u, c, w, key_padding_mask, out, raw, L, S, \
                     Eq, Eo, x_batch_stride, x_row_stride, rps)
  FK_DISPATCH(FK_FWD);
#undef FK_FWD
  SMML_LAUNCH_CHECK(fn);
  return SMML_OK;
}

size_t smml_fewk_attn_bwd_workspace_bytes(int B, int L, int S, int Eq, int Eo, int splits) {
  if (B <= 0 || L <= 0 || S <= 0 || Eq <= 0 || Eo <= 0) return 0;
  const size_t NS = (size_t)fewk_splits(L, fewk_rows_per_split(B, L, splits));
  return (size_t)B * NS * (size_t)S * (size_t)bwd_part_ld(Eq, Eo) * sizeof(float);     // part [B, NS, S, Eq + Eo + 4]
}

int smml_fewk_attn_bwd_f32(const float* x, const float* u, const float* w, const float* raw, const float* dout, const float* draw, float* dx,
                           float* du, float* dc, float* dw, void* workspace, size_t workspace_bytes, int B, int L, int S, int Eq, int Eo,
                           long long x_batch_stride, long long x_row_stride, long long dout_batch_stride, long long dout_row_stride,
                           long long dx_batch_stride, long long dx_row_stride, int splits, void* stream) {
  const char* fn = "smml_fewk_attn_bwd_f32";
  SMML_REQUIRE(x && u && w && raw && dout && du && dc && dw && workspace, "%s: null pointer", fn);
  SMML_REQUIRE(fewk_shape_ok(B, L, S, Eq, Eo), "%s: need 1 <= S <= %d keys, Eq and Eo multiples of 64 up to %d, L >= 1, B <= 65535 "
               "(got B %d, L %d, S %d, Eq %d, Eo %d)", fn, FK_MAXS, FK_MAXE, B, L, S, Eq, Eo);
  SMML_REQUIRE(strides_ok(x_batch_stride, x_row_stride, Eq) && strides_ok(dout_batch_stride, dout_row_stride, Eo) &&
               (!dx || strides_ok(dx_batch_stride, dx_row_stride, Eq)),
               "%s: row and batch strides must be multiples of 4 floats, rows at least their width apart", fn);
  SMML_REQUIRE(aligned16(x) && aligned16(u) && aligned16(w) && aligned16(dout) && aligned16(dx) && aligned16(workspace),
               "%s: x, u, w, dout, dx and workspace must be 16-byte aligned", fn);
  SMML_REQUIRE(workspace_bytes >= smml_fewk_attn_bwd_workspace_bytes(B, L, S, Eq, Eo, splits), "%s: workspace too small", fn);
  const int rps = fewk_rows_per_split(B, L, splits), NS = fewk_splits(L, rps), wide = std::max(Eq, Eo);
  float* part = (float*)workspace;
  const dim3 grid((unsigned)NS, (unsigned)B);
#define FK_BWD(SK, P)                                                                                                                \
  fewk_bwd_launch<SK, P>(grid, (hipStream_t)stream, x, u, w, raw, dout, draw, dx, part, L, S, Eq, Eo, x_batch_stride, x_row_stride,    \
                         dout_batch_stride, dout_row_stride, dx_batch_stride, dx_row_stride, rps)
  FK_DISPATCH(FK_BWD);
#undef FK_BWD
  SMML_LAUNCH_CHECK(fn);
  hipLaunchKernelGGL(fewk_bwd_reduce_kernel, dim3((unsigned)S, (unsigned)B), dim3(FK_THREADS), 0, (hipStream_t)stream, part, du, dc, dw, NS, S, Eq,
                     Eo);
  SMML_LAUNCH_CHECK(fn);
  return SMML_OK;
}

}  // extern "C"
