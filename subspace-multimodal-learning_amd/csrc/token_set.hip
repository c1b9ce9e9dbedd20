// Kernels for SETS OF AT MOST 8 TOKENS (MCAT_Surv after its co-attention, models/model.py:589-651: two 2-layer nn.TransformerEncoder with 8 heads
// over the 4 genomic tokens, each followed by Attn_Net_Gated + softmax + bmm).  A token set is a few KB: what the composed forms spend is
// launches (three projections, two permute copies, two batched products and a softmax for a 4 x 4 score matrix), not bandwidth, so each
// direction of each operation is ONE launch here.
//
//   token self-attention   grid (B, H), one wave per (sample, head).  The head's Q, K, V rows (and dO in the backward) go to LDS with an odd row
//             stride (the T rows of an operand sit on distinct banks); lane 8 i + j owns score (i, j): a dot over hd, the row's max / sum and
//             the backward's rowsum(dP P) over its 8 lanes with xor shuffles.  P keep and scale dS are parked in LDS [8][9]; the lanes then
//             walk the T hd output elements, one fmaf chain of length T each.
//   gated pooling          forward: grid B, 4 waves; every wave forms the T scores of its sample (one float4 of hv, hu and w per lane, T wave sums)
//             and the softmax over them, the first E / 4 threads each own one float4 of M.  backward: grid B + 1.  Workgroup b < B owns sample b:
//             every wave forms tau_t = dM . x_t and ds_t, wave w writes the dx and dh2 rows of tokens w and w + 4.  Workgroup B owns dw and db:
//             it re-forms ds of EVERY sample (wave w: samples w, w + 4, ... in ascending order), each lane adds its four columns of
//             ds hv hu into registers, and the four waves' sums are added in wave order - one owner per element, a fixed order, no hand-off
//             between workgroups and nothing to zero.
// No float atomics anywhere: the results are a function of the inputs alone.
#include "smml_common.h"

#include <math.h>

namespace {

constexpr int TS_MAXT = 8;
constexpr int TS_MAXE = 512;
constexpr int TS_MAXD = 256;
constexpr int TS_LD = 65;            // LDS row stride of a head's rows (hd <= 64): odd, so rows t and t' never share a bank at one column
constexpr int TS_PLD = 9;            // row stride of the two 8 x 8 score-sized tiles
constexpr int TS_POOL_THREADS = 256;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float dot4(const float4 a, const float4 b) { return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w))); }
__device__ __forceinline__ double dot4_f64(const float4 a, const float4 b) {
  return fma((double)a.x, (double)b.x, fma((double)a.y, (double)b.y, fma((double)a.z, (double)b.z, (double)a.w * (double)b.w)));
}
// sum over the 64 lanes in fp64, the same value in every lane (a butterfly: every lane adds the same pairs)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ void put4(float* d, const float4 v) { d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }
// over the 8 lanes 8 i .. 8 i + 7 that hold row i of the score tile
__device__ __forceinline__ float row8_sum(float v) { v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); return v + __shfl_xor(v, 4); }
__device__ __forceinline__ float row8_max(float v) { v = fmaxf(v, __shfl_xor(v, 1)); v = fmaxf(v, __shfl_xor(v, 2)); return fmaxf(v, __shfl_xor(v, 4)); }

// qkv rows [q | k | v] of width 3 E at qkv + b qbs + t qts; keep [B, H, T, T] or null -> o rows of width E at o + b obs + t ots, p [B, H, T, T]
__global__ __launch_bounds__(64) void token_attn_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ keep, float* __restrict__ o,
                                                            float* __restrict__ p, const int T, const int E, const int hd, const long long qbs,
                                                            const long long qts, const long long obs, const long long ots, const float scale) {
  const int b = blockIdx.x, h = blockIdx.y, H = gridDim.y, lane = threadIdx.x;
  __shared__ float sQ[TS_MAXT * TS_LD], sK[TS_MAXT * TS_LD], sV[TS_MAXT * TS_LD], sP[TS_MAXT * TS_PLD];
  const float* base = qkv + (size_t)b * qbs + h * hd;
  const int hv = hd >> 2;
  for (int idx = lane; idx < T * hv; idx += 64) {
    const int t = idx / hv, c = (idx - t * hv) * 4;
    const float* r = base + (size_t)t * qts + c;
    put4(&sQ[t * TS_LD + c], ld4(r));
    put4(&sK[t * TS_LD + c], ld4(r + E));
    put4(&sV[t * TS_LD + c], ld4(r + 2 * E));
  }
  __syncthreads();
  const int i = lane >> 3, j = lane & 7;
  const bool live = i < T && j < T;
  const float* qi = &sQ[min(i, T - 1) * TS_LD];
  const float* kj = &sK[min(j, T - 1) * TS_LD];
  float s = 0.f;
  for (int d = 0; d < hd; ++d) s = fmaf(qi[d], kj[d], s);
  s = live ? s * scale : -INFINITY;
  const float m = row8_max(s);                                 // a row past T holds -inf alone: its lanes are not live and form no exponential
  const float e = live ? expf(s - m) : 0.f;
  const float l = row8_sum(e);
  const size_t pij = (((size_t)b * H + h) * T + min(i, T - 1)) * T + min(j, T - 1);
  const float pv = live ? e / l : 0.f;
  const float kp = (live && keep) ? keep[pij] : 1.f;
  if (live) p[pij] = pv;
  sP[i * TS_PLD + j] = pv * kp;
  __syncthreads();
  float* ob = o + (size_t)b * obs + h * hd;
  for (int idx = lane; idx < T * hd; idx += 64) {
    const int t = idx / hd, d = idx - t * hd;
    float acc = 0.f;
    for (int jj = 0; jj < T; ++jj) acc = fmaf(sP[t * TS_PLD + jj], sV[jj * TS_LD + d], acc);
    ob[(size_t)t * ots + d] = acc;
  }
}

// the saved p, keep and dout rows of width E at dout + b gbs + t gts -> dqkv rows [dq | dk | dv] at dqkv + b dbs + t dts, every element written
__global__ __launch_bounds__(64) void token_attn_bwd_kernel(const float* __restrict__ qkv, const float* __restrict__ keep, const float* __restrict__ p,
                                                            const float* __restrict__ dout, float* __restrict__ dqkv, const int T, const int E,
                                                            const int hd, const long long qbs, const long long qts, const long long gbs,
                                                            const long long gts, const long long dbs, const long long dts, const float scale) {
  const int b = blockIdx.x, h = blockIdx.y, H = gridDim.y, lane = threadIdx.x;
  __shared__ float sQ[TS_MAXT * TS_LD], sK[TS_MAXT * TS_LD], sV[TS_MAXT * TS_LD], sG[TS_MAXT * TS_LD];
  __shared__ float sPk[TS_MAXT * TS_PLD], sDs[TS_MAXT * TS_PLD];
  const float* base = qkv + (size_t)b * qbs + h * hd;
  const float* gbase = dout + (size_t)b * gbs + h * hd;
  const int hv = hd >> 2;
  for (int idx = lane; idx < T * hv; idx += 64) {
    const int t = idx / hv, c = (idx - t * hv) * 4;
    const float* r = base + (size_t)t * qts + c;
    put4(&sQ[t * TS_LD + c], ld4(r));
    put4(&sK[t * TS_LD + c], ld4(r + E));
    put4(&sV[t * TS_LD + c], ld4(r + 2 * E));
    put4(&sG[t * TS_LD + c], ld4(gbase + (size_t)t * gts + c));
  }
  __syncthreads();
  const int i = lane >> 3, j = lane & 7;
  const bool live = i < T && j < T;
  const size_t pij = (((size_t)b * H + h) * T + min(i, T - 1)) * T + min(j, T - 1);
  const float pv = live ? p[pij] : 0.f;
  const float kp = live ? (keep ? keep[pij] : 1.f) : 0.f;
  const float* gi = &sG[min(i, T - 1) * TS_LD];
  const float* vj = &sV[min(j, T - 1) * TS_LD];
  float dp = 0.f;
  for (int d = 0; d < hd; ++d) dp = fmaf(gi[d], vj[d], dp);
  dp *= kp;                                                    // dP = (dO V^T) keep; a row whose keep is all zero: dP = 0, dS = 0
  const float rs = row8_sum(dp * pv);
  sDs[i * TS_PLD + j] = scale * (pv * (dp - rs));
  sPk[i * TS_PLD + j] = pv * kp;
  __syncthreads();
  float* db = dqkv + (size_t)b * dbs + h * hd;
  for (int idx = lane; idx < T * hd; idx += 64) {
    const int t = idx / hd, d = idx - t * hd;
    float dq = 0.f, dk = 0.f, dv = 0.f;
    for (int u = 0; u < T; ++u) {
      dq = fmaf(sDs[t * TS_PLD + u], sK[u * TS_LD + d], dq);
      dk = fmaf(sDs[u * TS_PLD + t], sQ[u * TS_LD + d], dk);
      dv = fmaf(sPk[u * TS_PLD + t], sG[u * TS_LD + d], dv);
    }
    float* r = db + (size_t)t * dts + d;
    r[0] = dq; r[E] = dk; r[2 * E] = dv;
  }
}

// the T scores of sample b and their softmax, in every lane of the calling wave: s_t = sum_d w_d hv[t, d] hu[t, d] + bias
__device__ __forceinline__ void pool_scores(const float* __restrict__ h2b, const float* __restrict__ w, const float bias, const int T, const int D,
                                            const int lane, float (&s)[TS_MAXT], float (&a)[TS_MAXT]) {
  const bool dc = 4 * lane < D;
  const int d0 = dc ? 4 * lane : 0;
  const float4 wv = dc ? ld4(w + d0) : make_float4(0.f, 0.f, 0.f, 0.f);
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < TS_MAXT; ++t) {
    s[t] = -INFINITY;
    if (t < T) {
      const float4 v = ld4(h2b + (size_t)t * 2 * D + d0), u = ld4(h2b + (size_t)t * 2 * D + D + d0);
      s[t] = wave_sum(dot4(wv, make_float4(v.x * u.x, v.y * u.y, v.z * u.z, v.w * u.w))) + bias;
      m = fmaxf(m, s[t]);
    }
  }
  float l = 0.f;
#pragma unroll
  for (int t = 0; t < TS_MAXT; ++t) { a[t] = t < T ? expf(s[t] - m) : 0.f; l += a[t]; }
  const float inv = 1.f / l;
#pragma unroll
  for (int t = 0; t < TS_MAXT; ++t) a[t] *= inv;
}

// x rows of width E at x + b xbs + t xts, h2 [B, T, 2 D] -> s [B, T], a [B, T], out [B, E]
__global__ __launch_bounds__(TS_POOL_THREADS) void token_pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ h2,
                                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                                         float* __restrict__ s_out, float* __restrict__ a_out, float* __restrict__ out,
                                                                         const int T, const int E, const int D, const long long xbs, const long long xts) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  float s[TS_MAXT], a[TS_MAXT];
  pool_scores(h2 + (size_t)b * T * 2 * D, w, bias[0], T, D, lane, s, a);
  if (tid < T) {
#pragma unroll
    for (int t = 0; t < TS_MAXT; ++t)
      if (t == tid) { s_out[(size_t)b * T + t] = s[t]; a_out[(size_t)b * T + t] = a[t]; }
  }
  if (4 * tid < E) {
    const float* xb = x + (size_t)b * xbs + 4 * tid;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < TS_MAXT; ++t) {
      if (t < T) {
        const float4 v = ld4(xb + (size_t)t * xts);
        acc.x = fmaf(a[t], v.x, acc.x); acc.y = fmaf(a[t], v.y, acc.y); acc.z = fmaf(a[t], v.z, acc.z); acc.w = fmaf(a[t], v.w, acc.w);
      }
    }
    *reinterpret_cast<float4*>(out + (size_t)b * E + 4 * tid) = acc;
  }
}

// ds_t = a_t (tau_t - sum_t a_t tau_t), tau_t = dM . x_t, of sample b, in every lane of the calling wave (t >= T: 0)
__device__ __forceinline__ void pool_ds(const float* __restrict__ xb, const long long xts, const float* __restrict__ ab, const float* __restrict__ gb,
                                        const int T, const int E, const int lane, float (&a)[TS_MAXT], float (&ds)[TS_MAXT]) {
  bool ec[2];
  int eo[2];
  float4 g[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    ec[k] = k * 256 + 4 * lane < E; eo[k] = ec[k] ? k * 256 + 4 * lane : 0;
    g[k] = ec[k] ? ld4(gb + eo[k]) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  // the tokens of a set can be close to one another (MCAT's four co-attended rows): tau_t - c then cancels to a few digits, so the dots and
  // c stay in fp64 up to the difference, as smml_attn_pool_bwd_f32 keeps them
  double tau[TS_MAXT], c = 0.0;
#pragma unroll
  for (int t = 0; t < TS_MAXT; ++t) {
    a[t] = 0.f; tau[t] = 0.0;
    if (t < T) {
      a[t] = ab[t];
      tau[t] = wave_sum_f64(dot4_f64(g[0], ld4(xb + (size_t)t * xts + eo[0])) + dot4_f64(g[1], ld4(xb + (size_t)t * xts + eo[1])));
      c = fma((double)a[t], tau[t], c);
    }
  }
#pragma unroll
  for (int t = 0; t < TS_MAXT; ++t) ds[t] = (float)((double)a[t] * (tau[t] - c));
}

// grid B + 1: workgroup b < B writes dx (rows at dx + b dxbs + t dxts) and dh2 [B, T, 2 D] of sample b, workgroup B writes dw [D] and db [1]
__global__ __launch_bounds__(TS_POOL_THREADS) void token_pool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ h2,
                                                                         const float* __restrict__ w, const float* __restrict__ a_in,
                                                                         const float* __restrict__ dout, float* __restrict__ dx, float* __restrict__ dh2,
                                                                         float* __restrict__ dw, float* __restrict__ dbias, const int B, const int T,
                                                                         const int E, const int D, const long long xbs, const long long xts,
                                                                         const long long dxbs, const long long dxts) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool dc = 4 * lane < D;
  const int d0 = dc ? 4 * lane : 0;
  float a[TS_MAXT], ds[TS_MAXT];
  if ((int)blockIdx.x < B) {
    const int b = blockIdx.x;
    const float* gb = dout + (size_t)b * E;
    pool_ds(x + (size_t)b * xbs, xts, a_in + (size_t)b * T, gb, T, E, lane, a, ds);
    const float4 wv = dc ? ld4(w + d0) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int t = 0; t < TS_MAXT; ++t) {
      if (t < T && (t & 3) == wave) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int e0 = k * 256 + 4 * lane;
          if (e0 < E) {
            const float4 g = ld4(gb + e0);
            *reinterpret_cast<float4*>(dx + (size_t)b * dxbs + (size_t)t * dxts + e0) = make_float4(a[t] * g.x, a[t] * g.y, a[t] * g.z, a[t] * g.w);
          }
        }
        if (dc) {
          const float* hr = h2 + ((size_t)b * T + t) * 2 * D;
          float* dr = dh2 + ((size_t)b * T + t) * 2 * D;
          const float4 v = ld4(hr + d0), u = ld4(hr + D + d0);
          const float4 gw = make_float4(ds[t] * wv.x, ds[t] * wv.y, ds[t] * wv.z, ds[t] * wv.w);
          *reinterpret_cast<float4*>(dr + d0) = make_float4(gw.x * u.x, gw.y * u.y, gw.z * u.z, gw.w * u.w);
          *reinterpret_cast<float4*>(dr + D + d0) = make_float4(gw.x * v.x, gw.y * v.y, gw.z * v.z, gw.w * v.w);
        }
      }
    }
    return;
  }
  // the owner of dw and db: samples wave, wave + 4, ... in ascending order per wave, then the four waves in wave order
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float accb = 0.f;
  for (int b = wave; b < B; b += 4) {
    pool_ds(x + (size_t)b * xbs, xts, a_in + (size_t)b * T, dout + (size_t)b * E, T, E, lane, a, ds);
#pragma unroll
    for (int t = 0; t < TS_MAXT; ++t) {
      if (t < T) {
        const float* hr = h2 + ((size_t)b * T + t) * 2 * D;
        const float4 v = ld4(hr + d0), u = ld4(hr + D + d0);
        acc.x = fmaf(ds[t], v.x * u.x, acc.x); acc.y = fmaf(ds[t], v.y * u.y, acc.y);
        acc.z = fmaf(ds[t], v.z * u.z, acc.z); acc.w = fmaf(ds[t], v.w * u.w, acc.w);
        accb += ds[t];
      }
    }
  }
  __shared__ __attribute__((aligned(16))) float sW[4][TS_MAXD];
  __shared__ float sB[4];
  if (dc) *reinterpret_cast<float4*>(&sW[wave][d0]) = acc;
  if (lane == 0) sB[wave] = accb;
  __syncthreads();
  for (int d = tid; d < D; d += TS_POOL_THREADS) dw[d] = ((sW[0][d] + sW[1][d]) + sW[2][d]) + sW[3][d];
  if (tid == 0) dbias[0] = ((sB[0] + sB[1]) + sB[2]) + sB[3];
}

bool aligned16(const void* p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }
// rows of width `width` with unit column stride: tokens and samples a multiple of four floats apart, tokens at least the width apart
bool strides_ok(long long bs, long long ts, int width) { return bs >= 0 && ts >= width && bs % 4 == 0 && ts % 4 == 0; }
bool attn_shape_ok(int B, int T, int E, int H) {
  if (B <= 0 || T <= 0 || T > TS_MAXT || E <= 0 || E > TS_MAXE || E % 64 || H <= 0 || E % H) return false;
  return E / H == 32 || E / H == 64;
}
bool pool_shape_ok(int B, int T, int E, int D) {
  return B > 0 && B < (1 << 30) && T > 0 && T <= TS_MAXT && E > 0 && E <= TS_MAXE && E % 64 == 0 && D > 0 && D <= TS_MAXD && D % 64 == 0;
}

}  // namespace

extern "C" {

int smml_token_attn_fwd_f32(const float* qkv, const float* keep, float* o, float* p, int B, int T, int E, int H, long long qkv_batch_stride,
                            long long qkv_token_stride, long long o_batch_stride, long long o_token_stride, float scale, void* stream) {
  const char* fn = "smml_token_attn_fwd_f32";
  SMML_REQUIRE(qkv && o && p, "%s: null pointer", fn);
  SMML_REQUIRE(attn_shape_ok(B, T, E, H), "%s: need 1 <= T <= %d tokens, E a multiple of 64 up to %d, a head dim E / H of 32 or 64, B >= 1 "
               "(got B %d, T %d, E %d, H %d)", fn, TS_MAXT, TS_MAXE, B, T, E, H);
  SMML_REQUIRE(strides_ok(qkv_batch_stride, qkv_token_stride, 3 * E) && strides_ok(o_batch_stride, o_token_stride, E),
               "%s: token and batch strides must be multiples of 4 floats, tokens at least their row's width apart", fn);
  SMML_REQUIRE(aligned16(qkv) && aligned16(o), "%s: qkv and o must be 16-byte aligned", fn);
  hipLaunchKernelGGL(token_attn_fwd_kernel, dim3((unsigned)B, (unsigned)H), dim3(64), 0, (hipStream_t)stream, qkv, keep, o, p, T, E, E / H,
                     qkv_batch_stride, qkv_token_stride, o_batch_stride, o_token_stride, scale);
  SMML_LAUNCH_CHECK(fn);
  return SMML_OK;
}

int smml_token_attn_bwd_f32(const float* qkv, const float* keep, const float* p, const float* dout, float* dqkv, int B, int T, int E, int H,
                            long long qkv_batch_stride, long long qkv_token_stride, long long dout_batch_stride, long long dout_token_stride,
                            long long dqkv_batch_stride, long long dqkv_token_stride, float scale, void* stream) {
  const char* fn = "smml_token_attn_bwd_f32";
  SMML_REQUIRE(qkv && p && dout && dqkv, "%s: null pointer", fn);
  SMML_REQUIRE(attn_shape_ok(B, T, E, H), "%s: need 1 <= T <= %d tokens, E a multiple of 64 up to %d, a head dim E / H of 32 or 64, B >= 1 "
               "(got B %d, T %d, E %d, H %d)", fn, TS_MAXT, TS_MAXE, B, T, E, H);
  SMML_REQUIRE(strides_ok(qkv_batch_stride, qkv_token_stride, 3 * E) && strides_ok(dout_batch_stride, dout_token_stride, E) &&
               strides_ok(dqkv_batch_stride, dqkv_token_stride, 3 * E),
               "%s: token and batch strides must be multiples of 4 floats, tokens at least their row's width apart", fn);
  SMML_REQUIRE(aligned16(qkv) && aligned16(dout) && aligned16(dqkv), "%s: qkv, dout and dqkv must be 16-byte aligned", fn);
  hipLaunchKernelGGL(token_attn_bwd_kernel, dim3((unsigned)B, (unsigned)H), dim3(64), 0, (hipStream_t)stream, qkv, keep, p, dout, dqkv, T, E, E / H,
                     qkv_batch_stride, qkv_token_stride, dout_batch_stride, dout_token_stride, dqkv_batch_stride, dqkv_token_stride, scale);
  SMML_LAUNCH_CHECK(fn);
  return SMML_OK;
}

int smml_token_pool_gated_fwd_f32(const float* x, const float* h2, const float* w, const float* b, float* s, float* a, float* out, int B, int T,
                                  int E, int D, long long x_batch_stride, long long x_token_stride, void* stream) {
  const char* fn = "smml_token_pool_gated_fwd_f32";
  SMML_REQUIRE(x && h2 && w && b && s && a && out, "%s: null pointer", fn);
  SMML_REQUIRE(pool_shape_ok(B, T, E, D), "%s: need 1 <= T <= %d tokens, E a multiple of 64 up to %d, D a multiple of 64 up to %d, B >= 1 "
               "(got B %d, T %d, E %d, D %d)", fn, TS_MAXT, TS_MAXE, TS_MAXD, B, T, E, D);
  SMML_REQUIRE(strides_ok(x_batch_stride, x_token_stride, E), "%s: token and batch strides must be multiples of 4 floats, tokens at least E apart", fn);
  SMML_REQUIRE(aligned16(x) && aligned16(h2) && aligned16(w) && aligned16(out), "%s: x, h2, w and out must be 16-byte aligned", fn);
  hipLaunchKernelGGL(token_pool_fwd_kernel, dim3((unsigned)B), dim3(TS_POOL_THREADS), 0, (hipStream_t)stream, x, h2, w, b, s, a, out, T, E, D,
                     x_batch_stride, x_token_stride);
  SMML_LAUNCH_CHECK(fn);
  return SMML_OK;
}

int smml_token_pool_gated_bwd_f32(const float* x, const float* h2, const float* w, const float* a, const float* dout, float* dx, float* dh2,
                                  float* dw, float* db, int B, int T, int E, int D, long long x_batch_stride, long long x_token_stride,
                                  long long dx_batch_stride, long long dx_token_stride, void* stream) {
  const char* fn = "smml_token_pool_gated_bwd_f32";
  SMML_REQUIRE(x && h2 && w && a && dout && dx && dh2 && dw && db, "%s: null pointer", fn);
  SMML_REQUIRE(pool_shape_ok(B, T, E, D), "%s: need 1 <= T <= %d tokens, E a multiple of 64 up to %d, D a multiple of 64 up to %d, B >= 1 "
               "(got B %d, T %d, E %d, D %d)", fn, TS_MAXT, TS_MAXE, TS_MAXD, B, T, E, D);
  SMML_REQUIRE(strides_ok(x_batch_stride, x_token_stride, E) && strides_ok(dx_batch_stride, dx_token_stride, E),
               "%s: token and batch strides must be multiples of 4 floats, tokens at least E apart", fn);
  SMML_REQUIRE(aligned16(x) && aligned16(h2) && aligned16(w) && aligned16(dout) && aligned16(dx) && aligned16(dh2),
               "%s: x, h2, w, dout, dx and dh2 must be 16-byte aligned", fn);
  hipLaunchKernelGGL(token_pool_bwd_kernel, dim3((unsigned)B + 1u), dim3(TS_POOL_THREADS), 0, (hipStream_t)stream, x, h2, w, a, dout, dx, dh2, dw, db,
                     B, T, E, D, x_batch_stride, x_token_stride, dx_batch_stride, dx_token_stride);
  SMML_LAUNCH_CHECK(fn);
  return SMML_OK;
}

}  // extern "C"
