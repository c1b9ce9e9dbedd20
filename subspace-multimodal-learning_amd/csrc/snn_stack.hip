// Self-normalising (SNN) encoder stacks: G <= 8 independent networks of `depth` <= 4 layers Linear -> ELU -> AlphaDropout each (MCAT_Surv / CMTA
// sig_networks, models/mcat_utils.py:81-95; MaxNet, models/model.py:142-187), every network of a model in ONE forward launch and TWO backward
// launches.  The arithmetic is tiny (B <= 8 rows per rank, about 100 000 weights per network): what the composed form spends is launches - a
// GEMM, an ELU and the seven elementwise kernels of ATen's AlphaDropout per layer, and as many again backward.
//
//   forward   grid (row tiles of 8, G), 8 waves.  The tile's input rows and two ping-pong activation buffers live in LDS; the layers of a
//             network are chained inside its workgroup with __syncthreads alone - no workgroup waits on another.  Per layer a wave owns groups
//             of 4 output columns: it reads their weight rows coalesced (float4 where the rows are 16-byte aligned, scalar otherwise: a row of
//             59 or 361 floats is not), keeps one accumulator per (column, row) and closes the 32 dot products with ONE folding butterfly -
//             at every step a lane hands the half of its values its partner keeps to that partner - 32 shuffles instead of 192.
//   chain     grid as the forward, 4 waves: dz_l = da_l . A keep . elu'(e_l) goes to the scratch and to LDS [n][8]; thread k then owns
//             da_{l-1}[:, k] = sum_n dz_l[:, n] W_l[n, k] (W read along k: coalesced), n ascending.  dx only where it is asked for.
//   weights   grid (groups of 4 rows of dW, G depth): thread k owns dW_l[n0 .. n0 + 3, k] = sum_b dz_l[b, n] a_{l-1}[b, k], b ascending; a_{l-1}
//             is the input or is re-formed from the saved e_{l-1} and keep.  db_l[n] = sum_b dz_l[b, n] has one owner as well.
// No float atomics, no hand-off between workgroups, one owner and one order per sum: the results are a function of the inputs alone.
#include "smml_common.h"

#include <math.h>

namespace {

constexpr int SNN_MAXG = 8;
constexpr int SNN_MAXDEPTH = 4;
constexpr int SNN_MAXN = 256;
constexpr int SNN_MAXK0 = 2048;
constexpr int SNN_ROWS = 8;            // rows of a tile
constexpr int SNN_FWD_THREADS = 512;
constexpr int SNN_FWD_WAVES = SNN_FWD_THREADS / 64;
constexpr int SNN_CB = 4;              // columns a wave carries at once
constexpr int SNN_BWD_THREADS = 256;
constexpr int SNN_WROWS = 4;           // rows of dW per workgroup of the weight pass
constexpr double SNN_ALPHA = 1.7580993408473766;      // torch's AlphaDropout: -selu_scale * selu_alpha

// the kernels' by-value argument: filled by the entry points from the caller's host tables during the call
struct SnnArgs {
  const float* x[SNN_MAXG];                        // first element of network g's rows (the column offset applied)
  long long xs[SNN_MAXG];                          // their row stride, floats
  const float* W[SNN_MAXG][SNN_MAXDEPTH];
  const float* b[SNN_MAXG][SNN_MAXDEPTH];
  float* out[SNN_MAXG];
  const float* dout[SNN_MAXG];
  float* dW[SNN_MAXG][SNN_MAXDEPTH];
  float* db[SNN_MAXG][SNN_MAXDEPTH];
  float* dx[SNN_MAXG];
  long long off[SNN_MAXG][SNN_MAXDEPTH];           // where e_l [B, N_l] of network g starts in acts / keep / dz, floats
  int width[SNN_MAXG][SNN_MAXDEPTH + 1];           // K_0, N_1 .. N_depth
  const float* keep;
  float* acts;
  float* dz;
  int depth, B, final_relu, ldx, lda;
  float ca, cb, cbp;                               // A, A alpha', A alpha' p
};

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float elu(const float z) { return z > 0.f ? z : expm1f(z); }
// torch's AlphaDropout given the 0 / 1 multiplier kp: A kp e + A alpha' (kp - 1) + A alpha' p
__device__ __forceinline__ float alpha_drop(const SnnArgs& a, const float e, const float kp) {
  return fmaf(e, a.ca * kp, fmaf(a.cb, kp - 1.f, a.cbp));
}

// One step of the folding butterfly that closes the wave's 32 dot products: at lane bit 2 HALF the lanes with the bit set keep the upper HALF of
// the values, the others the lower HALF, and each adds what its partner held of the half it keeps.  After the steps 16, 8, 4, 2, 1 a lane holds
// value (lane >> 1) summed over every lane but its pair's other one.  Every index is a constant (the values stay in registers), and every
// lane adds the same operands in the same order run after run.
template <int HALF> __device__ __forceinline__ void fold_step(float (&v)[SNN_CB * SNN_ROWS], const int lane) {
  static_assert(SNN_CB * SNN_ROWS == 32, "the fold is written for 32 values over 64 lanes");
  const bool hi = (lane & (2 * HALF)) != 0;
#pragma unroll
  for (int i = 0; i < HALF; ++i) {
    const float send = hi ? v[i] : v[i + HALF];
    const float kept = hi ? v[i + HALF] : v[i];
    v[i] = kept + __shfl_xor(send, 2 * HALF);
  }
}

__global__ __launch_bounds__(SNN_FWD_THREADS) void snn_fwd_kernel(const SnnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float snn_smem[];
  const int g = blockIdx.y, r0 = blockIdx.x * SNN_ROWS, R = min(SNN_ROWS, a.B - r0);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* sx = snn_smem;                              // [8][ldx]: the input rows
  float* sa0 = sx + SNN_ROWS * a.ldx;                // [8][lda] twice: the activations, ping-pong
  float* sa1 = sa0 + SNN_ROWS * a.lda;
  const int K0 = a.width[g][0];
  const float* __restrict__ xg = a.x[g];
  const long long xs = a.xs[g];
  for (int idx = tid; idx < SNN_ROWS * a.ldx; idx += SNN_FWD_THREADS) {
    const int r = idx / a.ldx, k = idx - r * a.ldx;
    sx[idx] = (r < R && k < K0) ? xg[(long long)(r0 + r) * xs + k] : 0.f;
  }
  for (int idx = tid; idx < 2 * SNN_ROWS * a.lda; idx += SNN_FWD_THREADS) sa0[idx] = 0.f;      // rows past R stay zero
  __syncthreads();
  const float* in = sx;
  int ldin = a.ldx;
  for (int l = 0; l < a.depth; ++l) {
    const int K = a.width[g][l], N = a.width[g][l + 1];
    const float* __restrict__ W = a.W[g][l];
    const float* __restrict__ bias = a.b[g][l];
    float* __restrict__ out = a.out[g];
    float* nxt = (l & 1) ? sa1 : sa0;
    const bool last = l + 1 == a.depth;
    const bool vec = (K & 3) == 0 && (reinterpret_cast<size_t>(W) & 15) == 0;      // every weight row starts on 16 bytes
    const long long off = a.off[g][l];
    for (int n0 = wave * SNN_CB; n0 < N; n0 += SNN_FWD_WAVES * SNN_CB) {
      float v[SNN_CB * SNN_ROWS];
#pragma unroll
      for (int i = 0; i < SNN_CB * SNN_ROWS; ++i) v[i] = 0.f;
      const float* wr[SNN_CB];
#pragma unroll
      for (int c = 0; c < SNN_CB; ++c) wr[c] = W + (size_t)min(n0 + c, N - 1) * K;
      if (vec) {
        for (int k = 4 * lane; k < K; k += 256) {
          float4 xv[SNN_ROWS];
#pragma unroll
          for (int r = 0; r < SNN_ROWS; ++r) xv[r] = ld4(in + r * ldin + k);
#pragma unroll
          for (int c = 0; c < SNN_CB; ++c) {
            const float4 w = ld4(wr[c] + k);
#pragma unroll
            for (int r = 0; r < SNN_ROWS; ++r)
              v[c * SNN_ROWS + r] = fmaf(w.x, xv[r].x, fmaf(w.y, xv[r].y, fmaf(w.z, xv[r].z, fmaf(w.w, xv[r].w, v[c * SNN_ROWS + r]))));
          }
        }
      } else {
        for (int k = lane; k < K; k += 64) {
          float xv[SNN_ROWS];
#pragma unroll
          for (int r = 0; r < SNN_ROWS; ++r) xv[r] = in[r * ldin + k];
#pragma unroll
          for (int c = 0; c < SNN_CB; ++c) {
            const float w = wr[c][k];
#pragma unroll
            for (int r = 0; r < SNN_ROWS; ++r) v[c * SNN_ROWS + r] = fmaf(w, xv[r], v[c * SNN_ROWS + r]);
          }
        }
      }
      fold_step<16>(v, lane);
      fold_step<8>(v, lane);
      fold_step<4>(v, lane);
      fold_step<2>(v, lane);
      fold_step<1>(v, lane);
      const float sum = v[0] + __shfl_xor(v[0], 1);
      const int idx = lane >> 1, c = idx >> 3, r = idx & 7, n = n0 + c;
      if (!(lane & 1) && n < N && r < R) {
        const float e = elu(sum + bias[n]);
        const long long o = off + (long long)(r0 + r) * N + n;
        a.acts[o] = e;
        const float y = a.keep ? alpha_drop(a, e, a.keep[o]) : e;
        if (last)
          out[(long long)(r0 + r) * N + n] = a.final_relu ? fmaxf(y, 0.f) : y;
        else
          nxt[r * a.lda + n] = y;
      }
    }
    __syncthreads();
    in = nxt;
    ldin = a.lda;
  }
}

// dz_l of every layer into a.dz (the layout of acts), dx where a.dx[g] is set
__global__ __launch_bounds__(SNN_BWD_THREADS) void snn_bwd_chain_kernel(const SnnArgs a) {
  __shared__ __attribute__((aligned(16))) float sda[SNN_MAXN * SNN_ROWS];      // da_l [n][8]
  __shared__ __attribute__((aligned(16))) float sdz[SNN_MAXN * SNN_ROWS];      // dz_l [n][8]
  const int g = blockIdx.y, r0 = blockIdx.x * SNN_ROWS, R = min(SNN_ROWS, a.B - r0);
  const int tid = threadIdx.x;
  {
    const int N = a.width[g][a.depth];
    const float* __restrict__ dout = a.dout[g];
    const float* __restrict__ out = a.out[g];
    for (int idx = tid; idx < SNN_ROWS * N; idx += SNN_BWD_THREADS) {
      const int r = idx / N, n = idx - r * N;
      float d = 0.f;
      if (r < R && dout) {
        const long long o = (long long)(r0 + r) * N + n;
        d = dout[o];
        if (a.final_relu && !(out[o] > 0.f)) d = 0.f;
      }
      sda[n * SNN_ROWS + r] = d;
    }
  }
  __syncthreads();
  for (int l = a.depth - 1; l >= 0; --l) {
    const int K = a.width[g][l], N = a.width[g][l + 1];
    const long long off = a.off[g][l];
    for (int idx = tid; idx < SNN_ROWS * N; idx += SNN_BWD_THREADS) {
      const int r = idx / N, n = idx - r * N;
      float d = 0.f;
      if (r < R) {
        const long long o = off + (long long)(r0 + r) * N + n;
        const float e = a.acts[o];
        d = sda[n * SNN_ROWS + r] * (e > 0.f ? 1.f : e + 1.f);
        if (a.keep) d *= a.ca * a.keep[o];
        a.dz[o] = d;
      }
      sdz[n * SNN_ROWS + r] = d;
    }
    __syncthreads();
    float* __restrict__ dx = a.dx[g];
    if (l == 0 && !dx) break;
    const float* __restrict__ W = a.W[g][l];
    for (int k = tid; k < K; k += SNN_BWD_THREADS) {
      float acc[SNN_ROWS];
#pragma unroll
      for (int r = 0; r < SNN_ROWS; ++r) acc[r] = 0.f;
#pragma unroll 4
      for (int n = 0; n < N; ++n) {
        const float w = W[(size_t)n * K + k];
        const float4 d0 = ld4(&sdz[n * SNN_ROWS]), d1 = ld4(&sdz[n * SNN_ROWS + 4]);
        acc[0] = fmaf(d0.x, w, acc[0]); acc[1] = fmaf(d0.y, w, acc[1]); acc[2] = fmaf(d0.z, w, acc[2]); acc[3] = fmaf(d0.w, w, acc[3]);
        acc[4] = fmaf(d1.x, w, acc[4]); acc[5] = fmaf(d1.y, w, acc[5]); acc[6] = fmaf(d1.z, w, acc[6]); acc[7] = fmaf(d1.w, w, acc[7]);
      }
      if (l == 0) {
#pragma unroll
        for (int r = 0; r < SNN_ROWS; ++r)
          if (r < R) dx[(long long)(r0 + r) * K + k] = acc[r];
      } else {                                      // K = N_l <= 256: one thread per column, nobody reads sda before the barrier
#pragma unroll
        for (int r = 0; r < SNN_ROWS; ++r) sda[k * SNN_ROWS + r] = acc[r];
      }
    }
    __syncthreads();
  }
}

// grid (groups of SNN_WROWS rows of dW, G depth): dW_l and db_l of every layer from a.dz, sums over the rows b = 0 .. B - 1 in that order
__global__ __launch_bounds__(SNN_BWD_THREADS) void snn_bwd_weight_kernel(const SnnArgs a) {
  const int g = blockIdx.y / a.depth, l = blockIdx.y - g * a.depth;
  const int K = a.width[g][l], N = a.width[g][l + 1], n0 = blockIdx.x * SNN_WROWS, tid = threadIdx.x;
  if (n0 >= N) return;
  const float* __restrict__ dz = a.dz + a.off[g][l];
  const float* __restrict__ x = a.x[g];
  const long long xs = a.xs[g];
  const float* __restrict__ prev = l ? a.acts + a.off[g][l - 1] : nullptr;          // e_{l-1} [B, K]
  const float* __restrict__ kprev = l && a.keep ? a.keep + a.off[g][l - 1] : nullptr;
  float* __restrict__ dW = a.dW[g][l];
  int nc[SNN_WROWS];
#pragma unroll
  for (int c = 0; c < SNN_WROWS; ++c) nc[c] = min(n0 + c, N - 1);
  for (int k = tid; k < K; k += SNN_BWD_THREADS) {
    float acc[SNN_WROWS];
#pragma unroll
    for (int c = 0; c < SNN_WROWS; ++c) acc[c] = 0.f;
    for (int bb = 0; bb < a.B; ++bb) {
      float av;
      if (l == 0) {
        av = x[(long long)bb * xs + k];
      } else {
        av = prev[(long long)bb * K + k];
        if (kprev) av = alpha_drop(a, av, kprev[(long long)bb * K + k]);
      }
#pragma unroll
      for (int c = 0; c < SNN_WROWS; ++c) acc[c] = fmaf(dz[(long long)bb * N + nc[c]], av, acc[c]);
    }
#pragma unroll
    for (int c = 0; c < SNN_WROWS; ++c)
      if (n0 + c < N) dW[(size_t)(n0 + c) * K + k] = acc[c];
  }
  if (tid < SNN_WROWS && n0 + tid < N) {
    float s = 0.f;
    for (int bb = 0; bb < a.B; ++bb) s += dz[(long long)bb * N + n0 + tid];
    a.db[g][l][n0 + tid] = s;
  }
}

template <typename T> T* as_ptr(unsigned long long v) { return reinterpret_cast<T*>(static_cast<uintptr_t>(v)); }

// the checks both directions share, then the part of SnnArgs both fill; every host table is read only after it is known to be there
int snn_fill(const char* fn, SnnArgs& a, const unsigned long long* x, const long long* x_row_stride, const long long* x_col_offset,
             const unsigned long long* W, const int* widths, const float* keep, int G, int depth, int B, float p, int final_relu) {
  SMML_REQUIRE(x && x_row_stride && x_col_offset && W && widths, "%s: null table (x, x_row_stride, x_col_offset, W and widths are host arrays)", fn);
  SMML_REQUIRE(G >= 1 && G <= SNN_MAXG, "%s: %d networks (1 to %d)", fn, G, SNN_MAXG);
  SMML_REQUIRE(depth >= 1 && depth <= SNN_MAXDEPTH, "%s: depth %d (1 to %d layers)", fn, depth, SNN_MAXDEPTH);
  SMML_REQUIRE(B >= 1 && B < (1 << 28), "%s: %d rows (at least 1, below 2^28)", fn, B);
  SMML_REQUIRE(p >= 0.f && p < 1.f, "%s: dropout rate %g (0 <= p < 1)", fn, (double)p);
  SMML_REQUIRE((p > 0.f) == (keep != nullptr), "%s: keep is required with p > 0 and must be null with p = 0", fn);
  SMML_REQUIRE(final_relu == 0 || final_relu == 1, "%s: final_relu is 0 or 1 (got %d)", fn, final_relu);
  a = SnnArgs{};
  long long off = 0;
  int ldx = 0, lda = 0;
  for (int g = 0; g < G; ++g) {
    const int* w = widths + (size_t)g * (depth + 1);
    SMML_REQUIRE(w[0] >= 1 && w[0] <= SNN_MAXK0, "%s: network %d has %d inputs (1 to %d)", fn, g, w[0], SNN_MAXK0);
    SMML_REQUIRE(x[g] != 0 && x_row_stride[g] >= 0 && x_col_offset[g] >= 0, "%s: network %d: null input, or a negative stride or offset", fn, g);
    a.x[g] = as_ptr<const float>(x[g]) + x_col_offset[g];
    a.xs[g] = x_row_stride[g];
    a.width[g][0] = w[0];
    ldx = w[0] > ldx ? w[0] : ldx;
    for (int l = 0; l < depth; ++l) {
      const int n = w[l + 1];
      SMML_REQUIRE(n >= 1 && n <= SNN_MAXN, "%s: layer %d of network %d has width %d (1 to %d)", fn, l, g, n, SNN_MAXN);
      SMML_REQUIRE(W[g * depth + l] != 0, "%s: null weight of layer %d of network %d", fn, l, g);
      a.W[g][l] = as_ptr<const float>(W[g * depth + l]);
      a.width[g][l + 1] = n;
      a.off[g][l] = off;
      off += (long long)B * n;
      lda = n > lda ? n : lda;
    }
  }
  a.keep = keep;
  a.depth = depth;
  a.B = B;
  a.final_relu = final_relu;
  a.ldx = (ldx + 3) & ~3;
  a.lda = (lda + 3) & ~3;
  const double A = 1.0 / sqrt((SNN_ALPHA * SNN_ALPHA * (double)p + 1.0) * (1.0 - (double)p));
  a.ca = (float)A;
  a.cb = (float)(A * SNN_ALPHA);
  a.cbp = (float)(A * SNN_ALPHA * (double)p);
  return SMML_OK;
}

}  // namespace

extern "C" {

int smml_snn_stack_fwd_f32(const unsigned long long* x, const long long* x_row_stride, const long long* x_col_offset, const unsigned long long* W,
                           const unsigned long long* b, const int* widths, const float* keep, float* acts, const unsigned long long* out, int G,
                           int depth, int B, float p, int final_relu, void* stream) {
  const char* fn = "smml_snn_stack_fwd_f32";
  SMML_REQUIRE(b && out && acts, "%s: null pointer (b and out are host arrays, acts is device memory)", fn);
  SnnArgs a;
  if (int rc = snn_fill(fn, a, x, x_row_stride, x_col_offset, W, widths, keep, G, depth, B, p, final_relu)) return rc;
  for (int g = 0; g < G; ++g) {
    SMML_REQUIRE(out[g] != 0, "%s: null output of network %d", fn, g);
    a.out[g] = as_ptr<float>(out[g]);
    for (int l = 0; l < depth; ++l) {
      SMML_REQUIRE(b[g * depth + l] != 0, "%s: null bias of layer %d of network %d", fn, l, g);
      a.b[g][l] = as_ptr<const float>(b[g * depth + l]);
    }
  }
  a.acts = acts;
  const size_t lds = ((size_t)SNN_ROWS * a.ldx + 2 * (size_t)SNN_ROWS * a.lda) * sizeof(float);
  if (lds > 48 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(snn_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    SMML_REQUIRE(e == hipSuccess, "%s: hipFuncSetAttribute failed: %s", fn, hipGetErrorString(e));
  }
  hipLaunchKernelGGL(snn_fwd_kernel, dim3((unsigned)((B + SNN_ROWS - 1) / SNN_ROWS), (unsigned)G), dim3(SNN_FWD_THREADS), lds, (hipStream_t)stream, a);
  SMML_LAUNCH_CHECK(fn);
  return SMML_OK;
}

int smml_snn_stack_bwd_f32(const unsigned long long* x, const long long* x_row_stride, const long long* x_col_offset, const unsigned long long* W,
                           const int* widths, const float* keep, const float* acts, const unsigned long long* out, const unsigned long long* dout,
                           float* dz, const unsigned long long* dW, const unsigned long long* db, const unsigned long long* dx, int G, int depth,
                           int B, float p, int final_relu, void* stream) {
  const char* fn = "smml_snn_stack_bwd_f32";
  SMML_REQUIRE(acts && dout && dz && dW && db, "%s: null pointer (dout, dW and db are host arrays, acts and dz device memory)", fn);
  SMML_REQUIRE(out || !final_relu, "%s: the outputs are needed for the mask of the final ReLU", fn);
  SnnArgs a;
  if (int rc = snn_fill(fn, a, x, x_row_stride, x_col_offset, W, widths, keep, G, depth, B, p, final_relu)) return rc;
  int nmax = 0;
  for (int g = 0; g < G; ++g) {
    SMML_REQUIRE(!final_relu || out[g] != 0, "%s: null output of network %d", fn, g);
    a.out[g] = out ? as_ptr<float>(out[g]) : nullptr;
    a.dout[g] = as_ptr<const float>(dout[g]);          // 0: no gradient arrived for this network
    a.dx[g] = dx ? as_ptr<float>(dx[g]) : nullptr;     // 0: not asked for
    for (int l = 0; l < depth; ++l) {
      SMML_REQUIRE(dW[g * depth + l] != 0 && db[g * depth + l] != 0, "%s: null dW or db of layer %d of network %d", fn, l, g);
      a.dW[g][l] = as_ptr<float>(dW[g * depth + l]);
      a.db[g][l] = as_ptr<float>(db[g * depth + l]);
      nmax = a.width[g][l + 1] > nmax ? a.width[g][l + 1] : nmax;
    }
  }
  a.acts = const_cast<float*>(acts);
  a.dz = dz;
  hipLaunchKernelGGL(snn_bwd_chain_kernel, dim3((unsigned)((B + SNN_ROWS - 1) / SNN_ROWS), (unsigned)G), dim3(SNN_BWD_THREADS), 0, (hipStream_t)stream, a);
  SMML_LAUNCH_CHECK(fn);
  hipLaunchKernelGGL(snn_bwd_weight_kernel, dim3((unsigned)((nmax + SNN_WROWS - 1) / SNN_WROWS), (unsigned)(G * depth)), dim3(SNN_BWD_THREADS), 0,
                     (hipStream_t)stream, a);
  SMML_LAUNCH_CHECK(fn);
  return SMML_OK;
}

}  // extern "C"
