// Attention maps of the fused deformable cross-attention from what its forward saved (include/smml.h, smml_attn_maps_f32): the
// probabilities P[b, h, i, j] = exp(score - lse) of softmax(scale q k^T + CPB(gq - vs)) BEFORE dropout
// (models/DeformableAttention2D.py:306-308, DeformableAttention1D.py:226-228), formed from the score tiles logits_t [B, H, nst / 32, J, 32]
// and lse [B, H, N] that every fp32-grade core writes - nothing of the forward is recomputed, the position-bias MLP in particular.
//   key_mass [B, H, J] = (1 / N) sum_i P[b, h, i, j]    the share of the bag's attention each sampled key receives
//   attn     [B, H, N, J]                               the probabilities themselves (optional: small bags and tests)
// One streaming pass over logits_t, 16 bytes per lane: a lane holds 4 consecutive queries of one key, 8 lanes one key of a 32-query tile, a
// wave 8 keys (1 KB contiguous), the 4 waves of a workgroup 32 keys (4 KB contiguous).  A workgroup owns a slice of AM_TILES query tiles of
// one (bag, head) and walks the keys; per key block every lane adds its probabilities over the slice's tiles in registers, the 8 lanes of a
// key combine, and the slice's column sums go to partial rows [B, H, slices, J] in the caller's workspace.  A second kernel adds the slices
// in ascending order: no float atomics, every sum in a fixed order - run-to-run identical results.
// Rows N .. nst - 1 of the last tiles are padding the forward never wrote: they have no lse and are masked out of the sums by a select
// (their bits may be anything, NaN included, so they are not multiplied by zero).
#include "smml_common.h"

namespace {

constexpr int AM_TILES = 8;                 // 32-query tiles per workgroup (256 queries): 8 independent 16-byte loads in flight per lane
constexpr int AM_WAVES = 4;
constexpr int AM_KEYS = 8 * AM_WAVES;       // keys per workgroup step
constexpr float AM_LOG2E = 1.4426950408889634f;
// the sizes the fused attention families accept (csrc/deform_common.h): every index below then stays inside 63 bits
constexpr int AM_MAX_QUERIES = 1 << 26, AM_MAX_KEYS = 1 << 22;

template <bool DENSE>
__global__ __launch_bounds__(64 * AM_WAVES) void attn_maps_kernel(const float* __restrict__ LT, const float* __restrict__ LSE,
                                                                  float* __restrict__ part, float* __restrict__ attn, int N, int J, int H,
                                                                  int NST, int nslices) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int kj = lane >> 3, cq = (lane & 7) * 4;          // this lane: key kj of the wave's 8, queries cq .. cq + 3 of a tile
  const int slice = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int nt = (N + 31) >> 5;                            // tiles with at least one live query
  const int t0 = slice * AM_TILES;
  const size_t bh = (size_t)b * H + h;

  // lse of this lane's 4 queries in each tile of the slice, and which of them exist (bit 4 i + e: tile i, query e)
  float ls[AM_TILES][4];
  unsigned live = 0u;
#pragma unroll
  for (int i = 0; i < AM_TILES; ++i) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = (t0 + i) * 32 + cq + e;
      const bool ok = (t0 + i) < nt && q < N;
      ls[i][e] = ok ? LSE[bh * N + q] : 0.f;
      live |= ok ? (1u << (4 * i + e)) : 0u;
    }
  }
  const float* LTb = LT + bh * (size_t)NST * J;            // tile t of this (bag, head): LTb + t * J * 32, element (key, query) at key * 32 + query
  size_t toff[AM_TILES];
#pragma unroll
  for (int i = 0; i < AM_TILES; ++i) toff[i] = (size_t)min(t0 + i, nt - 1) * J * 32 + cq;     // clamped: always in bounds, masked at use

  for (int j0 = wave * 8; j0 < J; j0 += AM_KEYS) {
    const int key = j0 + kj;
    const bool kok = key < J;
    const size_t koff = (size_t)min(key, J - 1) * 32;
    float4 v[AM_TILES];
#pragma unroll
    for (int i = 0; i < AM_TILES; ++i) v[i] = *reinterpret_cast<const float4*>(LTb + toff[i] + koff);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < AM_TILES; ++i) {
      const float x[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
      float p[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // exp(score - lse): the difference first (small where P is not), then one multiply into v_exp_f32's base
        const float pe = __builtin_amdgcn_exp2f((x[e] - ls[i][e]) * AM_LOG2E);
        p[e] = ((live >> (4 * i + e)) & 1u) ? pe : 0.f;
      }
      acc += (p[0] + p[1]) + (p[2] + p[3]);
      if (DENSE && kok) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int q = (t0 + i) * 32 + cq + e;
          if ((live >> (4 * i + e)) & 1u) attn[(bh * N + q) * J + key] = p[e];
        }
      }
    }
    // the 8 lanes of a key: a fixed butterfly
    acc += __shfl_xor(acc, 1);
    acc += __shfl_xor(acc, 2);
    acc += __shfl_xor(acc, 4);
    if (kok && (lane & 7) == 0) part[(bh * nslices + slice) * J + key] = acc;
  }
}

// key_mass[b, h, j] = (sum over the slices, ascending) / N
__global__ __launch_bounds__(256) void attn_maps_reduce_kernel(const float* __restrict__ part, float* __restrict__ key_mass, size_t BH, int J,
                                                               int nslices, float n) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= BH * J) return;
  const size_t bh = idx / J;
  const int j = (int)(idx - bh * J);
  const float* p = part + bh * nslices * J + j;
  float s = 0.f;
  for (int x = 0; x < nslices; ++x) s += p[(size_t)x * J];
  key_mass[idx] = s / n;
}

long long am_slices(int N) { return (((long long)N + 31) / 32 + AM_TILES - 1) / AM_TILES; }

}  // namespace

extern "C" {

// partial column sums [B, H, slices, J] fp32; saturates instead of wrapping
size_t smml_attn_maps_workspace_bytes(int B, int N, int J, int H) {
  if (B <= 0 || N <= 0 || J <= 0 || H <= 0) return 0;
  size_t n = (size_t)B;
  if (__builtin_mul_overflow(n, (size_t)H, &n) || __builtin_mul_overflow(n, (size_t)am_slices(N), &n) ||
      __builtin_mul_overflow(n, (size_t)J, &n) || __builtin_mul_overflow(n, sizeof(float), &n))
    return ~(size_t)0;
  return n;
}

int smml_attn_maps_f32(const float* logits_t, const float* lse, float* key_mass, float* attn, void* workspace, size_t workspace_bytes,
                       int B, int N, int J, int H, void* stream) {
  const char* fn = "smml_attn_maps_f32";
  SMML_REQUIRE(B > 0 && N > 0 && J > 0 && H > 0, "%s: non-positive dimension", fn);
  SMML_REQUIRE(B <= 65535 && H <= 65535 && N <= AM_MAX_QUERIES && J <= AM_MAX_KEYS, "%s: B, H <= 65535, N <= 2^26, J <= 2^22 (got B %d N %d J %d H %d)",
               fn, B, N, J, H);
  SMML_REQUIRE(logits_t && lse && key_mass && workspace, "%s: null pointer", fn);
  SMML_REQUIRE((reinterpret_cast<size_t>(logits_t) & 15) == 0 && (reinterpret_cast<size_t>(workspace) & 15) == 0,
               "%s: logits_t and workspace must be 16-byte aligned", fn);
  const size_t need = smml_attn_maps_workspace_bytes(B, N, J, H);
  SMML_REQUIRE(workspace_bytes >= need, "%s: workspace too small (%zu < %zu)", fn, workspace_bytes, need);
  const int nst = smml_deform_attn_nst(N);
  const int nslices = (int)am_slices(N);
  const size_t BH = (size_t)B * H;
  SMML_REQUIRE((BH * J + 255) / 256 <= 2147483647ULL, "%s: too many outputs", fn);
  hipStream_t st = (hipStream_t)stream;
  float* part = static_cast<float*>(workspace);
  const dim3 grid((unsigned)nslices, (unsigned)H, (unsigned)B), block(64 * AM_WAVES);
  if (attn)
    hipLaunchKernelGGL(attn_maps_kernel<true>, grid, block, 0, st, logits_t, lse, part, attn, N, J, H, nst, nslices);
  else
    hipLaunchKernelGGL(attn_maps_kernel<false>, grid, block, 0, st, logits_t, lse, part, attn, N, J, H, nst, nslices);
  SMML_LAUNCH_CHECK("smml_attn_maps_f32/maps");
  hipLaunchKernelGGL(attn_maps_reduce_kernel, dim3((unsigned)((BH * J + 255) / 256)), dim3(256), 0, st, part, key_mass, BH, J, nslices, (float)N);
  SMML_LAUNCH_CHECK("smml_attn_maps_f32/reduce");
  return SMML_OK;
}

}  // extern "C"
