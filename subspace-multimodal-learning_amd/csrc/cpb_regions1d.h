// Exact evaluation of the 1-D continuous position bias per LINEAR PIECE of its MLP (the 1-D sibling of cpb_regions.h).
//
// The bias MLP of the 1-D module (DeformableAttention1D.py:69-98: Linear(1, 32) - ReLU - Linear(32, 32) - ReLU - Linear(32, H/G) on the
// signed log p = sign(d) log(|d| + 1) of the offset) is a piecewise-affine function of ONE scalar: layer 1 kinks at p = -b1_i / w1_i (at
// most 32 points), and inside each of the <= 33 layer-1 intervals every layer-2 unit is affine in p, so it changes sign at most once.  The
// real line therefore splits into at most 32 + 33 * 32 = 1088 breakpoints and 1089 pieces on which the 64 ReLU decisions (D1, D2) are
// constant and  bias_o(p) = a_{r,o} p + c_{r,o}.  Per call:
//   build    (two small launches, fp64): the sorted breakpoints, the ReLU pattern and the (a, c) of every piece for every output, and a
//            uniform index grid over [-pmax, pmax]: first[c] = number of breakpoints whose (fp32) cell lies below c, so the piece of p lies
//            in [first[cell(p)], first[cell(p) + 1]] - a binary search over the breakpoints inside that cell (usually none or one).  Points
//            outside the grid search the breakpoints below / above it: exact everywhere, pmax is for speed only.
//   forward  per pair one signed log, the grid lookup, one LDS read of (a, c), 2 FMAs - instead of the per-pair MLP (7 MFMAs + ~150 vector
//            instructions per key and 32 queries); the piece id of every pair is saved (2 bytes, per head, the layout of the 2-D region ids).
//   backward per piece and output the two moments  d bias . (1, p)  in 64-bit fixed point (integer LDS adds: run-to-run identical); the six
//            parameter gradients are linear in them (a dense fp64 pass), and  d vs = - sum_heads d bias . a . slog'(d)  per pair.
// Decisions follow torch.relu's convention (x > 0 is active); a piece's pattern is the fp64 evaluation at a point inside it, so a pair's
// decisions can differ from an fp64 evaluation of the reference's formula only where p is within rounding of a breakpoint.
#pragma once
#include "cpb_regions.h"

namespace {

constexpr int R1_HPG = 2;                        // outputs of the MLP (heads per offset group) the path supports: 1 or 2
constexpr int R1_MAXBP = CH + (CH + 1) * CH;     // breakpoints: layer-1 kinks + one layer-2 zero per (layer-1 interval, unit)
constexpr int R1_MAXP = R1_MAXBP + 1;            // pieces
constexpr int R1_CELLS = 2048;                   // index grid cells over [-pmax, pmax]

struct Region1DHeader {                          // first 256 bytes of the table buffer
  unsigned n_bp, hpg, pad0, pad1;                // breakpoints (pieces = n_bp + 1), outputs
  float pmax, inv, off, pad2;                    // cell of p: floor(p * inv + off), clamped to [-1, R1_CELLS]
};
// fp64 copy of the parameters: w1 [32] at 0, b1 at 32, w2 [32][32] at 64, b2 at 1088, w3 [hpg][32] at 1120, b3 [hpg] at 1184
constexpr int W1D_W1 = 0, W1D_B1 = 32, W1D_W2 = 64, W1D_B2 = 1088, W1D_W3 = 1120, W1D_B3 = 1184, W1D_N = 1186;

struct Region1DLayout { size_t hdr, bp, pat, coef, first, bpd, wd, total; };
__host__ __device__ inline Region1DLayout region1d_layout() {
  Region1DLayout l;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  l.hdr = take(256);
  l.bp = take((size_t)R1_MAXBP * 4);             // sorted breakpoints, fp32 (what the attention kernels compare against)
  l.pat = take((size_t)R1_MAXP * 8);             // D1 | D2 << 32 per piece
  l.coef = take((size_t)R1_MAXP * 16);           // float4 {a_0, c_0, a_1, c_1} per piece
  l.first = take((size_t)(R1_CELLS + 1) * 2);    // u16 first piece per cell, cells 0 .. R1_CELLS
  l.bpd = take((size_t)R1_MAXBP * 8);            // sorted breakpoints, fp64
  l.wd = take((size_t)W1D_N * 8);
  l.total = o;
  return l;
}
struct Region1DTables {
  Region1DHeader* hdr; float* bp; unsigned long long* pat; float4* coef; unsigned short* first; double* bpd; double* wd;
};
inline Region1DTables region1d_tables(void* base) {
  const Region1DLayout l = region1d_layout();
  char* b = reinterpret_cast<char*>(base);
  return Region1DTables{reinterpret_cast<Region1DHeader*>(b + l.hdr), reinterpret_cast<float*>(b + l.bp),
                        reinterpret_cast<unsigned long long*>(b + l.pat), reinterpret_cast<float4*>(b + l.coef),
                        reinterpret_cast<unsigned short*>(b + l.first), reinterpret_cast<double*>(b + l.bpd),
                        reinterpret_cast<double*>(b + l.wd)};
}

// cell of p in the index grid, -1 below it, R1_CELLS above it (monotone in p: the build and the lookups use this same fp32 function)
__device__ __forceinline__ int r1_cell(float p, float inv, float off) {
  const int ci = (int)floorf(fminf(fmaxf(fmaf(p, inv, off), -1.f), (float)R1_CELLS));
  return min(max(ci, -1), R1_CELLS);
}
// piece of p = number of breakpoints < p.  Every breakpoint of a lower cell is < p, none of a higher cell is: the count lies in
// [first[c], first[c + 1]] (below the grid [0, first[0]], above it [first[R1_CELLS], n_bp]) - a binary search over that range.
__device__ __forceinline__ unsigned r1_lookup(const float* bp, const unsigned short* first, int nbp, float p, float inv, float off) {
  const int ci = r1_cell(p, inv, off);
  int lo = ci < 0 ? 0 : (int)first[ci];
  int hi = ci >= R1_CELLS ? nbp : (int)first[ci + 1];
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (bp[mid] < p) lo = mid + 1; else hi = mid;
  }
  return (unsigned)lo;
}

// a point strictly inside piece r of the sorted breakpoints bpd[0 .. n)
__device__ __forceinline__ double r1_inside(const double* bpd, int n, int r) {
  if (n == 0) return 0.0;
  if (r == 0) return bpd[0] - fmax(1.0, fabs(bpd[0]));
  if (r == n) return bpd[n - 1] + fmax(1.0, fabs(bpd[n - 1]));
  return 0.5 * (bpd[r - 1] + bpd[r]);
}

// build, launch 1 (one workgroup): parameters in fp64, the layer-1 kinks, the layer-2 zeros inside every layer-1 interval, all of them
// sorted (rank sort: the result does not depend on the order threads run in)
__global__ __launch_bounds__(256) void region1d_sort_kernel(CpbParams cp, int hpg, float pmax, Region1DTables t) {
  __shared__ double w[W1D_N];
  __shared__ double ks[CH + 1];
  __shared__ double cand[R1_MAXBP];
  __shared__ int nk;
  const int tid = threadIdx.x;
  for (int i = tid; i < W1D_N; i += 256) {
    double v = 0.0;
    if (i < W1D_B1) v = cp.w1[i];
    else if (i < W1D_W2) v = cp.b1[i - W1D_B1];
    else if (i < W1D_B2) v = cp.w2[i - W1D_W2];
    else if (i < W1D_W3) v = cp.b2[i - W1D_B2];
    else if (i < W1D_B3) v = (i - W1D_W3 < hpg * CH) ? cp.w3[i - W1D_W3] : 0.0;
    else v = (i - W1D_B3 < hpg) ? cp.b3[i - W1D_B3] : 0.0;
    w[i] = v;
    t.wd[i] = v;
  }
  __syncthreads();
  // layer-1 kinks (units with w1 = 0 are constant: no kink), sorted; +inf marks none (also for non-finite parameters)
  if (tid < CH) {
    const double wi = w[W1D_W1 + tid];
    double k = wi != 0.0 ? -w[W1D_B1 + tid] / wi : INFINITY;
    if (!(fabs(k) < INFINITY)) k = INFINITY;
    cand[tid] = k;
  }
  __syncthreads();
  if (tid < CH) {
    const double k = cand[tid];
    int rank = 0;
    for (int j = 0; j < CH; ++j) rank += (cand[j] < k || (cand[j] == k && j < tid)) ? 1 : 0;
    ks[rank] = k;
  }
  if (tid == 0) {
    int n = 0;
    for (int j = 0; j < CH; ++j) n += cand[j] < INFINITY ? 1 : 0;
    nk = n;
  }
  __syncthreads();
  // layer 2 inside interval it = (ks[it - 1], ks[it]) of layer 1: x2_o = alpha p + beta with the interval's layer-1 decisions
  const int m = nk;
  for (int s = tid; s < (CH + 1) * CH; s += 256) {
    const int it = s / CH, o = s - it * CH;
    double z = INFINITY;
    if (it <= m) {
      const double lo = it == 0 ? -INFINITY : ks[it - 1], hi = it == m ? INFINITY : ks[it];
      const double x = it == 0 ? (m ? ks[0] - fmax(1.0, fabs(ks[0])) : 0.0) : (it == m ? ks[m - 1] + fmax(1.0, fabs(ks[m - 1])) : 0.5 * (lo + hi));
      double al = 0.0, be = w[W1D_B2 + o];
      for (int i = 0; i < CH; ++i)
        if (fma(w[W1D_W1 + i], x, w[W1D_B1 + i]) > 0.0) {
          const double w2 = w[W1D_W2 + o * CH + i];
          al = fma(w2, w[W1D_W1 + i], al); be = fma(w2, w[W1D_B1 + i], be);
        }
      if (lo < hi && al != 0.0) {
        const double zz = -be / al;
        if (zz > lo && zz < hi) z = zz;
      }
    }
    cand[CH + s] = z;                                   // (cand[0 .. CH) keep the layer-1 kinks)
  }
  __syncthreads();
  int nfin = 0;
  for (int s = tid; s < R1_MAXBP; s += 256) {
    const double v = cand[s];
    if (!(v < INFINITY)) continue;
    int rank = 0;
    for (int j = 0; j < R1_MAXBP; ++j) rank += (cand[j] < v || (cand[j] == v && j < s)) ? 1 : 0;
    t.bpd[rank] = v;
    t.bp[rank] = (float)v;
    ++nfin;
  }
  // count of the finite candidates (= breakpoints): a fixed-order sum over the threads
  __shared__ int cnt[256];
  cnt[tid] = nfin;
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int j = 0; j < 256; ++j) n += cnt[j];
    double pm = pmax;
    if (!(pm > 0.0)) pm = n ? fmin(fmax(fmax(fabs(t.bpd[0]), fabs(t.bpd[n - 1])), 1.0), 16.0) : 1.0;
    Region1DHeader h;
    h.n_bp = (unsigned)n; h.hpg = (unsigned)hpg; h.pad0 = h.pad1 = 0u;
    h.pmax = (float)pm; h.inv = (float)((double)R1_CELLS / (2.0 * pm)); h.off = (float)(R1_CELLS / 2); h.pad2 = 0.f;
    *t.hdr = h;
  }
}

// build, launch 2: per piece its ReLU pattern (fp64 evaluation at a point inside it) and (a, c) per output; the index grid
//   c1_i = d1_i sum_o W2[o][i] w3[oo][o] d2_o;  a = sum_i c1_i w1_i;  c = sum_i c1_i b1_i + sum_o d2_o w3[oo][o] b2_o + b3[oo]
__global__ __launch_bounds__(64) void region1d_pieces_kernel(Region1DTables t) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  const double* __restrict__ wd = t.wd;
  const int n = min((int)t.hdr->n_bp, R1_MAXBP), hpg = min((int)t.hdr->hpg, R1_HPG);
  if (i <= n && i < R1_MAXP) {
    const double x = r1_inside(t.bpd, n, i);
    double h1[CH];
    unsigned d1 = 0u, d2 = 0u;
#pragma unroll
    for (int u = 0; u < CH; ++u) {
      const double x1 = fma(wd[W1D_W1 + u], x, wd[W1D_B1 + u]);
      d1 |= x1 > 0.0 ? (1u << u) : 0u;
      h1[u] = x1 > 0.0 ? x1 : 0.0;
    }
    for (int o = 0; o < CH; ++o) {
      double x2 = wd[W1D_B2 + o];
#pragma unroll
      for (int u = 0; u < CH; ++u) x2 = fma(wd[W1D_W2 + o * CH + u], h1[u], x2);
      d2 |= x2 > 0.0 ? (1u << o) : 0u;
    }
    t.pat[i] = (unsigned long long)d1 | ((unsigned long long)d2 << 32);
    float ac[4] = {0.f, 0.f, 0.f, 0.f};
    for (int oo = 0; oo < hpg; ++oo) {
      double a = 0.0, c = wd[W1D_B3 + oo];
      for (int o = 0; o < CH; ++o)
        if ((d2 >> o) & 1u) c = fma(wd[W1D_W3 + oo * CH + o], wd[W1D_B2 + o], c);
      for (int u = 0; u < CH; ++u) {
        if (!((d1 >> u) & 1u)) continue;
        double c1 = 0.0;
        for (int o = 0; o < CH; ++o)
          if ((d2 >> o) & 1u) c1 = fma(wd[W1D_W2 + o * CH + u], wd[W1D_W3 + oo * CH + o], c1);
        a = fma(c1, wd[W1D_W1 + u], a);
        c = fma(c1, wd[W1D_B1 + u], c);
      }
      ac[2 * oo] = (float)a; ac[2 * oo + 1] = (float)c;
    }
    t.coef[i] = make_float4(ac[0], ac[1], ac[2], ac[3]);
  }
  // first[c] = #{k : cell(bp[k]) < c}: the cells of the sorted breakpoints are non-decreasing - a binary search
  if (i <= R1_CELLS) {
    const float inv = t.hdr->inv, off = t.hdr->off;
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (r1_cell(t.bp[mid], inv, off) < i) lo = mid + 1; else hi = mid;
    }
    t.first[i] = (unsigned short)lo;
  }
}

static void region1d_build_launch(CpbParams cp, int hpg, float pmax, void* tables, hipStream_t st) {
  const Region1DTables t = region1d_tables(tables);
  hipLaunchKernelGGL(region1d_sort_kernel, dim3(1), dim3(256), 0, st, cp, hpg, pmax, t);
  constexpr int n = (R1_CELLS + 1) > R1_MAXP ? (R1_CELLS + 1) : R1_MAXP;
  hipLaunchKernelGGL(region1d_pieces_kernel, dim3((n + 63) / 64), dim3(64), 0, st, t);
}

struct Region1DView { const Region1DHeader* hdr; const float* bp; const float4* coef; const unsigned short* first; };
inline Region1DView region1d_view(const void* base) {
  const Region1DTables t = region1d_tables(const_cast<void*>(base));
  return Region1DView{t.hdr, t.bp, t.coef, t.first};
}

// ------------------------------------------------------------------------------------------------
// forward, 1-D positions, signed-log offsets, fp32-grade core, H / G in {1, 2}
// ------------------------------------------------------------------------------------------------
// The fused forward of deform_region_fwd_kernel<SAVE, float> (one wave = 32 queries on the MFMA lane axis, S^T = K . Q^T and
// O^T += V^T . P^T as fp16 hi / lo split products, online softmax, the same counter-based dropout with the keep decision stashed in the
// saved score) with the bias of head h = output h % (H / G) of its group's MLP looked up per pair in LDS.
template <bool SAVE>
__global__ __launch_bounds__(256, 2) void deform_region1d_fwd_kernel(
    const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V, const float* __restrict__ VS,
    const float* __restrict__ GQ, Region1DView rv, float* __restrict__ O, float* __restrict__ LSE, float* __restrict__ LT,
    unsigned short* __restrict__ RID, int N, int J, int H, int G, int NST, float scale, DropCfg dc_in) {
  const DropCfg dc = drop_resolve(dc_in);
  __shared__ __attribute__((aligned(16))) _Float16 Kp[2][KT * FRLD];
  __shared__ __attribute__((aligned(16))) _Float16 Vp[2][KT * FTLD];
  __shared__ float2 coefl[R1_MAXP];                                         // (a, c) of this head's output per piece
  __shared__ float bpl[R1_MAXBP];
  __shared__ unsigned short firstl[R1_CELLS + 1];
  __shared__ float vsl[2][KT];
  __shared__ __attribute__((aligned(16))) unsigned short ridl[WAVES][KT][QT + 8];

  const int tid = threadIdx.x, lane = tid & 63, c = lane & 31, hf = lane >> 5;
  const int wave = tid >> 6;
  const int b = blockIdx.z, h = blockIdx.y;
  const int hpg = H / G, g = h / hpg, oi = h - g * hpg;
  const int q0 = blockIdx.x * (QT * WAVES) + wave * QT;
  const int HD = H * DH;
  const bool qvalid = (q0 + c) < N;
  const int qi = qvalid ? (q0 + c) : (N - 1);
  const float* VSb = VS + (size_t)(b * G + g) * J;
  const int nbp = min((int)rv.hdr->n_bp, R1_MAXBP);
  {
    for (int i = tid; i <= nbp; i += 256) { const float4 r = rv.coef[i]; coefl[i] = oi ? make_float2(r.z, r.w) : make_float2(r.x, r.y); }
    for (int i = tid; i < nbp; i += 256) bpl[i] = rv.bp[i];
    for (int i = tid; i <= R1_CELLS; i += 256) firstl[i] = rv.first[i];
    if (tid < KT) vsl[0][tid] = VSb[min(tid, J - 1)];
  }
  __syncthreads();
  const float inv = rv.hdr->inv, off = rv.hdr->off;

  half8 qh[4], ql[4];
  {
    const float* qp = Q + ((size_t)b * N + qi) * HD + h * DH + hf * 8;
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const float4 t0 = *reinterpret_cast<const float4*>(qp + 16 * st), t1 = *reinterpret_cast<const float4*>(qp + 16 * st + 4);
      const float x8[8] = {t0.x * scale, t0.y * scale, t0.z * scale, t0.w * scale, t1.x * scale, t1.y * scale, t1.z * scale, t1.w * scale};
      split8(x8, qh[st], ql[st]);
    }
  }
  const int trq = (lane & 15) >> 2, trc = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  const float gq0 = GQ[qi];

  floatx16 oacc0 = {0}, oacc1 = {0};
  float m_run = -INFINITY, l_run = 0.f;
  const unsigned long long drop_row = dc.seed + ((unsigned long long)(b * H + h) * N + qi) * ((J + 1) >> 1);
  const float* Kb = K + (size_t)b * J * HD + h * DH;
  const float* Vb = V + (size_t)b * J * HD + h * DH;
  float* LTb = LT ? LT + ((size_t)(b * H + h) * NST + q0) * J : nullptr;
  unsigned short* RIDb = RID ? RID + ((size_t)(b * H + h) * NST + q0) * J : nullptr;

  float4 kreg[2], vreg[2];
  float vsn = 0.f;
  auto fetch_kv = [&](int jn) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = jn + (tid >> 4) + 16 * i, d4 = (tid & 15) * 4;
      kreg[i] = make_float4(0.f, 0.f, 0.f, 0.f); vreg[i] = kreg[i];
      if (key < J) {
        kreg[i] = *reinterpret_cast<const float4*>(Kb + (size_t)key * HD + d4);
        vreg[i] = *reinterpret_cast<const float4*>(Vb + (size_t)key * HD + d4);
      }
    }
    if (tid < KT) vsn = VSb[min(jn + KT + tid, J - 1)];
  };
  fetch_kv(0);
  const int ntiles = (J + KT - 1) / KT;
  for (int kt = 0; kt < ntiles; ++kt) {
    const int j0 = kt * KT;
    lds_barrier();                                   // every wave is done with the previous tile's K / V images
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = (tid >> 4) + 16 * i, d4 = (tid & 15) * 4;
      uint2v hi, lo;
      split4_h2(kreg[i], hi, lo);
      *reinterpret_cast<uint2v*>(&Kp[0][key * FRLD + d4]) = hi; *reinterpret_cast<uint2v*>(&Kp[1][key * FRLD + d4]) = lo;
      split4_h2(vreg[i], hi, lo);
      *reinterpret_cast<uint2v*>(&Vp[0][key * FTLD + d4]) = hi; *reinterpret_cast<uint2v*>(&Vp[1][key * FTLD + d4]) = lo;
    }
    if (tid < KT) vsl[(kt + 1) & 1][tid] = vsn;      // the NEXT tile's sample positions
    lds_barrier();
    if (kt + 1 < ntiles) fetch_kv(j0 + KT);          // in flight during this tile's products, lookups and softmax

    floatx16 s = {0};
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int o = c * FRLD + 16 * st + 8 * hf;
      const half8 kh = *reinterpret_cast<const half8*>(&Kp[0][o]), kl = *reinterpret_cast<const half8*>(&Kp[1][o]);
      s = mfma16(kl, qh[st], s);
      s = mfma16(kh, ql[st], s);
      s = mfma16(kh, qh[st], s);
    }
    const int nk = min(KT, J - j0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = acc_row(r, hf);
      const float p = slog1p(gq0 - vsl[kt & 1][key]);
      const unsigned id = r1_lookup(bpl, firstl, nbp, p, inv, off);
      const float2 ac = coefl[id];
      s[r] += fmaf(ac.x, p, ac.y);
      if (SAVE) ridl[wave][key][c] = (unsigned short)id;
    }
    if (SAVE) {
      // the tile's piece ids leave as whole rows: [key][32 queries] is 64 bytes per key (two 16-byte stores per lane)
      wave_lds_fence();
      const int key = lane >> 1, qh16 = (lane & 1) * 16;
      const uint4 w0 = *reinterpret_cast<const uint4*>(&ridl[wave][key][qh16]), w1 = *reinterpret_cast<const uint4*>(&ridl[wave][key][qh16 + 8]);
      if (key < nk) {
        uint4* dst = reinterpret_cast<uint4*>(RIDb + (size_t)(j0 + key) * 32 + qh16);
        dst[0] = w0;
        dst[1] = w1;
      }
      wave_lds_fence();
    }
    if (nk < KT) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] = acc_row(r, hf) < nk ? s[r] : -INFINITY;
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, s[r]);
    unsigned keepbits = 0xFFFFu;
    if (dc.thresh) {
      unsigned long long z0 = drop_row + (unsigned)((j0 >> 1) + 2 * hf);
      asm volatile("" : "+v"(z0));
      keepbits = 0u;
#pragma unroll
      for (int r = 0; r < 16; r += 2) keepbits |= drop_keep2_z(dc, z0 + (unsigned)(acc_row(r, 0) >> 1)) << r;
    }
    if constexpr (SAVE) {
      if (dc.thresh) {
        tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (nk == KT || acc_row(r, hf) < nk) s[r] = stash_keep_trunc(s[r], (keepbits >> r) & 1u);
          tmax = fmaxf(tmax, s[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = acc_row(r, hf);
        if (key < nk) LTb[(size_t)(j0 + key) * 32 + c] = s[r];
      }
    }
    tmax = xhalf_max(tmax);
    const float m_new = fmaxf(m_run, tmax);
    const float alpha = sexp(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = sexp(s[r] - m_new);
      psum += p;
      s[r] = p;
    }
    if (dc.thresh) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] *= ((keepbits >> r) & 1u) ? dc.keep_scale : 0.f;
    }
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) { oacc0[r] *= alpha; oacc1[r] *= alpha; }
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      float p8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) p8[j] = s[8 * kb + j];
      const int ro = (16 * kb + 4 * hf + trq) * FTLD + trc;
      half8 ph, pl;
      split8(p8, ph, pl);
      const half8 vh0 = lds_frag_tr_h(&Vp[0][ro], &Vp[0][ro + 8 * FTLD]), vl0 = lds_frag_tr_h(&Vp[1][ro], &Vp[1][ro + 8 * FTLD]);
      const half8 vh1 = lds_frag_tr_h(&Vp[0][ro + 32], &Vp[0][ro + 32 + 8 * FTLD]), vl1 = lds_frag_tr_h(&Vp[1][ro + 32], &Vp[1][ro + 32 + 8 * FTLD]);
      oacc0 = mfma16(vl0, ph, oacc0); oacc0 = mfma16(vh0, pl, oacc0); oacc0 = mfma16(vh0, ph, oacc0);
      oacc1 = mfma16(vl1, ph, oacc1); oacc1 = mfma16(vh1, pl, oacc1); oacc1 = mfma16(vh1, ph, oacc1);
    }
  }

  l_run = xhalf_sum(l_run);
  const float rinv = 1.f / l_run;
  if (qvalid) {
    float* op = O + ((size_t)b * N + qi) * HD + h * DH;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int d = 8 * rg + 4 * hf;
      *reinterpret_cast<float4*>(op + d) = make_float4(oacc0[4 * rg] * rinv, oacc0[4 * rg + 1] * rinv, oacc0[4 * rg + 2] * rinv, oacc0[4 * rg + 3] * rinv);
      *reinterpret_cast<float4*>(op + 32 + d) = make_float4(oacc1[4 * rg] * rinv, oacc1[4 * rg + 1] * rinv, oacc1[4 * rg + 2] * rinv, oacc1[4 * rg + 3] * rinv);
    }
    if (hf == 0) LSE[(size_t)(b * H + h) * N + qi] = m_run + logf(l_run);
  }
}

// ------------------------------------------------------------------------------------------------
// backward of the 1-D position bias per piece: d vs per pair, piece moments of d bias in 64-bit fixed point
// ------------------------------------------------------------------------------------------------
// grid (chunks * key groups, H, B), block 64 * nkbg * wpk (the plan of region_bwd_plan, shared with the 2-D kernel): lane = key (keys of
// a wave are nkb apart), each wave walks every wpk-th 32-query tile of its chunk; per tile a lane reads its key's 32 d scores and 32 piece
// ids (one 128-byte and one 64-byte row; the next tile's rows in flight).  The two moments of a RUN of queries in the same piece and the
// run's d vs sum stay in fp32 registers; a run ends when the piece changes AND at the end of every tile, so it holds at most 32 pairs and
// |run sum . S| <= 32 . 4 amax . 2^(kbits - e) <= 2^45 stays inside the exact range (2^51) of region_fix.  (In 1-D a key keeps its piece
// while the queries advance, so without the tile bound runs would be as long as the chunk.)  Non-finite d scores raise a flag that
// turns the parameter gradients into NaN (fixed point has no NaN).
struct Region1DBwdLds {
  unsigned long long hist[R1_MAXP * 2];
  float slope[R1_MAXP];
  float dvs[16][64];
};
__global__ __launch_bounds__(768) void cpb_region1d_bwd_kernel(
    const float* __restrict__ dLT, const unsigned short* __restrict__ RID, const float* __restrict__ VS, const float* __restrict__ GQ,
    Region1DView rv, const unsigned* __restrict__ AMAX, unsigned* __restrict__ FLAG, unsigned long long* __restrict__ HIST,
    float* __restrict__ dvs_slab, int N, int J, int H, int G, int NST, int nkb, int nkbg, int chunks, int wpk, int tiles_per_chunk, int kbits,
    int shift) {
  __shared__ __attribute__((aligned(16))) Region1DBwdLds L;
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 31;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.z, h = blockIdx.y, chunk = blockIdx.x % chunks, grp = blockIdx.x / chunks;
  const int hpg = H / G, g = h / hpg, oi = h - g * hpg;
  const int nthreads = blockDim.x;
  const int npc = min((int)rv.hdr->n_bp, R1_MAXBP) + 1;
  for (int i = tid; i < R1_MAXP * 2; i += nthreads) L.hist[i] = 0ull;
  for (int i = tid; i < npc; i += nthreads) { const float4 r = rv.coef[i]; L.slope[i] = oi ? r.z : r.x; }
  __syncthreads();
  const RegionScale sc = region_scale(*AMAX, kbits);
  float big;
  asm("s_mov_b32 %0, 0x71800000" : "=s"(big));

  const int kb = grp * nkbg + __builtin_amdgcn_readfirstlane(wave % nkbg), tslot = __builtin_amdgcn_readfirstlane(wave / nkbg);
  const int key = lane * nkb + kb;
  const bool kvalid = key < J && kb < nkb;
  const int keyc = min(key, J - 1);
  const float vsk = VS[(size_t)(b * G + g) * J + keyc];
  const int ntq = (N + QT - 1) / QT;
  const int t_begin = chunk * tiles_per_chunk, t_end = min(t_begin + tiles_per_chunk, ntq);
  float dv = 0.f;
  unsigned bad = 0u;
  unsigned cur = ~0u;
  float r0 = 0.f, r1 = 0.f, u = 0.f;
  typedef __attribute__((address_space(3))) unsigned long long lds_u64;
  lds_u64* const hist_l = (lds_u64*)L.hist;
  auto flush = [&]() {
    if (cur < (unsigned)npc) {
      dv = fmaf(-L.slope[cur], u, dv);
      lds_u64* hp = hist_l + cur * 2;
      __hip_atomic_fetch_add(hp, (unsigned long long)region_fix(r0, sc.S), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(hp + 1, (unsigned long long)region_fix(r1, sc.S), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    cur = ~0u;
    r0 = 0.f; r1 = 0.f; u = 0.f;
  };

  float4 dbn[8];
  uint4 ridn[4];
  float gqn;
  auto fetch = [&](int tile) {
    const size_t row = ((size_t)(b * H + h) * NST + (size_t)tile * QT) * J + (size_t)keyc * 32;
    const float4* dp = reinterpret_cast<const float4*>(dLT + row);
    const uint4* rp = reinterpret_cast<const uint4*>(RID + row);
#pragma unroll
    for (int i = 0; i < 8; ++i) dbn[i] = dp[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) ridn[i] = rp[i];
    gqn = GQ[min(tile * QT + c, N - 1)];
  };
  if (t_begin + tslot < t_end) fetch(t_begin + tslot);
  for (int tile = t_begin + tslot; tile < t_end; tile += wpk) {
    const int q0 = __builtin_amdgcn_readfirstlane(tile) * QT;
    const int nq = min(QT, N - q0);
    float dbr[32];
    unsigned ridw[16];
#pragma unroll
    for (int i = 0; i < 8; ++i) { dbr[4 * i] = dbn[i].x; dbr[4 * i + 1] = dbn[i].y; dbr[4 * i + 2] = dbn[i].z; dbr[4 * i + 3] = dbn[i].w; }
#pragma unroll
    for (int i = 0; i < 4; ++i) { ridw[4 * i] = ridn[i].x; ridw[4 * i + 1] = ridn[i].y; ridw[4 * i + 2] = ridn[i].z; ridw[4 * i + 3] = ridn[i].w; }
    const int gqb = __float_as_int(gqn);
    if (tile + wpk < t_end) fetch(tile + wpk);
    if (kvalid) {
#pragma unroll
      for (int q = 0; q < 32; ++q) {
        if (q < nq) {
          const float d = __int_as_float(__builtin_amdgcn_readlane(gqb, q)) - vsk;
          const float p = slog1p(d), sp = dpos_of<false>(d, big);
          const unsigned id = (ridw[q >> 1] >> (16 * (q & 1))) & 0xFFFFu;
          const float dbv = dbr[q];
          unsigned ub = __float_as_uint(dbv);
          asm("" : "+v"(ub));                                       // (opaque: this file is built with -fno-honor-nans)
          bad |= ((ub & 0x7F800000u) == 0x7F800000u) ? 1u : 0u;
          if (id != cur) { flush(); cur = id; }
          r0 += dbv; r1 = fmaf(dbv, p, r1); u = fmaf(dbv, sp, u);
        }
      }
      flush();                                                      // runs end with the tile (bounded length, see above)
    }
  }
  if (__ballot(bad != 0u) && lane == 0) atomicOr(FLAG, 1u);
  L.dvs[wave][lane] = dv;
  __syncthreads();
  if (wave < nkbg && kvalid) {
    float sum = L.dvs[wave][lane];
    for (int s2 = 1; s2 < wpk; ++s2) sum += L.dvs[wave + s2 * nkbg][lane];
    dvs_slab[((size_t)chunk * gridDim.z * gridDim.y + (size_t)(b * H + h)) * J + key] = sum;
  }
  // piece moments -> global accumulators [piece][output][2] (coarser scale: 2^-shift, rounded)
  const long long half = shift > 0 ? (1ll << (shift - 1)) : 0ll;
  for (int i = tid; i < npc * 2; i += nthreads) {
    const long long v = (long long)L.hist[i];
    if (v != 0ll) atomicAdd(&HIST[((size_t)(i >> 1) * R1_HPG + oi) * 2 + (i & 1)], (unsigned long long)((v + half) >> shift));
  }
}

// the 1-D geometry of the dense tail (region_final_launch, cpb_regions.h): two moments (1, p) per piece and output
struct Region1DGeo {
  typedef Region1DTables Tables;
  typedef float Pos;
  static constexpr int PD = 1, W1 = W1D_W1, B1 = W1D_B1, W2 = W1D_W2, B2 = W1D_B2, GROUPS = (R1_MAXP + RG_FIN - 1) / RG_FIN;
  static constexpr bool DIRECT = false;
  __device__ static int w3(int o) { return W1D_W3 + o * CH; }
  __device__ static int count(const Tables& t) { return min((int)t.hdr->n_bp, R1_MAXBP) + 1; }
  __device__ static double moment(const unsigned long long* HIST, int o, int r, int m) {       // [piece][R1_HPG][2]
    return (double)(long long)HIST[((size_t)r * R1_HPG + o) * 2 + m];
  }
  __device__ static double x1(const double* wd, int i, const double* M) { return fma(wd[W1 + i], M[1], wd[B1 + i] * M[0]); }
};
static_assert(R1_HPG == RG_HPG && RegionSlab<Region1DGeo, R1_HPG>::STRIDE == RG_GRAD && Region1DGeo::GROUPS <= Region2DGeo::GROUPS,
              "the 1-D backward runs in the workspace of region_bwd_plan");

// pass 3 of a piece backward: d vs per pair and piece moments (cpb_region1d_bwd_kernel), then the dense pass to the six parameter gradients.
// wsb: the call's workspace (bytes), pl: its plan (region_bwd_plan); amax | flag | hist | grad were zeroed and amax filled by the dq pass.
static int region1d_bias_bwd_launch(const char* fn, const float* dlogits, const unsigned short* region_ids, const float* vs, const float* gq,
                                    const void* tables, char* wsb, const RegionBwdPlan& pl, int B, int N, int J, int H, int G, int nst, float* dvs,
                                    float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, void* ev_start, void* ev_stop,
                                    hipStream_t st) {
  unsigned* amax = reinterpret_cast<unsigned*>(wsb + pl.amax);
  unsigned* flag = amax + 1;                                 // non-finite d score seen (same zeroed 256-byte block)
  unsigned long long* hist = reinterpret_cast<unsigned long long*>(wsb + pl.hist);
  float* dvs_slab = reinterpret_cast<float*>(wsb + pl.dvs);
  const Region1DView rv = region1d_view(tables);
  if (ev_start) (void)hipEventRecord((hipEvent_t)ev_start, st);
  hipLaunchKernelGGL(cpb_region1d_bwd_kernel, dim3(pl.chunks * pl.ngrp, H, B), dim3(64 * pl.nkbg * pl.wpk), 0, st, dlogits, region_ids, vs, gq, rv,
                     amax, flag, hist, dvs_slab, N, J, H, G, nst, pl.nkb, pl.nkbg, pl.chunks, pl.wpk, pl.tiles_per_chunk, pl.kbits, pl.shift);
  if (ev_stop) (void)hipEventRecord((hipEvent_t)ev_stop, st);
  if (int rc = launch_check(fn, "cpb")) return rc;
  region_final_launch<Region1DGeo>(region1d_tables(const_cast<void*>(tables)), wsb, pl, B, J, H, G, dvs, dw1, db1, dw2, db2, dw3, db3, st);
  return launch_check(fn, "reduce");
}

}  // namespace
