// Wide position-bias family of the fp32-grade fused deformable cross-attention core (gfx950): bias-MLP hidden widths W = 64 and 128
// (dim = 256 / 512 of the modules; deform_attn.hip is built for W = 32).  MLP shape posdim -> W -> W -> heads // groups.
//
// Reference: models/DeformableAttention2D.py:120-157 (CPB), :284-312 (sim, bias, softmax, attn @ v); models/DeformableAttention1D.py:60-102.
//
// The bias is evaluated ONCE per (bag, offset group, query, key) by cpb_wide_bias_kernel into a tile buffer in the score-tile layout
// [B, H, nst / 32, J, 32]; deform_attn_biasmem_fwd_kernel is deform_attn_fwd_kernel (deform_attn.hip) with the bias read from that buffer
// (in training the buffer IS logits_t: every element is read and then overwritten by the lane that owns it).  The backward is the existing
// bwd_dq_dkv followed by cpb_wide_bwd_kernel, which recomputes the MLP.
//
// One evaluator (wide_eval) serves the bias kernel, the backward and the decision export, so the three take bit-identical ReLU decisions
// and no mask tensor is saved (2 W bits per pair would be 16 - 32 bytes):
//   layer 1   plain fp32 FMAs; lane (query c, half hf) evaluates the channels of parity hf: exactly the B operand of layer 2
//   layer 2   v_mfma_f32_32x32x2_f32 (exact fp32, a k-ordered fmaf chain): D[out][query] = b2 + sum_in W2[out][in] h1[in][query],
//             A = W2[out = 32 ot + c][in = 2 s + hf] from the transposed LDS image w2t[in][out] (rows of W + 1 floats: this read and the
//             backward's transposed read are both free of bank conflicts), B = h1[2 s + hf][c] from the lane's own registers:
//             (W / 32) (W / 2) MFMAs per key and 32 queries.
// Backward per key and wave (32 queries), all reductions over queries on the fp32 MFMA or by one lane per channel, then per-wave slabs that
// two small kernels add in a fixed order - no float atomics anywhere:
//   r2 = relu(D) and h1 are staged [channel][query] in LDS; one lane per channel forms g2 = [D > 0] (w3^T d bias) in place, d b2, d w3
//   d W2[out][in] += sum_q g2[out][q] h1[in][q]      A = g2[32 ot + c][q = 2 s + hf], B = h1[32 it + c][q = 2 s + hf]
//   d h1[in][q]    = sum_out W2[out][in] g2[out][q]  A = w2t[32 it + c][out = 2 s + hf], B = g2[2 s + hf][c]
//   g1 = [x1 > 0] d h1 (x1 recomputed by the evaluator's own layer-1 function), d vs per key; one lane per channel: d b1, d W1.
#include "deform_common.h"

namespace {

// LDS image of the MLP (floats): w2t[in][out] (rows of W + 1) | w1x[W] | w1y[W] | b1[W] | b2[W] | w3[2][W]
template <int W> struct WideLds {
  static constexpr int LD = W + 1;
  static constexpr int W1X = W * LD, W1Y = W1X + W, B1 = W1Y + W, B2 = B1 + W, W3 = B2 + W;
  static constexpr int PARAMS = W3 + 2 * W;
  static constexpr int STG = W * 33;                       // one [channel][32 queries] staging block, rows of 33 floats
  static constexpr int WAVE = 2 * STG + 128;               // backward, per wave: X | H1 | d bias[2][32] | pos[2][32]
  static constexpr int BWD_WAVES = (W == 64) ? 4 : 2;      // 88 KB / 138 KB of the 160 KB
  static constexpr int SLAB = W * W + 6 * W + 4;           // dW2 | dW1[W][2] | db1 | db2 | dW3[2][W] | db3[2] (+ pad)
};

template <int W, int PD>
__device__ __forceinline__ void wide_load_params(float* S, const CpbParams& cp, int o, int tid, int nthreads) {
  typedef WideLds<W> L;
  for (int i = tid; i < W * W; i += nthreads) {
    const int out = i / W, in = i - out * W;
    S[in * L::LD + out] = cp.w2[i];
  }
  for (int i = tid; i < W; i += nthreads) {
    S[L::W1X + i] = cp.w1[i * PD];
    S[L::W1Y + i] = (PD == 2) ? cp.w1[i * PD + 1] : 0.f;
    S[L::B1 + i] = cp.b1[i];
    S[L::B2 + i] = cp.b2[i];
    S[L::W3 + i] = cp.w3[i];
    S[L::W3 + W + i] = (o == 2) ? cp.w3[W + i] : 0.f;
  }
}

// layer-1 pre-activation of hidden channel ch: the ONE expression every kernel of the family evaluates it with
template <int W> __device__ __forceinline__ float wide_x1(const float* S, int ch, float p0, float p1) {
  typedef WideLds<W> L;
  return fmaf(S[L::W1X + ch], p0, fmaf(S[L::W1Y + ch], p1, S[L::B1 + ch]));
}

// Layers 1 and 2 for 32 queries (lane c, both halves) and one key.  x1[s]: pre-activation of hidden channel 2 s + hf;
// d[ot][r]: layer-2 pre-activation of output channel 32 ot + acc_row(r, hf) of query c.
template <int W>
__device__ __forceinline__ void wide_eval(const float* S, float p0, float p1, int c, int hf, float (&x1)[W / 2], floatx16 (&d)[W / 32]) {
  typedef WideLds<W> L;
#pragma unroll
  for (int s = 0; s < W / 2; ++s) x1[s] = wide_x1<W>(S, 2 * s + hf, p0, p1);
#pragma unroll
  for (int ot = 0; ot < W / 32; ++ot)
#pragma unroll
    for (int r = 0; r < 16; ++r) d[ot][r] = S[L::B2 + 32 * ot + acc_row(r, hf)];
#pragma unroll
  for (int s = 0; s < W / 2; ++s) {
    const float h = x1[s] > 0.f ? x1[s] : 0.f;
#pragma unroll
    for (int ot = 0; ot < W / 32; ++ot) d[ot] = mfma32(S[(2 * s + hf) * L::LD + 32 * ot + c], h, d[ot]);
  }
}

__device__ __forceinline__ unsigned xhalf_or(unsigned u) {
  auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return r[0] | r[1];
}

// ------------------------------------------------------------------------------------------------
// bias tiles: BT[B, H, NST / 32, J, 32] for the heads of group g = blockIdx.y
// ------------------------------------------------------------------------------------------------
template <int W, int PDX>
__global__ __launch_bounds__(256) void cpb_wide_bias_kernel(const float* __restrict__ VS, const float* __restrict__ GQ, CpbParams cp,
                                                            float* __restrict__ BT, int N, int J, int H, int G, int NST) {
  typedef WideLds<W> L;
  constexpr int PD = PosCfg<PDX>::PD;
  constexpr bool RAW = PosCfg<PDX>::RAW;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, hf = lane >> 5;
  const int b = blockIdx.z, g = blockIdx.y, o = H / G;
  const int q0 = blockIdx.x * (QT * WAVES) + wave * QT;     // < NST: rows of padded query lanes exist
  const int qi = min(q0 + c, N - 1);
  wide_load_params<W, PD>(smem, cp, o, tid, 256);
  __syncthreads();
  const float gq0 = GQ[(size_t)qi * PD];
  const float gq1 = (PD == 2) ? GQ[(size_t)qi * PD + 1] : 0.f;
  const float b30 = cp.b3[0], b31 = (o == 2) ? cp.b3[1] : 0.f;
  const float* VSb = VS + (size_t)(b * G + g) * J * PD;
  float* BT0 = BT + ((size_t)(b * H + g * o) * NST + q0) * J;          // this wave's [J][32] block of the group's first head
  float* BT1 = BT0 + (size_t)NST * J;                                  // ... of its second head (o == 2)
  for (int j = 0; j < J; ++j) {
    const float p0 = pos_of<RAW>(gq0 - VSb[(size_t)j * PD]);
    const float p1 = (PD == 2) ? slog1p(gq1 - VSb[(size_t)j * PD + 1]) : 0.f;
    float x1[W / 2];
    floatx16 d[W / 32];
    wide_eval<W>(smem, p0, p1, c, hf, x1, d);
    float t0 = 0.f, t1 = 0.f;
#pragma unroll
    for (int ot = 0; ot < W / 32; ++ot)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ch = 32 * ot + acc_row(r, hf);
        const float rl = d[ot][r] > 0.f ? d[ot][r] : 0.f;
        t0 = fmaf(rl, smem[L::W3 + ch], t0);
        t1 = fmaf(rl, smem[L::W3 + W + ch], t1);
      }
    t0 = xhalf_sum(t0) + b30;
    t1 = xhalf_sum(t1) + b31;
    if (hf == 0) {
      BT0[(size_t)j * 32 + c] = t0;
      if (o == 2) BT1[(size_t)j * 32 + c] = t1;
    }
  }
}

// Decision export (tests only): DM[(B G), N, J, 2, W / 32] uint32 - layer (0: [x1 > 0], 1: [D > 0]), channel ch at bit ch % 32 of word ch / 32
template <int W, int PDX>
__global__ __launch_bounds__(256) void cpb_wide_decisions_kernel(const float* __restrict__ VS, const float* __restrict__ GQ, CpbParams cp,
                                                                 unsigned* __restrict__ DM, int N, int J, int G) {
  constexpr int PD = PosCfg<PDX>::PD;
  constexpr bool RAW = PosCfg<PDX>::RAW;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, hf = lane >> 5;
  const int b = blockIdx.z, g = blockIdx.y;
  const int q0 = blockIdx.x * (QT * WAVES) + wave * QT;
  const bool qvalid = (q0 + c) < N;
  const int qi = qvalid ? (q0 + c) : (N - 1);
  wide_load_params<W, PD>(smem, cp, 1, tid, 256);
  __syncthreads();
  const float gq0 = GQ[(size_t)qi * PD];
  const float gq1 = (PD == 2) ? GQ[(size_t)qi * PD + 1] : 0.f;
  const float* VSb = VS + (size_t)(b * G + g) * J * PD;
  unsigned* DMq = DM + ((size_t)(b * G + g) * N + qi) * J * (2 * (W / 32));
  for (int j = 0; j < J; ++j) {
    const float p0 = pos_of<RAW>(gq0 - VSb[(size_t)j * PD]);
    const float p1 = (PD == 2) ? slog1p(gq1 - VSb[(size_t)j * PD + 1]) : 0.f;
    float x1[W / 2];
    floatx16 d[W / 32];
    wide_eval<W>(smem, p0, p1, c, hf, x1, d);
    unsigned m1[W / 32], m2[W / 32];
#pragma unroll
    for (int w = 0; w < W / 32; ++w) { m1[w] = 0u; m2[w] = 0u; }
#pragma unroll
    for (int s = 0; s < W / 2; ++s) {
      const int ch = 2 * s + hf;
      if (x1[s] > 0.f) m1[s / 16] |= 1u << (ch & 31);          // ch / 32 = s / 16
    }
#pragma unroll
    for (int ot = 0; ot < W / 32; ++ot)
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (d[ot][r] > 0.f) m2[ot] |= 1u << acc_row(r, hf);
#pragma unroll
    for (int w = 0; w < W / 32; ++w) { m1[w] = xhalf_or(m1[w]); m2[w] = xhalf_or(m2[w]); }
    if (hf == 0 && qvalid) {
#pragma unroll
      for (int w = 0; w < W / 32; ++w) {
        DMq[(size_t)j * (2 * (W / 32)) + w] = m1[w];
        DMq[(size_t)j * (2 * (W / 32)) + W / 32 + w] = m2[w];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------
// attention forward with the bias read from tiles: tile geometry and arithmetic of deform_attn_fwd_kernel (deform_attn.hip).
// BIAS and LT may be the same buffer (training): lane (c, hf) reads element (key, c) before it writes it, and no other lane touches it.
// ------------------------------------------------------------------------------------------------
template <bool SAVE>
__global__ __launch_bounds__(256, 2) void deform_attn_biasmem_fwd_kernel(
    const float* __restrict__ Q, const float* __restrict__ K, const float* __restrict__ V, const float* BIAS, float* __restrict__ O,
    float* __restrict__ LSE, float* LT, int N, int J, int H, int NST, float scale, DropCfg dc_in) {
  const DropCfg dc = drop_resolve(dc_in);
  __shared__ __attribute__((aligned(16))) _Float16 Kp[2][KT * FRLD];         // K tile, fp16 hi / lo planes, row image (A operand of S^T)
  __shared__ __attribute__((aligned(16))) _Float16 Vp[2][KT * FTLD];         // V tile, hi / lo planes, read transposed (A operand of O^T)
  __shared__ __attribute__((aligned(16))) _Float16 Qp[WAVES][2][QT * FRLD];  // per-wave scaled Q tile, hi / lo planes, row image

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, hf = lane >> 5;
  const int b = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * (QT * WAVES) + wave * QT;
  const int HD = H * DH;
  const bool qvalid = (q0 + c) < N;
  const int qi = qvalid ? (q0 + c) : (N - 1);
  {
    const float4* qp = reinterpret_cast<const float4*>(Q + ((size_t)b * N + qi) * HD + h * DH + hf * 32);
#pragma unroll
    for (int s4 = 0; s4 < 8; ++s4) {
      const float4 t = qp[s4];
      uint2v hi, lo;
      split4_h2(make_float4(t.x * scale, t.y * scale, t.z * scale, t.w * scale), hi, lo);
      *reinterpret_cast<uint2v*>(&Qp[wave][0][c * FRLD + 32 * hf + 4 * s4]) = hi;
      *reinterpret_cast<uint2v*>(&Qp[wave][1][c * FRLD + 32 * hf + 4 * s4]) = lo;
    }
  }
  const int trq = (lane & 15) >> 2, trc = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);      // transposed-read lane map

  floatx16 oacc0 = {0}, oacc1 = {0};
  float m_run = -INFINITY, l_run = 0.f;
  const float* Kb = K + (size_t)b * J * HD + h * DH;
  const float* Vb = V + (size_t)b * J * HD + h * DH;
  const float* Bb = BIAS + ((size_t)(b * H + h) * NST + q0) * J;             // this wave's [J][32] block
  float* LTb = SAVE ? LT + ((size_t)(b * H + h) * NST + q0) * J : nullptr;

  const int ntiles = (J + KT - 1) / KT;
  for (int kt = 0; kt < ntiles; ++kt) {
    const int j0 = kt * KT;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = (tid >> 4) + 16 * i, d4 = (tid & 15) * 4;
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (j0 + key < J) {
        kv = *reinterpret_cast<const float4*>(Kb + (size_t)(j0 + key) * HD + d4);
        vv = *reinterpret_cast<const float4*>(Vb + (size_t)(j0 + key) * HD + d4);
      }
      uint2v hi, lo;
      split4_h2(kv, hi, lo);
      *reinterpret_cast<uint2v*>(&Kp[0][key * FRLD + d4]) = hi; *reinterpret_cast<uint2v*>(&Kp[1][key * FRLD + d4]) = lo;
      split4_h2(vv, hi, lo);
      *reinterpret_cast<uint2v*>(&Vp[0][key * FTLD + d4]) = hi; *reinterpret_cast<uint2v*>(&Vp[1][key * FTLD + d4]) = lo;
    }
    __syncthreads();

    // S^T[key, query] = K . (scale Q)^T
    floatx16 s = {0};
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      const int o = c * FRLD + 16 * st + 8 * hf;
      const half8 kh = *reinterpret_cast<const half8*>(&Kp[0][o]), kl = *reinterpret_cast<const half8*>(&Kp[1][o]);
      const half8 qh = *reinterpret_cast<const half8*>(&Qp[wave][0][o]), ql = *reinterpret_cast<const half8*>(&Qp[wave][1][o]);
      s = mfma16(kl, qh, s);
      s = mfma16(kh, ql, s);
      s = mfma16(kh, qh, s);
    }
    const int nk = min(KT, J - j0);

    // bias add (from the tile buffer), key mask, online softmax
    float tmax = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = acc_row(r, hf);
      const float sv = (key < nk) ? s[r] + Bb[(size_t)(j0 + key) * 32 + c] : -INFINITY;
      s[r] = sv;
      tmax = fmaxf(tmax, sv);
    }
    unsigned keepbits = 0xFFFFu;              // dropout decisions of this lane's 16 keys (bit r)
    if (dc.thresh) {
      const unsigned long long base2 = ((unsigned long long)(b * H + h) * N + qi) * ((J + 1) >> 1) + (j0 >> 1);
      keepbits = 0u;
#pragma unroll
      for (int r = 0; r < 16; r += 2) keepbits |= drop_keep2(dc, base2 + (acc_row(r, hf) >> 1)) << r;     // registers r, r + 1: keys 2 jp, 2 jp + 1
    }
    if (SAVE) {                               // rows are padded to whole workgroup tiles: lanes past N write padding
      if (dc.thresh) {
        tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (acc_row(r, hf) < nk) s[r] = stash_keep(s[r], (keepbits >> r) & 1u);      // finite scores only
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
      psum += p;                                  // the normaliser sums the un-dropped probabilities
      s[r] = p;
    }
    if (dc.thresh) {                              // dropped / rescaled probabilities feed P.V only
#pragma unroll
      for (int r = 0; r < 16; ++r) s[r] *= ((keepbits >> r) & 1u) ? dc.keep_scale : 0.f;
    }
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) { oacc0[r] *= alpha; oacc1[r] *= alpha; }

    // O^T[d, query] += V^T . P^T   (accumulator registers of P^T are the B operand as they stand)
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
      float p8[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) p8[j] = s[8 * kb + j];
      half8 ph, pl;
      split8(p8, ph, pl);
      const int ro = (16 * kb + 4 * hf + trq) * FTLD + trc;
      const half8 vh0 = lds_frag_tr_h(&Vp[0][ro], &Vp[0][ro + 8 * FTLD]), vl0 = lds_frag_tr_h(&Vp[1][ro], &Vp[1][ro + 8 * FTLD]);
      const half8 vh1 = lds_frag_tr_h(&Vp[0][ro + 32], &Vp[0][ro + 32 + 8 * FTLD]), vl1 = lds_frag_tr_h(&Vp[1][ro + 32], &Vp[1][ro + 32 + 8 * FTLD]);
      oacc0 = mfma16(vl0, ph, oacc0); oacc0 = mfma16(vh0, pl, oacc0); oacc0 = mfma16(vh0, ph, oacc0);
      oacc1 = mfma16(vl1, ph, oacc1); oacc1 = mfma16(vh1, pl, oacc1); oacc1 = mfma16(vh1, ph, oacc1);
    }
    wave_lds_fence();
  }

  l_run = xhalf_sum(l_run);
  const float inv = 1.f / l_run;
  if (qvalid) {
    float* op = O + ((size_t)b * N + qi) * HD + h * DH;
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) {
      const int d = 8 * rg + 4 * hf;
      *reinterpret_cast<float4*>(op + d) = make_float4(oacc0[4 * rg] * inv, oacc0[4 * rg + 1] * inv,
                                                       oacc0[4 * rg + 2] * inv, oacc0[4 * rg + 3] * inv);
      *reinterpret_cast<float4*>(op + 32 + d) = make_float4(oacc1[4 * rg] * inv, oacc1[4 * rg + 1] * inv,
                                                            oacc1[4 * rg + 2] * inv, oacc1[4 * rg + 3] * inv);
    }
    if (hf == 0) LSE[(size_t)(b * H + h) * N + qi] = m_run + logf(l_run);
  }
}

// ------------------------------------------------------------------------------------------------
// position-bias backward: one workgroup per (query tile of 32 BWD_WAVES, offset group, bag); every wave writes its own slab
// [SLAB] and its own d vs row [J][2] (file header for the arithmetic)
// ------------------------------------------------------------------------------------------------
template <int W, int PDX>
__global__ __launch_bounds__(64 * WideLds<W>::BWD_WAVES) void cpb_wide_bwd_kernel(
    const float* __restrict__ dLT, const float* __restrict__ VS, const float* __restrict__ GQ, CpbParams cp, float* __restrict__ slab,
    float* __restrict__ dvs_rows, int N, int J, int H, int G, int NST) {
  typedef WideLds<W> L;
  constexpr int PD = PosCfg<PDX>::PD;
  constexpr bool RAW = PosCfg<PDX>::RAW;
  constexpr int WV = L::BWD_WAVES, NT = W / 32, CPL = W / 64;       // channels per lane of the one-lane-per-channel passes
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, c = lane & 31, hf = lane >> 5;
  const int b = blockIdx.z, g = blockIdx.y, o = H / G;
  const int q0 = blockIdx.x * (QT * WV) + wave * QT;                // < NST (a multiple of 128)
  const bool qvalid = (q0 + c) < N;
  const int qi = qvalid ? (q0 + c) : (N - 1);
  float* X = smem + L::PARAMS + wave * L::WAVE;                     // [W][33]: r2, then g2, then g1
  float* Hs = X + L::STG;                                           // [W][33]: h1
  float* DB = Hs + L::STG;                                          // [2][32] d bias of the group's heads
  float* PS = DB + 64;                                              // [2][32] positions
  const int wg = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  float* sl = slab + (size_t)(wg * WV + wave) * L::SLAB;
  float2* dvs_row = reinterpret_cast<float2*>(dvs_rows) + (size_t)(wg * WV + wave) * J;
  wide_load_params<W, PD>(smem, cp, o, tid, 64 * WV);
  __syncthreads();                                                  // the only workgroup barrier: the waves are independent from here

  floatx16 acc2[NT][NT];                                            // d W2: rows = out, lane = in
#pragma unroll
  for (int a = 0; a < NT; ++a)
#pragma unroll
    for (int bb = 0; bb < NT; ++bb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[a][bb][r] = 0.f;
  float adb2[CPL], adw30[CPL], adw31[CPL], adb1[CPL], adw1x[CPL], adw1y[CPL];
#pragma unroll
  for (int i = 0; i < CPL; ++i) { adb2[i] = adw30[i] = adw31[i] = adb1[i] = adw1x[i] = adw1y[i] = 0.f; }
  float ab30 = 0.f, ab31 = 0.f;

  if (q0 < N) {                                                     // wave-uniform
    const float gq0 = GQ[(size_t)qi * PD];
    const float gq1 = (PD == 2) ? GQ[(size_t)qi * PD + 1] : 0.f;
    const float* VSb = VS + (size_t)(b * G + g) * J * PD;
    const float* dL0 = dLT + ((size_t)(b * H + g * o) * NST + q0) * J;     // this wave's [J][32] blocks of the group's heads
    const float* dL1 = dL0 + (size_t)NST * J;
    float big;                                                      // 2^100 (dpos_of)
    asm("s_mov_b32 %0, 0x71800000" : "=s"(big));
    for (int j = 0; j < J; ++j) {
      const float d0 = gq0 - VSb[(size_t)j * PD];
      const float d1 = (PD == 2) ? gq1 - VSb[(size_t)j * PD + 1] : 0.f;
      const float p0 = pos_of<RAW>(d0);
      const float p1 = (PD == 2) ? slog1p(d1) : 0.f;
      const float db0 = qvalid ? dL0[(size_t)j * 32 + c] : 0.f;     // lanes past the bag end read padding of their own tile: zeroed
      const float db1 = (qvalid && o == 2) ? dL1[(size_t)j * 32 + c] : 0.f;
      {
        float x1[W / 2];
        floatx16 d[NT];
        wide_eval<W>(smem, p0, p1, c, hf, x1, d);
#pragma unroll
        for (int s = 0; s < W / 2; ++s) Hs[(2 * s + hf) * 33 + c] = x1[s] > 0.f ? x1[s] : 0.f;
#pragma unroll
        for (int ot = 0; ot < NT; ++ot)
#pragma unroll
          for (int r = 0; r < 16; ++r) X[(32 * ot + acc_row(r, hf)) * 33 + c] = d[ot][r] > 0.f ? d[ot][r] : 0.f;
      }
      if (hf == 0) {
        DB[c] = db0; DB[32 + c] = db1;
        PS[c] = p0; PS[32 + c] = p1;
        ab30 += db0; ab31 += db1;
      }
      wave_lds_fence();
      // one lane per output channel: g2 = [D > 0] (w3^T d bias) in place of r2; d b2, d w3
#pragma unroll
      for (int i = 0; i < CPL; ++i) {
        const int ch = lane + 64 * i;
        const float w30 = smem[L::W3 + ch], w31 = smem[L::W3 + W + ch];
        float sb = 0.f, s0 = 0.f, s1 = 0.f;
        for (int qq = 0; qq < 32; ++qq) {
          const float r2 = X[ch * 33 + qq], e0 = DB[qq], e1 = DB[32 + qq];
          const float gg = r2 > 0.f ? fmaf(w31, e1, w30 * e0) : 0.f;
          X[ch * 33 + qq] = gg;
          sb += gg;
          s0 = fmaf(e0, r2, s0);
          s1 = fmaf(e1, r2, s1);
        }
        adb2[i] += sb; adw30[i] += s0; adw31[i] += s1;
      }
      wave_lds_fence();
      // d W2 += g2 . h1^T over the 32 queries
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        float av[NT], bv[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) { av[t] = X[(32 * t + c) * 33 + 2 * s + hf]; bv[t] = Hs[(32 * t + c) * 33 + 2 * s + hf]; }
#pragma unroll
        for (int ot = 0; ot < NT; ++ot)
#pragma unroll
          for (int it = 0; it < NT; ++it) acc2[ot][it] = mfma32(av[ot], bv[it], acc2[ot][it]);
      }
      // d h1 = W2^T g2, the layer-1 mask, d vs
      float sx = 0.f, sy = 0.f;
      floatx16 e[NT];
#pragma unroll
      for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int r = 0; r < 16; ++r) e[it][r] = 0.f;
#pragma unroll
      for (int s = 0; s < W / 2; ++s) {
        const float gv = X[(2 * s + hf) * 33 + c];
#pragma unroll
        for (int it = 0; it < NT; ++it) e[it] = mfma32(smem[(32 * it + c) * L::LD + 2 * s + hf], gv, e[it]);
      }
      wave_lds_fence();                                             // every read of g2 is done: X takes g1
#pragma unroll
      for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int ch = 32 * it + acc_row(r, hf);
          const float g1 = wide_x1<W>(smem, ch, p0, p1) > 0.f ? e[it][r] : 0.f;
          X[ch * 33 + c] = g1;
          sx = fmaf(g1, smem[L::W1X + ch], sx);
          sy = fmaf(g1, smem[L::W1Y + ch], sy);
        }
      // d pos / d vs = - d pos / d (gq - vs)
      const float vx = wave_sum(-sx * dpos_of<RAW>(d0, big));
      const float vy = (PD == 2) ? wave_sum(-sy * dpos_of<false>(d1, big)) : 0.f;
      if (lane == 0) dvs_row[j] = make_float2(vx, vy);
      wave_lds_fence();
      // one lane per hidden channel: d b1, d W1
#pragma unroll
      for (int i = 0; i < CPL; ++i) {
        const int ch = lane + 64 * i;
        float sb = 0.f, s0 = 0.f, s1 = 0.f;
        for (int qq = 0; qq < 32; ++qq) {
          const float g1 = X[ch * 33 + qq];
          sb += g1;
          s0 = fmaf(g1, PS[qq], s0);
          s1 = fmaf(g1, PS[32 + qq], s1);
        }
        adb1[i] += sb; adw1x[i] += s0; adw1y[i] += s1;
      }
      wave_lds_fence();
    }
  } else {
    for (int j = lane; j < J; j += 64) dvs_row[j] = make_float2(0.f, 0.f);
  }

#pragma unroll
  for (int ot = 0; ot < NT; ++ot)
#pragma unroll
    for (int it = 0; it < NT; ++it)
#pragma unroll
      for (int r = 0; r < 16; ++r) sl[(32 * ot + acc_row(r, hf)) * W + 32 * it + c] = acc2[ot][it][r];
  float* tail = sl + W * W;
#pragma unroll
  for (int i = 0; i < CPL; ++i) {
    const int ch = lane + 64 * i;
    tail[2 * ch] = adw1x[i];
    tail[2 * ch + 1] = adw1y[i];
    tail[2 * W + ch] = adb1[i];
    tail[3 * W + ch] = adb2[i];
    tail[4 * W + ch] = adw30[i];
    tail[5 * W + ch] = adw31[i];
  }
  const float t0 = wave_sum(ab30), t1 = wave_sum(ab31);
  if (lane == 0) { tail[6 * W] = t0; tail[6 * W + 1] = t1; tail[6 * W + 2] = 0.f; tail[6 * W + 3] = 0.f; }
}

// slab sums in a fixed order, two stages.  Stage 1: part[chunk][k] = sum of the chunk's slabs, in slab order
__global__ void wide_partial_kernel(const float* __restrict__ slab, int nslabs, int slab_len, int chunk, float* __restrict__ part) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= slab_len) return;
  const int s0 = blockIdx.y * chunk, s1 = min(s0 + chunk, nslabs);
  float t = 0.f;
  for (int s = s0; s < s1; ++s) t += slab[(size_t)s * slab_len + k];
  part[(size_t)blockIdx.y * slab_len + k] = t;
}
// Stage 2: one thread per output adds the chunk sums, in chunk order, and scatters into the parameter gradients
__global__ void wide_final_kernel(const float* __restrict__ part, int nchunks, int slab_len, int W, int PD, int o, float* __restrict__ dW1,
                                  float* __restrict__ db1, float* __restrict__ dW2, float* __restrict__ db2, float* __restrict__ dW3,
                                  float* __restrict__ db3) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= slab_len) return;
  float t = 0.f;
  for (int p = 0; p < nchunks; ++p) t += part[(size_t)p * slab_len + k];
  const int WW = W * W, r = k - WW;
  if (k < WW) dW2[k] = t;
  else if (r < 2 * W) { if ((r & 1) < PD) dW1[(r >> 1) * PD + (r & 1)] = t; }
  else if (r < 3 * W) db1[r - 2 * W] = t;
  else if (r < 4 * W) db2[r - 3 * W] = t;
  else if (r < 5 * W) dW3[r - 4 * W] = t;
  else if (r < 6 * W) { if (o == 2) dW3[W + r - 5 * W] = t; }
  else if (r == 6 * W) db3[0] = t;
  else if (r == 6 * W + 1) { if (o == 2) db3[1] = t; }
}
// dVS[(b, g)][j][0..PD) = sum of the group's rows (query tile, wave) in that order
__global__ void wide_dvs_reduce_kernel(const float2* __restrict__ rows, float* __restrict__ dVS, long long outs, int rows_per_group, int J, int PD) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= outs) return;
  const long long bg = t / J;
  const int j = (int)(t - bg * J);
  const float2* p = rows + (size_t)bg * rows_per_group * J + j;
  float sx = 0.f, sy = 0.f;
  for (int r = 0; r < rows_per_group; ++r) { const float2 v = p[(size_t)r * J]; sx += v.x; sy += v.y; }
  dVS[t * PD] = sx;
  if (PD == 2) dVS[t * PD + 1] = sy;
}

constexpr int WIDE_CHUNKS = 64;
// workspace of the backward (floats): [bwd_workspace of the dq / dkv passes][slabs][chunk sums][d vs rows]
struct WideWorkspace { size_t slab, part, dvs, total; int waves, xtiles, slab_len; size_t nslabs; };
WideWorkspace wide_workspace(int B, int N, int J, int H, int G, int W) {
  WideWorkspace w;
  w.waves = (W == 64) ? WideLds<64>::BWD_WAVES : WideLds<128>::BWD_WAVES;
  w.slab_len = (W == 64) ? WideLds<64>::SLAB : WideLds<128>::SLAB;
  w.xtiles = (N + QT * w.waves - 1) / (QT * w.waves);
  w.nslabs = (size_t)B * G * w.xtiles * w.waves;
  w.slab = (bwd_workspace(B, N, J, H).total + 3) & ~(size_t)3;
  w.part = w.slab + w.nslabs * w.slab_len;
  w.dvs = w.part + (size_t)WIDE_CHUNKS * w.slab_len;
  w.total = w.dvs + w.nslabs * (size_t)J * 2;
  return w;
}

int check_wide(const char* fn, int B, int N, int J, int H, int G, int W, int posdim) {
  SMML_REQUIRE(W == 64 || W == 128, "%s: the bias-MLP width W must be 64 or 128 (got %d)", fn, W);
  return check_common(fn, B, N, J, H, G, posdim);
}
template <typename Kern> int wide_lds(const char* fn, Kern kern, size_t bytes) {
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  SMML_REQUIRE(e == hipSuccess, "%s: hipFuncSetAttribute failed: %s", fn, hipGetErrorString(e));
  return SMML_OK;
}

template <int W, int PDX>
int wide_bias_launch(const char* fn, const float* vs, const float* gq, const CpbParams& cp, float* bt, int B, int N, int J, int H, int G,
                     hipStream_t st) {
  const size_t lds = (size_t)WideLds<W>::PARAMS * sizeof(float);
  if (int rc = wide_lds(fn, cpb_wide_bias_kernel<W, PDX>, lds)) return rc;
  hipLaunchKernelGGL((cpb_wide_bias_kernel<W, PDX>), dim3((N + QT * WAVES - 1) / (QT * WAVES), G, B), dim3(256), lds, st, vs, gq, cp, bt, N, J, H,
                     G, smml_deform_attn_nst(N));
  return launch_check(fn, "bias");
}
template <int W, int PDX>
int wide_decisions_launch(const char* fn, const float* vs, const float* gq, const CpbParams& cp, unsigned* dm, int B, int N, int J, int G,
                          hipStream_t st) {
  const size_t lds = (size_t)WideLds<W>::PARAMS * sizeof(float);
  if (int rc = wide_lds(fn, cpb_wide_decisions_kernel<W, PDX>, lds)) return rc;
  hipLaunchKernelGGL((cpb_wide_decisions_kernel<W, PDX>), dim3((N + QT * WAVES - 1) / (QT * WAVES), G, B), dim3(256), lds, st, vs, gq, cp, dm, N,
                     J, G);
  return launch_check(fn, "decisions");
}
template <int W, int PDX>
int wide_bwd_launch(const char* fn, const float* dlt, const float* vs, const float* gq, const CpbParams& cp, float* wsf, const WideWorkspace& w,
                    int B, int N, int J, int H, int G, hipStream_t st) {
  typedef WideLds<W> L;
  const size_t lds = ((size_t)L::PARAMS + (size_t)L::BWD_WAVES * L::WAVE) * sizeof(float);
  if (int rc = wide_lds(fn, cpb_wide_bwd_kernel<W, PDX>, lds)) return rc;
  hipLaunchKernelGGL((cpb_wide_bwd_kernel<W, PDX>), dim3(w.xtiles, G, B), dim3(64 * L::BWD_WAVES), lds, st, dlt, vs, gq, cp, wsf + w.slab,
                     wsf + w.dvs, N, J, H, G, smml_deform_attn_nst(N));
  return launch_check(fn, "cpb_wide");
}
// W in {64, 128} x PDX in {1, 2, 3}
#define WIDE_DISPATCH(W, pdx, CALL)                                                          \
  ((W) == 64 ? ((pdx) == 2 ? CALL(64, 2) : (pdx) == 3 ? CALL(64, 3) : CALL(64, 1))           \
             : ((pdx) == 2 ? CALL(128, 2) : (pdx) == 3 ? CALL(128, 3) : CALL(128, 1)))

}  // namespace

extern "C" {

size_t smml_deform_attn_wide_bwd_workspace_bytes(int B, int N, int J, int H, int G, int W) {
  if (!deform_dims_ok(B, N, J, H) || G <= 0 || H % G != 0 || (W != 64 && W != 128)) return 0;
  return wide_workspace(B, N, J, H, G, W).total * sizeof(float);
}

int smml_deform_attn_wide_fwd_f32(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* w1,
                                  const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, float* out, float* lse,
                                  float* logits_t, float* bias_t, int B, int N, int J, int H, int G, int W, int posdim, float scale,
                                  float dropout_p, unsigned long long dropout_seed, void* ev_start, void* ev_stop, void* stream,
                                  const SmmlDeformOpts* opts) {
  static const char* fn = "smml_deform_attn_wide_fwd_f32";
  int rc = check_wide(fn, B, N, J, H, G, W, posdim);
  if (!rc) rc = check_dropout(fn, dropout_p);
  if (rc) return rc;
  SMML_REQUIRE(q && k && v && vs && gq && w1 && b1 && w2 && b2 && w3 && b3 && out && lse, "%s: null pointer", fn);
  SMML_REQUIRE((logits_t == nullptr) != (bias_t == nullptr), "%s: pass logits_t (training: the bias tiles are built there and overwritten by "
               "the scores) or bias_t (inference: scratch of the same size), not both", fn);
  const DropCfg dc = make_drop(dropout_p, dropout_seed, opts);
  const CpbParams cp{w1, b1, w2, b2, w3, b3};
  const int pdx = pdx_of(posdim, opts);
  hipStream_t st = (hipStream_t)stream;
  float* bt = logits_t ? logits_t : bias_t;
  if (ev_start) (void)hipEventRecord((hipEvent_t)ev_start, st);
#define WIDE_BIAS(W_, P_) wide_bias_launch<W_, P_>(fn, vs, gq, cp, bt, B, N, J, H, G, st)
  rc = WIDE_DISPATCH(W, pdx, WIDE_BIAS);
#undef WIDE_BIAS
  if (rc) return rc;
  const dim3 grid((N + QT * WAVES - 1) / (QT * WAVES), H, B);
  const int nst = smml_deform_attn_nst(N);
  if (logits_t)
    hipLaunchKernelGGL(deform_attn_biasmem_fwd_kernel<true>, grid, dim3(256), 0, st, q, k, v, bt, out, lse, logits_t, N, J, H, nst, scale, dc);
  else
    hipLaunchKernelGGL(deform_attn_biasmem_fwd_kernel<false>, grid, dim3(256), 0, st, q, k, v, bt, out, lse, (float*)nullptr, N, J, H, nst, scale,
                       dc);
  if (ev_stop) (void)hipEventRecord((hipEvent_t)ev_stop, st);
  return launch_check(fn, "attn");
}

int smml_deform_attn_wide_bwd_f32(const float* q, const float* k, const float* v, const float* vs, const float* gq, const float* w1,
                                  const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, const float* out,
                                  const float* dout, const float* lse, const float* logits_t, float* dlogits_t, float* dq, float* dk, float* dv,
                                  float* dvs, float* dw1, float* db1, float* dw2, float* db2, float* dw3, float* db3, void* workspace,
                                  size_t workspace_bytes, int B, int N, int J, int H, int G, int W, int posdim, float scale, float dropout_p,
                                  unsigned long long dropout_seed, void* ev_start, void* ev_stop, void* stream, const SmmlDeformOpts* opts) {
  static const char* fn = "smml_deform_attn_wide_bwd_f32";
  int rc = check_wide(fn, B, N, J, H, G, W, posdim);
  if (!rc) rc = check_dropout(fn, dropout_p);
  if (rc) return rc;
  SMML_REQUIRE(q && k && v && vs && gq && w1 && b1 && w2 && b2 && w3 && b3 && out && dout && lse && logits_t && dlogits_t && dq && dk && dv &&
                   dvs && dw1 && db1 && dw2 && db2 && dw3 && db3 && workspace, "%s: null pointer", fn);
  if ((rc = check_workspace(fn, workspace, workspace_bytes, smml_deform_attn_wide_bwd_workspace_bytes(B, N, J, H, G, W), 16))) return rc;
  const CpbParams cp{w1, b1, w2, b2, w3, b3};
  hipStream_t st = (hipStream_t)stream;
  float* wsf = reinterpret_cast<float*>(workspace);
  if ((rc = smml_wide_bwd_dq_dkv(fn, q, k, v, out, dout, lse, logits_t, dlogits_t, dq, dk, dv, wsf, B, N, J, H, scale, dropout_p, dropout_seed,
                                 opts, stream)))
    return rc;
  const WideWorkspace w = wide_workspace(B, N, J, H, G, W);
  SMML_REQUIRE(w.nslabs <= (size_t)1 << 30, "%s: %zu per-wave slabs (at most 2^30)", fn, w.nslabs);
  const int pdx = pdx_of(posdim, opts);
  if (ev_start) (void)hipEventRecord((hipEvent_t)ev_start, st);   // brackets the position-bias backward kernel only
#define WIDE_BWD(W_, P_) wide_bwd_launch<W_, P_>(fn, dlogits_t, vs, gq, cp, wsf, w, B, N, J, H, G, st)
  rc = WIDE_DISPATCH(W, pdx, WIDE_BWD);
#undef WIDE_BWD
  if (ev_stop) (void)hipEventRecord((hipEvent_t)ev_stop, st);
  if (rc) return rc;
  const long long outs = (long long)B * G * J;
  hipLaunchKernelGGL(wide_dvs_reduce_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float2*>(wsf + w.dvs),
                     dvs, outs, w.xtiles * w.waves, J, posdim);
  const int nslabs = (int)w.nslabs;
  const int nchunks = min(WIDE_CHUNKS, nslabs), chunk = (nslabs + nchunks - 1) / nchunks;
  const int used = (nslabs + chunk - 1) / chunk;                  // chunks that hold at least one slab
  hipLaunchKernelGGL(wide_partial_kernel, dim3((w.slab_len + 255) / 256, used), dim3(256), 0, st, wsf + w.slab, nslabs, w.slab_len, chunk,
                     wsf + w.part);
  hipLaunchKernelGGL(wide_final_kernel, dim3((w.slab_len + 255) / 256), dim3(256), 0, st, wsf + w.part, used, w.slab_len, W, posdim, H / G, dw1,
                     db1, dw2, db2, dw3, db3);
  return launch_check(fn, "reduce");
}

int smml_deform_attn_wide_decisions(const float* vs, const float* gq, const float* w1, const float* b1, const float* w2, const float* b2,
                                    unsigned* masks, int B, int N, int J, int G, int W, int posdim, void* stream, const SmmlDeformOpts* opts) {
  static const char* fn = "smml_deform_attn_wide_decisions";
  SMML_REQUIRE(W == 64 || W == 128, "%s: the bias-MLP width W must be 64 or 128 (got %d)", fn, W);
  SMML_REQUIRE(deform_dims_ok(B, N, J, G) && (posdim == 1 || posdim == 2), "%s: bad size", fn);
  SMML_REQUIRE(vs && gq && w1 && b1 && w2 && b2 && masks, "%s: null pointer", fn);
  const CpbParams cp{w1, b1, w2, b2, w2, b2};                     // w3 / b3 are not read (o = 1 loads W floats of w3: any W readable floats)
  const int pdx = pdx_of(posdim, opts);
  hipStream_t st = (hipStream_t)stream;
#define WIDE_DEC(W_, P_) wide_decisions_launch<W_, P_>(fn, vs, gq, cp, masks, B, N, J, G, st)
  const int rc = WIDE_DISPATCH(W, pdx, WIDE_DEC);
#undef WIDE_DEC
  return rc;
}

}  // extern "C"
