// CDNA4 kernels for GatedDeltaNet (the fla-core replacement:
// reference d9d/module/block/attention/linear/gated_deltanet.py:6-8,360-370).
//
// 1. causal_conv_silu fwd/bwd: per-channel causal conv (kernel<=4) fused
//    with SiLU over (B, S, C) — one HBM read + write instead of the
//    pad/conv1d/silu chain.
// 2. gdn_chunk_fwd: the chunked-parallel WY gated delta rule, one
//    workgroup per (b, h), chunks of 64 sequential with the fp32 state
//    resident in LDS. MFMA bf16 for the chunk GEMMs (KK^T, QK^T, K@S,
//    Q@S, N@R, K^T@R), fp32 blocked forward-substitution for the
//    unit-lower triangular solve. Dk = Dv = 64.
//    (The python wrapper pairs this forward with a recompute-through-the
//    torch-WY-graph backward; a native bwd kernel is the follow-up.)
// 3. Packed-document (cu_seqlens) variants of all four entry points: the
//    same kernel bodies under a VARLEN template flag — one workgroup per
//    (document, head) from a zero state, conv taps clipped at the
//    document start. cu_seqlens is validated on the host before launch.
#include "common.h"
#include "mfma.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace d9d {

// ---------------------------------------------------------------------------
// causal depthwise conv (kernel <= 4) + SiLU, bf16
// ---------------------------------------------------------------------------
//
// VARLEN: x is one packed row of documents (B == 1) and cu (nseq+1 int32,
// host-validated: cu[0] = 0, non-decreasing, cu[nseq] = S) bounds them; a
// tap is taken only inside the document that row s belongs to. Dense is the
// same code with the document being the whole row [0, S).

// Document [lo, hi) holding packed row s: the last i with cu[i] <= s (empty
// documents repeat an entry; the last repeat is the non-empty one).
D9D_DEVICE void conv_doc_bounds(const int* __restrict__ cu, int nseq,
                                int64_t s, int64_t& lo, int64_t& hi) {
  int a = 0, b = nseq - 1;
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if ((int64_t)cu[mid] <= s) a = mid; else b = mid - 1;
  }
  lo = cu[a];
  hi = cu[a + 1];
}

template <bool VARLEN>
__global__ void causal_conv_silu_fwd_kernel(
    const bf16_t* __restrict__ x,   // (B, S, C)
    const bf16_t* __restrict__ w,   // (C, K)
    bf16_t* __restrict__ out,       // (B, S, C)
    const int* __restrict__ cu, int nseq,
    int64_t B, int64_t S, int64_t C, int K) {
  const int64_t total = B * S * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = i % C;
    const int64_t s = (i / C) % S;
    const int64_t b = i / (C * S);
    int64_t lo = 0, hi = S;
    if constexpr (VARLEN) conv_doc_bounds(cu, nseq, s, lo, hi);
    (void)hi;
    float acc = 0.f;
#pragma unroll 4
    for (int t = 0; t < K; ++t) {
      const int64_t sp = s - (K - 1 - t);
      if (sp >= lo) {
        acc += (float)x[(b * S + sp) * C + c] * (float)w[c * K + t];
      }
    }
    const float sig = 1.f / (1.f + __builtin_amdgcn_exp2f(-acc * 1.44269504f));
    out[i] = (bf16_t)(acc * sig);
  }
}

// dx and dw for conv+silu. dpre = dy * silu'(pre); dx[s] = sum_t dpre[s+K-1-t]*w[t]
// (within bounds); dw[c,t] = sum_{b,s} dpre[b,s,c] * x[b, s-(K-1-t), c].
template <bool VARLEN>
__global__ void causal_conv_silu_bwd_kernel(
    const bf16_t* __restrict__ x,
    const bf16_t* __restrict__ w,
    const bf16_t* __restrict__ dy,
    bf16_t* __restrict__ dx,        // (B, S, C)
    float* __restrict__ dw,         // (C, K) fp32 (atomic)
    const int* __restrict__ cu, int nseq,
    int64_t B, int64_t S, int64_t C, int K) {
  const int64_t total = B * S * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t c = i % C;
    const int64_t s = (i / C) % S;
    const int64_t b = i / (C * S);
    // every row this thread touches (s-K+1 .. s+K-1, clipped) is in s's
    // document, so one lookup serves the dx, dw and recompute taps
    int64_t lo = 0, hi = S;
    if constexpr (VARLEN) conv_doc_bounds(cu, nseq, s, lo, hi);

    // recompute pre-activation at s (cheap: K<=4 reads)
    auto pre_at = [&](int64_t sq) -> float {
      float acc = 0.f;
#pragma unroll 4
      for (int t = 0; t < K; ++t) {
        const int64_t sp = sq - (K - 1 - t);
        if (sp >= lo) acc += (float)x[(b * S + sp) * C + c] * (float)w[c * K + t];
      }
      return acc;
    };
    auto dsilu = [&](float a) -> float {
      const float sig = 1.f / (1.f + __builtin_amdgcn_exp2f(-a * 1.44269504f));
      return sig * (1.f + a * (1.f - sig));
    };

    // dx[s]: gather from future positions using dpre there
    float acc_dx = 0.f;
#pragma unroll 4
    for (int t = 0; t < K; ++t) {
      const int64_t sq = s + (K - 1 - t);
      if (sq < hi) {
        const float dpre = (float)dy[(b * S + sq) * C + c] * dsilu(pre_at(sq));
        acc_dx += dpre * (float)w[c * K + t];
      }
    }
    dx[i] = (bf16_t)acc_dx;

    // dw contributions from THIS position's dpre
    const float dpre_s = (float)dy[i] * dsilu(pre_at(s));
#pragma unroll 4
    for (int t = 0; t < K; ++t) {
      const int64_t sp = s - (K - 1 - t);
      if (sp >= lo) {
        atomicAdd(&dw[c * K + t], dpre_s * (float)x[(b * S + sp) * C + c]);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// chunked gated delta rule forward, Dk = Dv = 64, chunk C = 64
// ---------------------------------------------------------------------------
//
// One workgroup (4 waves, 256 threads) per (b, h). Chunks run sequentially
// with the fp32 state resident in LDS. Per chunk (t, j in [0, 64); rows
// past the sequence end are ZERO-padded so every product is exact):
//   gc      = cumsum(g)                                   (serial scan)
//   M[t,j]  = beta_t (K K^T)[t,j] e^{gc_t-gc_j}  (j < t)  (MFMA)
//   rhs     = diag(beta) (V - (e^{gc} K) @ S)             (MFMA, S as bf16)
//   R: (I + M) R = rhs    forward substitution, fp32, 4-way j-split
//   N[t,j]  = (Q K^T)[t,j] e^{gc_t-gc_j}  (j <= t)        (MFMA)
//   O       = (e^{gc} Q) @ S + N @ R                      (MFMA, R as bf16)
//   S       = e^{gc_last} S + (K e^{gc_last-gc})^T @ R    (fp32 VALU)
//
// MFMA fragment map: see mfma.h (verified by attention.hip's
//   mfma_selfcheck). All tiles here are row-major [row][64] so A fragments
//   are contiguous row reads; B fragments read the row of the TRANSPOSED
//   operand copy (kc rows for K^T, sbT rows for S, rbT rows for R).

constexpr int kGdnC = 64;   // chunk rows
constexpr int kGdnD = 64;   // Dk = Dv

// DVT: this block's Dv slice (64 = whole head, 32 = half). The state
// columns are independent, so gridDim.y splits Dv across blocks — K-side
// work (KK^T, M, N, the decay scan) is duplicated per split, but B*H
// workgroups only fill half the 256 CUs at the bench shape, so a 2-way
// split still wins well below chip saturation.
template <int DVT>
struct GdnLds {
  float state[kGdnD][DVT];        // S (k, v-slice) fp32
  float M[kGdnC][kGdnC + 1];      // solve matrix (+1 pad)
  float R[kGdnC][DVT];            // solve result fp32
  float rhs[kGdnC][DVT];          // rhs / partials scratch
  bf16_t kc[kGdnC][kGdnD];        // K chunk
  bf16_t qc[kGdnC][kGdnD];        // Q chunk
  bf16_t vc[kGdnC][DVT];          // V chunk slice
  bf16_t ks[kGdnC][kGdnD];        // scaled K / scaled Q / scaled-K2 scratch
  bf16_t sbT[DVT][kGdnD];         // state^T cast to bf16: sbT[v][k]
  bf16_t nb[kGdnC][kGdnC];        // N cast to bf16
  bf16_t rbT[DVT][kGdnC];         // R^T cast to bf16: rbT[v][t]
  float gc[kGdnC];
  float beta[kGdnC];
};

// What one workgroup walks: `len` rows starting at flat row `row0` of the
// (B*H*S) row space, whose chunks are numbered from `chunk0` in the
// (B*H*nc) chunk space.
//   dense : workgroup = (b, h); the whole sequence, row0 = bh*S.
//   varlen: workgroup = (document, head) of ONE packed row (B == 1, S = T
//           packed tokens); the document's rows only, chunks local to the
//           document and numbered after those of the documents before it
//           (chunk_off, nc_total = chunk_off[nseq]). cu / chunk_off are
//           host-validated: cu[0] = 0, non-decreasing, cu[nseq] = S.
struct GdnSpan {
  int64_t row0;
  int64_t chunk0;
  int64_t len;
};

template <bool VARLEN>
D9D_DEVICE GdnSpan gdn_span(int64_t wg, int64_t S, const int* __restrict__ cu,
                            const int* __restrict__ chunk_off, int H,
                            int64_t nc_total) {
  GdnSpan sp;
  if constexpr (VARLEN) {
    const int64_t doc = wg / H;
    const int64_t h = wg % H;
    const int64_t start = cu[doc];
    sp.row0 = h * S + start;
    sp.chunk0 = h * nc_total + chunk_off[doc];
    sp.len = (int64_t)cu[doc + 1] - start;
  } else {
    sp.row0 = wg * S;
    sp.chunk0 = wg * ((S + kGdnC - 1) / kGdnC);
    sp.len = S;
  }
  return sp;
}

template <int DVT, bool VARLEN>
__global__ __launch_bounds__(256, 1) void gdn_chunk_fwd_kernel(
    const bf16_t* __restrict__ q,   // (B, H, S, D)
    const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v,
    const float* __restrict__ beta,      // (B, H, S)
    const float* __restrict__ decay_log, // (B, H, S)
    bf16_t* __restrict__ out,            // (B, H, S, D)
    float* __restrict__ final_state,     // (n_wg, D, D) or nullptr
    float* __restrict__ r_out,           // (B, H, S, D) fp32 or nullptr
    float* __restrict__ s0_out,          // (B, H, nc, D, D) fp32 or nullptr
    int64_t n_wg, int64_t S,
    const int* __restrict__ cu,          // varlen only
    const int* __restrict__ chunk_off,   // varlen only
    int H, int64_t nc_total) {           // varlen only
  constexpr int NTV = DVT / 16;        // v tiles per wave quarter
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  GdnLds<DVT>& L = *reinterpret_cast<GdnLds<DVT>*>(smem_raw);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;   // 4 waves; wave w owns m-rows 16w..16w+15
  const int64_t bh = blockIdx.x;
  const int v0 = blockIdx.y * DVT;     // this block's Dv slice
  if (bh >= n_wg) return;

  const GdnSpan span = gdn_span<VARLEN>(bh, S, cu, chunk_off, H, nc_total);
  const int64_t len = span.len;
  const bf16_t* qp = q + span.row0 * kGdnD;
  const bf16_t* kp = k + span.row0 * kGdnD;
  const bf16_t* vp = v + span.row0 * kGdnD;
  const float* bp = beta + span.row0;
  const float* gp = decay_log + span.row0;
  bf16_t* op = out + span.row0 * kGdnD;

  for (int i = threadIdx.x; i < kGdnD * DVT; i += 256) {
    (&L.state[0][0])[i] = 0.f;
  }
  __syncthreads();

  const float kLog2eG = 1.44269504f;
  const int n_chunks = (int)((len + kGdnC - 1) / kGdnC);
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int s0 = ch * kGdnC;
    const int c_rows = min((int)(len - (int64_t)s0), kGdnC);

    // ---- stage chunk tiles (zero-pad past c_rows) + state^T bf16 -------
    for (int i = threadIdx.x; i < kGdnC * kGdnD / 8; i += 256) {
      const int row = (i * 8) / kGdnD;
      const int col = (i * 8) % kGdnD;
      if (row < c_rows) {
        const int64_t off = (int64_t)(s0 + row) * kGdnD + col;
        *reinterpret_cast<bf16x8*>(&L.kc[row][col]) =
            *reinterpret_cast<const bf16x8*>(kp + off);
        *reinterpret_cast<bf16x8*>(&L.qc[row][col]) =
            *reinterpret_cast<const bf16x8*>(qp + off);
      } else {
        bf16x8 z = {};
        *reinterpret_cast<bf16x8*>(&L.kc[row][col]) = z;
        *reinterpret_cast<bf16x8*>(&L.qc[row][col]) = z;
      }
    }
    for (int i = threadIdx.x; i < kGdnC * DVT / 8; i += 256) {
      const int row = (i * 8) / DVT;
      const int col = (i * 8) % DVT;
      if (row < c_rows) {
        *reinterpret_cast<bf16x8*>(&L.vc[row][col]) =
            *reinterpret_cast<const bf16x8*>(
                vp + (int64_t)(s0 + row) * kGdnD + v0 + col);
      } else {
        bf16x8 z = {};
        *reinterpret_cast<bf16x8*>(&L.vc[row][col]) = z;
      }
    }
    for (int i = threadIdx.x; i < DVT * kGdnD; i += 256) {
      const int vcol = i / kGdnD;
      const int dk = i % kGdnD;
      L.sbT[vcol][dk] = (bf16_t)L.state[dk][vcol];
    }
    if (threadIdx.x == 0) {
      float run = 0.f;
      for (int t = 0; t < kGdnC; ++t) {
        if (t < c_rows) run += gp[s0 + t];
        L.gc[t] = run;                       // clamped-constant past end
        L.beta[t] = (t < c_rows) ? bp[s0 + t] : 0.f;
      }
    }
    __syncthreads();

    if (s0_out != nullptr) {
      float* sp = s0_out + (span.chunk0 + ch) * (int64_t)kGdnD * kGdnD;
      for (int i = threadIdx.x; i < kGdnD * DVT; i += 256) {
        const int dk = i / DVT;
        const int dv = i % DVT;
        sp[dk * kGdnD + v0 + dv] = L.state[dk][dv];
      }
    }

    // ---- M = tril(beta * KK^T * ratio, -1) -----------------------------
    {
      f32x4 acc[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
      const int arow = wave * 16 + (lane & 15);
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        const int d0 = ks2 * 32 + (lane >> 4) * 8;
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(&L.kc[arow][d0]);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int brow = nt * 16 + (lane & 15);   // B = K^T: col j = K row j
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(&L.kc[brow][d0]);
          acc[nt] = mfma16(a, b, acc[nt]);
        }
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = wave * 16 + (lane >> 4) * 4 + r;
          const int j = nt * 16 + (lane & 15);
          float m = 0.f;
          if (j < t) {
            m = L.beta[t] * acc[nt][r] *
                __builtin_amdgcn_exp2f((L.gc[t] - L.gc[j]) * kLog2eG);
          }
          L.M[t][j] = m;
        }
      }
    }
    __syncthreads();

    // ---- rhs = diag(beta) (V - (e^{gc} K) @ S) -------------------------
    for (int i = threadIdx.x; i < kGdnC * kGdnD / 8; i += 256) {
      const int row = (i * 8) / kGdnD;
      const int col = (i * 8) % kGdnD;
      const float sc = __builtin_amdgcn_exp2f(L.gc[row] * kLog2eG);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        L.ks[row][col + j] = (bf16_t)((float)L.kc[row][col + j] * sc);
      }
    }
    __syncthreads();
    {
      f32x4 acc[NTV];
#pragma unroll
      for (int nt = 0; nt < NTV; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
      const int arow = wave * 16 + (lane & 15);
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        const int d0 = ks2 * 32 + (lane >> 4) * 8;
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(&L.ks[arow][d0]);
#pragma unroll
        for (int nt = 0; nt < NTV; ++nt) {
          const int vcol = nt * 16 + (lane & 15);
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(&L.sbT[vcol][d0]);
          acc[nt] = mfma16(a, b, acc[nt]);
        }
      }
#pragma unroll
      for (int nt = 0; nt < NTV; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = wave * 16 + (lane >> 4) * 4 + r;
          const int vcol = nt * 16 + (lane & 15);
          L.rhs[t][vcol] =
              L.beta[t] * ((float)L.vc[t][vcol] - acc[nt][r]);
        }
      }
    }
    __syncthreads();

    // ---- forward substitution: (I + M) R = rhs -------------------------
    // wave w owns Dv columns [16w, 16w+16); its 64 lanes split as
    // (j-quarter, col): lane = qj*16 + c. Row t: each lane partial-sums its
    // j-quarter of M[t,:]*R[:,col], a 2-step xor-shuffle combines the 4
    // partials, and the qj==0 lane writes R[t][col] (+ bf16 R^T copy).
    {
      // wave owns DVT/4 columns; its 64 lanes split as (j-group, col):
      // DVT=64: 16 cols x 4 j-quarters; DVT=32: 8 cols x 8 j-octants.
      constexpr int CPW = DVT / 4;           // cols per wave
      constexpr int JG = 64 / CPW;           // j groups
      const int c = lane % CPW;
      const int qj = lane / CPW;
      const int col = wave * CPW + c;
      const int jspan = kGdnC / JG;
      for (int t = 0; t < kGdnC; ++t) {
        float part = 0.f;
        const int jend = min(t, (qj + 1) * jspan);
        for (int j = qj * jspan; j < jend; ++j) {
          part += L.M[t][j] * L.R[j][col];
        }
        // all 64 lanes active and convergent: xor-shuffles are safe
#pragma unroll
        for (int off = CPW; off < 64; off <<= 1) {
          part += __shfl_xor(part, off, 64);
        }
        const float r_t = L.rhs[t][col] - part;
        if (qj == 0) {
          L.R[t][col] = r_t;
          L.rbT[col][t] = (bf16_t)r_t;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();

    if (r_out != nullptr) {
      for (int i = threadIdx.x; i < kGdnC * DVT; i += 256) {
        const int t = i / DVT;
        const int dv = i % DVT;
        if (t < c_rows) {
          r_out[(span.row0 + s0 + t) * kGdnD + v0 + dv] = L.R[t][dv];
        }
      }
    }

    // ---- N (bf16) and O = (e^{gc} Q) @ S + N @ R -----------------------
    // (skipped when out == nullptr: the backward recompute only needs the
    // solve results and chunk states)
    if (out != nullptr) {
      for (int i = threadIdx.x; i < kGdnC * kGdnD / 8; i += 256) {
        const int row = (i * 8) / kGdnD;
        const int col = (i * 8) % kGdnD;
        const float sc = __builtin_amdgcn_exp2f(L.gc[row] * kLog2eG);
  #pragma unroll
        for (int j = 0; j < 8; ++j) {
          L.ks[row][col + j] = (bf16_t)((float)L.qc[row][col + j] * sc);
        }
      }
      __syncthreads();
      {
        // N = tril(QK^T * ratio, 0) -> nb (bf16)
        f32x4 acc[4];
  #pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
        const int arow = wave * 16 + (lane & 15);
  #pragma unroll
        for (int ks2 = 0; ks2 < 2; ++ks2) {
          const int d0 = ks2 * 32 + (lane >> 4) * 8;
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(&L.qc[arow][d0]);
  #pragma unroll
          for (int nt = 0; nt < 4; ++nt) {
            const int brow = nt * 16 + (lane & 15);
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(&L.kc[brow][d0]);
            acc[nt] = mfma16(a, b, acc[nt]);
          }
        }
  #pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
  #pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int t = wave * 16 + (lane >> 4) * 4 + r;
            const int j = nt * 16 + (lane & 15);
            float n = 0.f;
            if (j <= t) {
              n = acc[nt][r] *
                  __builtin_amdgcn_exp2f((L.gc[t] - L.gc[j]) * kLog2eG);
            }
            L.nb[t][j] = (bf16_t)n;
          }
        }
      }
      __syncthreads();
      {
        f32x4 acc[NTV];
  #pragma unroll
        for (int nt = 0; nt < NTV; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
        const int arow = wave * 16 + (lane & 15);
        // (e^{gc} Q) @ S
  #pragma unroll
        for (int ks2 = 0; ks2 < 2; ++ks2) {
          const int d0 = ks2 * 32 + (lane >> 4) * 8;
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(&L.ks[arow][d0]);
  #pragma unroll
          for (int nt = 0; nt < NTV; ++nt) {
            const int vcol = nt * 16 + (lane & 15);
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(&L.sbT[vcol][d0]);
            acc[nt] = mfma16(a, b, acc[nt]);
          }
        }
        // + N @ R  (k dim = chunk rows j, 64 wide)
  #pragma unroll
        for (int ks2 = 0; ks2 < 2; ++ks2) {
          const int j0 = ks2 * 32 + (lane >> 4) * 8;
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(&L.nb[arow][j0]);
  #pragma unroll
          for (int nt = 0; nt < NTV; ++nt) {
            const int vcol = nt * 16 + (lane & 15);
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(&L.rbT[vcol][j0]);
            acc[nt] = mfma16(a, b, acc[nt]);
          }
        }
  #pragma unroll
        for (int nt = 0; nt < NTV; ++nt) {
  #pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int t = wave * 16 + (lane >> 4) * 4 + r;
            const int vcol = nt * 16 + (lane & 15);
            if (t < c_rows) {
              op[(int64_t)(s0 + t) * kGdnD + v0 + vcol] = (bf16_t)acc[nt][r];
            }
          }
        }
      }
      __syncthreads();

    }

    // ---- state = e^{gc_last} S + (K e^{gc_last - gc})^T @ R ------------
    {
      const float g_tot = L.gc[c_rows - 1];
      for (int i = threadIdx.x; i < kGdnC * kGdnD / 8; i += 256) {
        const int row = (i * 8) / kGdnD;
        const int col = (i * 8) % kGdnD;
        const float sc =
            (row < c_rows)
                ? __builtin_amdgcn_exp2f((g_tot - L.gc[row]) * kLog2eG)
                : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          L.ks[row][col + j] = (bf16_t)((float)L.kc[row][col + j] * sc);
        }
      }
      __syncthreads();
      const float e_tot = __builtin_amdgcn_exp2f(g_tot * kLog2eG);
      for (int i = threadIdx.x; i < kGdnD * DVT; i += 256) {
        const int dk = i / DVT;
        const int dv = i % DVT;
        float acc = L.state[dk][dv] * e_tot;
        for (int t = 0; t < c_rows; ++t) {
          acc += (float)L.ks[t][dk] * L.R[t][dv];
        }
        L.state[dk][dv] = acc;
      }
    }
    __syncthreads();
  }

  if (final_state != nullptr) {
    float* fs = final_state + bh * kGdnD * kGdnD;
    for (int i = threadIdx.x; i < kGdnD * DVT; i += 256) {
      const int dk = i / DVT;
      const int dv = i % DVT;
      fs[dk * kGdnD + v0 + dv] = L.state[dk][dv];
    }
  }
}

// ---------------------------------------------------------------------------
// chunked gated delta rule backward REVERSE SCAN, Dk = Dv = 64
// ---------------------------------------------------------------------------
//
// Mirror of the forward chunk kernel for the sequential half of the
// hand-derived backward (gated_deltanet.py _chunk_gdn_backward): one
// workgroup per (b, h), chunks walked BACKWARD with dL/dState fp32 in LDS.
// Per chunk (incoming dS = dL/d(S1) of this chunk):
//   M, N      recomputed exactly as the forward kernel
//   dR        = (w K) @ dS + N^T @ dO,     w_t = e^{gc_last - gc_t}
//   drhs      : (I + M)^T drhs = dR        backward substitution, in place
//   dS        = e^{gc_last} dS + (e^{gc} K)^T @ (-beta drhs)
//                                + (e^{gc} Q)^T @ dO
// Outputs drhs (B,H,S,D fp32) and the per-chunk dL/dS0 (B,H,nc,D,D fp32);
// the non-sequential leaf gradients stay batched torch GEMMs.
template <int DVT>
struct GdnBwdLds {
  float dS[kGdnD][DVT];           // dL/dState fp32 (v slice)
  float M[kGdnC][kGdnC + 1];      // solve matrix (+1 pad)
  float dx[kGdnC][DVT + 1];       // dR -> drhs in place (+1 pad)
  bf16_t kc[kGdnC][kGdnD];        // K chunk
  bf16_t qc[kGdnC][kGdnD];        // Q chunk
  bf16_t doc[kGdnC][DVT];         // dO chunk slice
  bf16_t doT[DVT][kGdnC];         // dO^T (B fragments of N^T @ dO)
  bf16_t ks[kGdnC][kGdnD];        // scaled K / scaled Q scratch
  bf16_t dsT[DVT][kGdnD];         // dS^T cast to bf16 (B fragments)
  bf16_t nbT[kGdnC][kGdnC];       // N^T cast to bf16 (A fragments)
  float gc[kGdnC];
  float beta[kGdnC];
};

template <int DVT, bool VARLEN>
__global__ __launch_bounds__(256, 1) void gdn_chunk_bwd_scan_kernel(
    const bf16_t* __restrict__ q,    // (B, H, S, D)
    const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ dout, // (B, H, S, D)
    const float* __restrict__ beta,
    const float* __restrict__ decay_log,
    float* __restrict__ drhs_out,    // (B, H, S, D)
    float* __restrict__ ds0_out,     // (B, H, nc, D, D)
    int64_t n_wg, int64_t S,
    const int* __restrict__ cu,          // varlen only (see GdnSpan)
    const int* __restrict__ chunk_off,   // varlen only
    int H, int64_t nc_total) {           // varlen only
  constexpr int NTV = DVT / 16;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  GdnBwdLds<DVT>& L = *reinterpret_cast<GdnBwdLds<DVT>*>(smem_raw);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t bh = blockIdx.x;
  const int v0 = blockIdx.y * DVT;
  if (bh >= n_wg) return;

  const GdnSpan span = gdn_span<VARLEN>(bh, S, cu, chunk_off, H, nc_total);
  const int64_t len = span.len;
  const bf16_t* qp = q + span.row0 * kGdnD;
  const bf16_t* kp = k + span.row0 * kGdnD;
  const bf16_t* dop = dout + span.row0 * kGdnD;
  const float* bp = beta + span.row0;
  const float* gp = decay_log + span.row0;

  for (int i = threadIdx.x; i < kGdnD * DVT; i += 256) {
    (&L.dS[0][0])[i] = 0.f;
  }
  __syncthreads();

  const float kLog2eG = 1.44269504f;
  const int n_chunks = (int)((len + kGdnC - 1) / kGdnC);
  for (int ch = n_chunks - 1; ch >= 0; --ch) {
    const int s0 = ch * kGdnC;
    const int c_rows = min((int)(len - (int64_t)s0), kGdnC);

    // ---- stage chunk tiles (zero-pad), dS^T, decay scan ----------------
    for (int i = threadIdx.x; i < kGdnC * kGdnD / 8; i += 256) {
      const int row = (i * 8) / kGdnD;
      const int col = (i * 8) % kGdnD;
      if (row < c_rows) {
        const int64_t off = (int64_t)(s0 + row) * kGdnD + col;
        *reinterpret_cast<bf16x8*>(&L.kc[row][col]) =
            *reinterpret_cast<const bf16x8*>(kp + off);
        *reinterpret_cast<bf16x8*>(&L.qc[row][col]) =
            *reinterpret_cast<const bf16x8*>(qp + off);
      } else {
        bf16x8 z = {};
        *reinterpret_cast<bf16x8*>(&L.kc[row][col]) = z;
        *reinterpret_cast<bf16x8*>(&L.qc[row][col]) = z;
      }
    }
    for (int i = threadIdx.x; i < kGdnC * DVT / 8; i += 256) {
      const int row = (i * 8) / DVT;
      const int col = (i * 8) % DVT;
      if (row < c_rows) {
        *reinterpret_cast<bf16x8*>(&L.doc[row][col]) =
            *reinterpret_cast<const bf16x8*>(
                dop + (int64_t)(s0 + row) * kGdnD + v0 + col);
      } else {
        bf16x8 z = {};
        *reinterpret_cast<bf16x8*>(&L.doc[row][col]) = z;
      }
    }
    if (threadIdx.x == 0) {
      float run = 0.f;
      for (int t = 0; t < kGdnC; ++t) {
        if (t < c_rows) run += gp[s0 + t];
        L.gc[t] = run;
        L.beta[t] = (t < c_rows) ? bp[s0 + t] : 0.f;
      }
    }
    for (int i = threadIdx.x; i < kGdnD * DVT; i += 256) {
      const int a = i / DVT;
      const int b = i % DVT;
      L.dsT[b][a] = (bf16_t)L.dS[a][b];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kGdnC * DVT; i += 256) {
      const int t = i / DVT;
      const int d = i % DVT;
      L.doT[d][t] = L.doc[t][d];
    }

    // ---- M (fp32, solve matrix) and N^T (bf16) -------------------------
    {
      f32x4 accm[4], accn[4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        accm[nt] = {0.f, 0.f, 0.f, 0.f};
        accn[nt] = {0.f, 0.f, 0.f, 0.f};
      }
      const int arow = wave * 16 + (lane & 15);
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        const int d0 = ks2 * 32 + (lane >> 4) * 8;
        const bf16x8 ak = *reinterpret_cast<const bf16x8*>(&L.kc[arow][d0]);
        const bf16x8 aq = *reinterpret_cast<const bf16x8*>(&L.qc[arow][d0]);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int brow = nt * 16 + (lane & 15);
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(&L.kc[brow][d0]);
          accm[nt] = mfma16(ak, b, accm[nt]);
          accn[nt] = mfma16(aq, b, accn[nt]);
        }
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = wave * 16 + (lane >> 4) * 4 + r;
          const int j = nt * 16 + (lane & 15);
          const float ratio =
              __builtin_amdgcn_exp2f((L.gc[t] - L.gc[j]) * kLog2eG);
          L.M[t][j] = (j < t) ? L.beta[t] * accm[nt][r] * ratio : 0.f;
          L.nbT[j][t] = (bf16_t)((j <= t) ? accn[nt][r] * ratio : 0.f);
        }
      }
    }
    // wK scratch: ks[t][dk] = K * e^{gc_last - gc_t}
    {
      const float g_tot = L.gc[c_rows - 1];
      for (int i = threadIdx.x; i < kGdnC * kGdnD / 8; i += 256) {
        const int row = (i * 8) / kGdnD;
        const int col = (i * 8) % kGdnD;
        const float sc =
            (row < c_rows)
                ? __builtin_amdgcn_exp2f((g_tot - L.gc[row]) * kLog2eG)
                : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          L.ks[row][col + j] = (bf16_t)((float)L.kc[row][col + j] * sc);
        }
      }
    }
    __syncthreads();

    // ---- dR = wK @ dS + N^T @ dO  (fp32 into L.dx) ---------------------
    {
      f32x4 acc[NTV];
#pragma unroll
      for (int nt = 0; nt < NTV; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
      const int arow = wave * 16 + (lane & 15);
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        const int d0 = ks2 * 32 + (lane >> 4) * 8;
        const bf16x8 aw = *reinterpret_cast<const bf16x8*>(&L.ks[arow][d0]);
        const bf16x8 an = *reinterpret_cast<const bf16x8*>(&L.nbT[arow][d0]);
#pragma unroll
        for (int nt = 0; nt < NTV; ++nt) {
          const int dv = nt * 16 + (lane & 15);
          const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(&L.dsT[dv][d0]);
          const bf16x8 b2 = *reinterpret_cast<const bf16x8*>(&L.doT[dv][d0]);
          acc[nt] = mfma16(aw, b1, acc[nt]);
          acc[nt] = mfma16(an, b2, acc[nt]);
        }
      }
      // wait: nbT rows are A fragments over k = t (the q-row index) —
      // dimensionally N^T is (c x c) with reduction over t' = dO rows; the
      // A fragment of row j needs nbT[j][t' slice] which is exactly
      // L.nbT[arow][d0] with arow = j. Correct as written.
#pragma unroll
      for (int nt = 0; nt < NTV; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = wave * 16 + (lane >> 4) * 4 + r;
          const int dv = nt * 16 + (lane & 15);
          L.dx[t][dv] = acc[nt][r];
        }
      }
    }
    __syncthreads();

    // ---- backward substitution: (I + M)^T drhs = dR, in place ----------
    // drhs[t] = dR[t] - sum_{j > t} M[j][t] * drhs[j]; same 4-way j-split
    // as the forward solve, t walked downward.
    {
      constexpr int CPW = DVT / 4;           // cols per wave
      constexpr int JG = 64 / CPW;           // j groups
      const int c = lane % CPW;
      const int qj = lane / CPW;
      const int col = wave * CPW + c;
      const int jspan = kGdnC / JG;
      for (int t = kGdnC - 2; t >= 0; --t) {
        float part = 0.f;
        const int jlo = max(t + 1, qj * jspan);
        const int jhi = (qj + 1) * jspan;
        for (int j = jlo; j < jhi; ++j) {
          part += L.M[j][t] * L.dx[j][col];
        }
#pragma unroll
        for (int off = CPW; off < 64; off <<= 1) {
          part += __shfl_xor(part, off, 64);
        }
        if (qj == 0) {
          L.dx[t][col] -= part;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();

    // drhs out (fp32)
    for (int i = threadIdx.x; i < kGdnC * DVT; i += 256) {
      const int t = i / DVT;
      const int dv = i % DVT;
      if (t < c_rows) {
        drhs_out[(span.row0 + s0 + t) * kGdnD + v0 + dv] = L.dx[t][dv];
      }
    }

    // ---- dS = e^{g_tot} dS + EK^T @ (-beta drhs) + EQ^T @ dO -----------
    {
      const float g_tot = L.gc[c_rows - 1];
      // ks = e^{gc} K
      for (int i = threadIdx.x; i < kGdnC * kGdnD / 8; i += 256) {
        const int row = (i * 8) / kGdnD;
        const int col = (i * 8) % kGdnD;
        const float sc =
            (row < c_rows) ? __builtin_amdgcn_exp2f(L.gc[row] * kLog2eG) : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          L.ks[row][col + j] = (bf16_t)((float)L.kc[row][col + j] * sc);
        }
      }
      __syncthreads();
      const float e_tot = __builtin_amdgcn_exp2f(g_tot * kLog2eG);
      for (int i = threadIdx.x; i < kGdnD * DVT; i += 256) {
        const int dk = i / DVT;
        const int dv = i % DVT;
        float acc = L.dS[dk][dv] * e_tot;
        for (int t = 0; t < c_rows; ++t) {
          acc -= (float)L.ks[t][dk] * L.beta[t] * L.dx[t][dv];
        }
        L.dS[dk][dv] = acc;
      }
      __syncthreads();
      // ks = e^{gc} Q
      for (int i = threadIdx.x; i < kGdnC * kGdnD / 8; i += 256) {
        const int row = (i * 8) / kGdnD;
        const int col = (i * 8) % kGdnD;
        const float sc =
            (row < c_rows) ? __builtin_amdgcn_exp2f(L.gc[row] * kLog2eG) : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          L.ks[row][col + j] = (bf16_t)((float)L.qc[row][col + j] * sc);
        }
      }
      __syncthreads();
      for (int i = threadIdx.x; i < kGdnD * DVT; i += 256) {
        const int dk = i / DVT;
        const int dv = i % DVT;
        float acc = L.dS[dk][dv];
        for (int t = 0; t < c_rows; ++t) {
          acc += (float)L.ks[t][dk] * (float)L.doc[t][dv];
        }
        L.dS[dk][dv] = acc;
        ds0_out[(span.chunk0 + ch) * (int64_t)kGdnD * kGdnD +
                dk * kGdnD + v0 + dv] = acc;
      }
    }
    __syncthreads();
  }
}

}  // namespace d9d

// ---------------------------------------------------------------------------
// host wrappers
// ---------------------------------------------------------------------------

namespace {

// Packed-document boundaries, checked on the host BEFORE anything is
// launched: the kernels index global memory straight from these values, so
// a bad cu_seqlens must never reach them. The CPU copy also sizes the grid
// (as flash_attn_fwd does for its varlen path).
struct GdnDocs {
  torch::Tensor cu_dev;         // (nseq+1,) int32 on the device
  torch::Tensor chunk_off_dev;  // (nseq+1,) int32: 64-row chunks before doc i
  int64_t nseq = 0;
  int64_t nc = 0;               // chunk_off[nseq]
};

GdnDocs gdn_check_docs(const torch::Tensor& cu_seqlens, int64_t batch,
                       int64_t T, const torch::Device& dev, bool with_chunks) {
  TORCH_CHECK(batch == 1, "packed cu_seqlens input expects batch dim 1, got ",
              batch);
  TORCH_CHECK(cu_seqlens.scalar_type() == torch::kInt32,
              "cu_seqlens must be int32");
  TORCH_CHECK(cu_seqlens.dim() == 1 && cu_seqlens.numel() >= 2,
              "cu_seqlens must be (nseq+1,) with nseq >= 1");
  auto cu_cpu = cu_seqlens.cpu().contiguous();
  const int* cu = cu_cpu.data_ptr<int>();
  GdnDocs d;
  d.nseq = cu_cpu.numel() - 1;
  TORCH_CHECK(cu[0] == 0, "cu_seqlens[0] must be 0, got ", cu[0]);
  for (int64_t i = 0; i < d.nseq; ++i) {
    TORCH_CHECK(cu[i + 1] >= cu[i], "cu_seqlens decreases at entry ", i + 1);
  }
  TORCH_CHECK((int64_t)cu[d.nseq] == T, "cu_seqlens[-1] = ", cu[d.nseq],
              " does not match the ", T, " packed rows");
  d.cu_dev = (cu_seqlens.device() == dev) ? cu_seqlens.contiguous()
                                            : cu_cpu.to(dev);
  if (with_chunks) {
    auto off = torch::empty({d.nseq + 1}, torch::dtype(torch::kInt32));
    int* p = off.data_ptr<int>();
    int total = 0;
    for (int64_t i = 0; i < d.nseq; ++i) {
      p[i] = total;
      total += (cu[i + 1] - cu[i] + d9d::kGdnC - 1) / d9d::kGdnC;
    }
    p[d.nseq] = total;
    d.nc = total;
    d.chunk_off_dev = off.to(dev);
  }
  return d;
}

template <bool VARLEN>
torch::Tensor conv_silu_fwd_impl(const torch::Tensor& x, const torch::Tensor& w,
                                 const int* cu, int nseq) {
  auto xc = x.contiguous();
  auto wc = w.contiguous();
  auto out = torch::empty_like(xc);
  const int64_t B = xc.size(0), S = xc.size(1), C = xc.size(2);
  const int64_t total = B * S * C;
  if (total == 0) return out;
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 8192);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(d9d::causal_conv_silu_fwd_kernel<VARLEN>, dim3(blocks),
                     dim3(256), 0, stream,
                     reinterpret_cast<const __bf16*>(xc.data_ptr()),
                     reinterpret_cast<const __bf16*>(wc.data_ptr()),
                     reinterpret_cast<__bf16*>(out.data_ptr()),
                     cu, nseq, B, S, C, (int)w.size(1));
  return out;
}

template <bool VARLEN>
std::vector<torch::Tensor> conv_silu_bwd_impl(
    const torch::Tensor& x, const torch::Tensor& w, const torch::Tensor& dy,
    const int* cu, int nseq) {
  auto xc = x.contiguous();
  auto wc = w.contiguous();
  auto dyc = dy.contiguous();
  auto dx = torch::empty_like(xc);
  auto dw = torch::zeros(
      {w.size(0), w.size(1)},
      torch::dtype(torch::kFloat32).device(w.device()));
  const int64_t B = xc.size(0), S = xc.size(1), C = xc.size(2);
  const int64_t total = B * S * C;
  if (total == 0) return {dx, dw.to(w.scalar_type())};
  const int blocks = (int)std::min<int64_t>((total + 255) / 256, 8192);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(d9d::causal_conv_silu_bwd_kernel<VARLEN>, dim3(blocks),
                     dim3(256), 0, stream,
                     reinterpret_cast<const __bf16*>(xc.data_ptr()),
                     reinterpret_cast<const __bf16*>(wc.data_ptr()),
                     reinterpret_cast<const __bf16*>(dyc.data_ptr()),
                     reinterpret_cast<__bf16*>(dx.data_ptr()),
                     dw.data_ptr<float>(), cu, nseq, B, S, C, (int)w.size(1));
  return {dx, dw.to(w.scalar_type())};
}

void conv_varlen_checks(const torch::Tensor& x, const torch::Tensor& w) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(x.dim() == 3 && w.dim() == 2 && w.size(0) == x.size(2),
              "expected x (1, T, C) and w (C, K)");
  TORCH_CHECK(w.size(1) <= 4, "conv kernel must be <= 4");
}

// dense conv backward: x, dy (B, S, C) and w (C, K), all bf16 on the device
void conv_bwd_checks(const torch::Tensor& x, const torch::Tensor& w,
                     const torch::Tensor& dy) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16,
              "causal_conv_silu_bwd: x must be a bf16 device tensor");
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16,
              "causal_conv_silu_bwd: w must be a bf16 device tensor");
  TORCH_CHECK(x.dim() == 3 && w.dim() == 2 && w.size(0) == x.size(2),
              "causal_conv_silu_bwd: expected x (B, S, C) and w (C, K)");
  TORCH_CHECK(w.size(1) >= 1 && w.size(1) <= 4,
              "causal_conv_silu_bwd: conv kernel must be <= 4");
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == torch::kBFloat16 &&
                  dy.sizes() == x.sizes(),
              "causal_conv_silu_bwd: dy must match x");
}

// Dv-split rule shared by every chunk launch: below ~1.5 workgroups/CU the
// duplicated K-side work is cheaper than idle CUs.
bool gdn_split_dv(int64_t n_wg) { return n_wg * 2 <= 384; }

template <bool VARLEN>
void gdn_fwd_launch(int64_t n_wg, int64_t S, const torch::Tensor& q,
                    const torch::Tensor& k, const torch::Tensor& v,
                    const torch::Tensor& beta, const torch::Tensor& g,
                    __bf16* out, float* fs, float* r, float* s0,
                    const int* cu, const int* chunk_off, int H, int64_t nc) {
  static bool attr_set = false;
  if (!attr_set) {
    hipFuncSetAttribute(
        reinterpret_cast<const void*>(&d9d::gdn_chunk_fwd_kernel<64, VARLEN>),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)sizeof(d9d::GdnLds<64>));
    hipFuncSetAttribute(
        reinterpret_cast<const void*>(&d9d::gdn_chunk_fwd_kernel<32, VARLEN>),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)sizeof(d9d::GdnLds<32>));
    attr_set = true;
  }
  auto stream = at::hip::getCurrentHIPStream();
  if (gdn_split_dv(n_wg)) {
    hipLaunchKernelGGL((d9d::gdn_chunk_fwd_kernel<32, VARLEN>),
                       dim3((unsigned)n_wg, 2), dim3(256),
                       sizeof(d9d::GdnLds<32>), stream,
                       reinterpret_cast<const __bf16*>(q.data_ptr()),
                       reinterpret_cast<const __bf16*>(k.data_ptr()),
                       reinterpret_cast<const __bf16*>(v.data_ptr()),
                       beta.data_ptr<float>(), g.data_ptr<float>(),
                       out, fs, r, s0, n_wg, S, cu, chunk_off, H, nc);
  } else {
    hipLaunchKernelGGL((d9d::gdn_chunk_fwd_kernel<64, VARLEN>),
                       dim3((unsigned)n_wg, 1), dim3(256),
                       sizeof(d9d::GdnLds<64>), stream,
                       reinterpret_cast<const __bf16*>(q.data_ptr()),
                       reinterpret_cast<const __bf16*>(k.data_ptr()),
                       reinterpret_cast<const __bf16*>(v.data_ptr()),
                       beta.data_ptr<float>(), g.data_ptr<float>(),
                       out, fs, r, s0, n_wg, S, cu, chunk_off, H, nc);
  }
}

template <bool VARLEN>
void gdn_bwd_scan_launch(int64_t n_wg, int64_t S, const torch::Tensor& q,
                         const torch::Tensor& k, const torch::Tensor& dout,
                         const torch::Tensor& beta, const torch::Tensor& g,
                         float* drhs, float* ds0, const int* cu,
                         const int* chunk_off, int H, int64_t nc) {
  static bool attr_set = false;
  if (!attr_set) {
    hipFuncSetAttribute(
        reinterpret_cast<const void*>(
            &d9d::gdn_chunk_bwd_scan_kernel<64, VARLEN>),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)sizeof(d9d::GdnBwdLds<64>));
    hipFuncSetAttribute(
        reinterpret_cast<const void*>(
            &d9d::gdn_chunk_bwd_scan_kernel<32, VARLEN>),
        hipFuncAttributeMaxDynamicSharedMemorySize,
        (int)sizeof(d9d::GdnBwdLds<32>));
    attr_set = true;
  }
  auto stream = at::hip::getCurrentHIPStream();
  // same Dv-split heuristic as the forward kernel
  if (gdn_split_dv(n_wg)) {
    hipLaunchKernelGGL((d9d::gdn_chunk_bwd_scan_kernel<32, VARLEN>),
                       dim3((unsigned)n_wg, 2), dim3(256),
                       sizeof(d9d::GdnBwdLds<32>), stream,
                       reinterpret_cast<const __bf16*>(q.data_ptr()),
                       reinterpret_cast<const __bf16*>(k.data_ptr()),
                       reinterpret_cast<const __bf16*>(dout.data_ptr()),
                       beta.data_ptr<float>(), g.data_ptr<float>(),
                       drhs, ds0, n_wg, S, cu, chunk_off, H, nc);
  } else {
    hipLaunchKernelGGL((d9d::gdn_chunk_bwd_scan_kernel<64, VARLEN>),
                       dim3((unsigned)n_wg, 1), dim3(256),
                       sizeof(d9d::GdnBwdLds<64>), stream,
                       reinterpret_cast<const __bf16*>(q.data_ptr()),
                       reinterpret_cast<const __bf16*>(k.data_ptr()),
                       reinterpret_cast<const __bf16*>(dout.data_ptr()),
                       beta.data_ptr<float>(), g.data_ptr<float>(),
                       drhs, ds0, n_wg, S, cu, chunk_off, H, nc);
  }
}

// dense entry points: (B, H, S, 64) bf16 rows + (B, H, S) gates
void gdn_dense_checks(const char* who, const torch::Tensor& q,
                      const torch::Tensor& k, const torch::Tensor& v,
                      const torch::Tensor& beta,
                      const torch::Tensor& decay_log) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == torch::kBFloat16, who,
              ": q must be a bf16 device tensor");
  TORCH_CHECK(k.is_cuda() && k.scalar_type() == torch::kBFloat16, who,
              ": k must be a bf16 device tensor");
  TORCH_CHECK(v.is_cuda() && v.scalar_type() == torch::kBFloat16, who,
              ": v / dout must be a bf16 device tensor");
  TORCH_CHECK(q.dim() == 4 && q.size(-1) == 64, who,
              " supports (B, H, S, 64)");
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes(), who,
              ": q, k, v / dout must share one (B, H, S, 64) shape");
  TORCH_CHECK(beta.is_cuda() && decay_log.is_cuda(), who,
              ": beta and decay_log must be device tensors");
  TORCH_CHECK(beta.dim() == 3 && beta.size(0) == q.size(0) &&
                  beta.size(1) == q.size(1) && beta.size(2) == q.size(2) &&
                  decay_log.sizes() == beta.sizes(),
              who, ": beta and decay_log must be (B, H, S)");
}

// (1, H, T, 64) bf16 rows + (1, H, T) gates of one packed row
void gdn_varlen_checks(const torch::Tensor& q, const torch::Tensor& k,
                       const torch::Tensor& v, const torch::Tensor& beta,
                       const torch::Tensor& decay_log) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(k.is_cuda() && k.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(v.is_cuda() && v.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(q.dim() == 4 && q.size(-1) == 64,
              "gdn varlen kernels support (1, H, T, 64)");
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes(),
              "q, k, v / dout must share one (1, H, T, 64) shape");
  TORCH_CHECK(beta.is_cuda() && decay_log.is_cuda());
  TORCH_CHECK(beta.dim() == 3 && beta.size(0) == q.size(0) &&
                  beta.size(1) == q.size(1) && beta.size(2) == q.size(2) &&
                  decay_log.sizes() == beta.sizes(),
              "beta and decay_log must be (1, H, T)");
}

}  // namespace

torch::Tensor causal_conv_silu_fwd(torch::Tensor x, torch::Tensor w) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(w.size(1) <= 4, "conv kernel must be <= 4");
  return conv_silu_fwd_impl<false>(x, w, nullptr, 0);
}

std::vector<torch::Tensor> causal_conv_silu_bwd(
    torch::Tensor x, torch::Tensor w, torch::Tensor dy) {
  conv_bwd_checks(x, w, dy);
  return conv_silu_bwd_impl<false>(x, w, dy, nullptr, 0);
}

torch::Tensor causal_conv_silu_varlen_fwd(torch::Tensor x, torch::Tensor w,
                                          torch::Tensor cu_seqlens) {
  conv_varlen_checks(x, w);
  auto docs = gdn_check_docs(cu_seqlens, x.size(0), x.size(1), x.device(),
                             /*with_chunks=*/false);
  return conv_silu_fwd_impl<true>(x, w, docs.cu_dev.data_ptr<int>(),
                                  (int)docs.nseq);
}

std::vector<torch::Tensor> causal_conv_silu_varlen_bwd(
    torch::Tensor x, torch::Tensor w, torch::Tensor dy,
    torch::Tensor cu_seqlens) {
  conv_varlen_checks(x, w);
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == torch::kBFloat16 &&
                  dy.sizes() == x.sizes(),
              "dy must match x");
  auto docs = gdn_check_docs(cu_seqlens, x.size(0), x.size(1), x.device(),
                             /*with_chunks=*/false);
  return conv_silu_bwd_impl<true>(x, w, dy, docs.cu_dev.data_ptr<int>(),
                                  (int)docs.nseq);
}

std::vector<torch::Tensor> gdn_chunk_bwd_scan(
    torch::Tensor q, torch::Tensor k, torch::Tensor dout,
    torch::Tensor beta, torch::Tensor decay_log) {
  gdn_dense_checks("gdn_chunk_bwd_scan", q, k, dout, beta, decay_log);
  auto qc = q.contiguous();
  auto kc = k.contiguous();
  auto dc = dout.contiguous();
  auto bc = beta.to(torch::kFloat32).contiguous();
  auto gc = decay_log.to(torch::kFloat32).contiguous();
  const int64_t B = qc.size(0), H = qc.size(1), S = qc.size(2);
  const int64_t nc = (S + 63) / 64;
  auto f32 = torch::dtype(torch::kFloat32).device(q.device());
  auto drhs = torch::empty({B, H, S, 64}, f32);
  auto ds0 = torch::empty({B, H, nc, 64, 64}, f32);
  gdn_bwd_scan_launch<false>(B * H, S, qc, kc, dc, bc, gc,
                             drhs.data_ptr<float>(), ds0.data_ptr<float>(),
                             nullptr, nullptr, 0, 0);
  return {drhs, ds0};
}

std::vector<torch::Tensor> gdn_chunk_bwd_scan_varlen(
    torch::Tensor q, torch::Tensor k, torch::Tensor dout,
    torch::Tensor beta, torch::Tensor decay_log, torch::Tensor cu_seqlens) {
  gdn_varlen_checks(q, k, dout, beta, decay_log);
  const int64_t H = q.size(1), T = q.size(2);
  auto docs = gdn_check_docs(cu_seqlens, q.size(0), T, q.device(),
                             /*with_chunks=*/true);
  auto qc = q.contiguous();
  auto kc = k.contiguous();
  auto dc = dout.contiguous();
  auto bc = beta.to(torch::kFloat32).contiguous();
  auto gc = decay_log.to(torch::kFloat32).contiguous();
  auto f32 = torch::dtype(torch::kFloat32).device(q.device());
  auto drhs = torch::empty({1, H, T, 64}, f32);
  auto ds0 = torch::empty({1, H, docs.nc, 64, 64}, f32);
  gdn_bwd_scan_launch<true>(docs.nseq * H, T, qc, kc, dc, bc, gc,
                            drhs.data_ptr<float>(), ds0.data_ptr<float>(),
                            docs.cu_dev.data_ptr<int>(),
                            docs.chunk_off_dev.data_ptr<int>(), (int)H,
                            docs.nc);
  return {drhs, ds0};
}

namespace {

// Output allocation + launch shared by the dense and packed forward:
// `n_state` workgroups (B*H, or nseq*H) each own one final state.
template <bool VARLEN>
std::vector<torch::Tensor> gdn_chunk_fwd_impl(
    const torch::Tensor& q, const torch::Tensor& k, const torch::Tensor& v,
    const torch::Tensor& beta, const torch::Tensor& decay_log,
    bool return_state, bool return_aux, bool skip_out,
    std::vector<int64_t> state_lead, int64_t nc, const int* cu,
    const int* chunk_off) {
  auto qc = q.contiguous();
  auto kc = k.contiguous();
  auto vc = v.contiguous();
  auto bc = beta.to(torch::kFloat32).contiguous();
  auto gc = decay_log.to(torch::kFloat32).contiguous();
  const int64_t B = qc.size(0), H = qc.size(1), S = qc.size(2);
  auto out = skip_out ? torch::Tensor() : torch::empty_like(vc);
  __bf16* out_ptr =
      skip_out ? nullptr : reinterpret_cast<__bf16*>(out.data_ptr());
  auto f32 = torch::dtype(torch::kFloat32).device(q.device());
  torch::Tensor fs;
  float* fs_ptr = nullptr;
  if (return_state) {
    fs = torch::empty({state_lead[0], state_lead[1], 64, 64}, f32);
    fs_ptr = fs.data_ptr<float>();
  }
  // aux outputs for the hand-derived backward: per-row solve results R and
  // the per-chunk entry states S0
  torch::Tensor r_aux, s0_aux;
  float* r_ptr = nullptr;
  float* s0_ptr = nullptr;
  if (return_aux) {
    r_aux = torch::empty({B, H, S, 64}, f32);
    s0_aux = torch::empty({B, H, nc, 64, 64}, f32);
    r_ptr = r_aux.data_ptr<float>();
    s0_ptr = s0_aux.data_ptr<float>();
  }
  gdn_fwd_launch<VARLEN>(state_lead[0] * state_lead[1], S, qc, kc, vc, bc, gc,
                         out_ptr, fs_ptr, r_ptr, s0_ptr, cu, chunk_off, (int)H,
                         nc);
  std::vector<torch::Tensor> outs;
  if (!skip_out) outs.push_back(out);
  if (return_state) outs.push_back(fs);
  if (return_aux) {
    outs.push_back(r_aux);
    outs.push_back(s0_aux);
  }
  return outs;
}

}  // namespace

std::vector<torch::Tensor> gdn_chunk_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor beta, torch::Tensor decay_log, bool return_state,
    bool return_aux, bool skip_out) {
  gdn_dense_checks("gdn_chunk_fwd", q, k, v, beta, decay_log);
  return gdn_chunk_fwd_impl<false>(
      q, k, v, beta, decay_log, return_state, return_aux, skip_out,
      {q.size(0), q.size(1)}, (q.size(2) + 63) / 64, nullptr, nullptr);
}

// Packed documents: q, k, v (1, H, T, 64), one workgroup per (document,
// head), zero state at each document start. Final state (nseq, H, 64, 64);
// aux r (1, H, T, 64) by packed row, s0 (1, H, NC, 64, 64) by
// chunk_off[doc] + local chunk.
std::vector<torch::Tensor> gdn_chunk_fwd_varlen(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor beta, torch::Tensor decay_log, torch::Tensor cu_seqlens,
    bool return_state, bool return_aux, bool skip_out) {
  gdn_varlen_checks(q, k, v, beta, decay_log);
  auto docs = gdn_check_docs(cu_seqlens, q.size(0), q.size(2), q.device(),
                             /*with_chunks=*/true);
  return gdn_chunk_fwd_impl<true>(
      q, k, v, beta, decay_log, return_state, return_aux, skip_out,
      {docs.nseq, q.size(1)}, docs.nc, docs.cu_dev.data_ptr<int>(),
      docs.chunk_off_dev.data_ptr<int>());
}
