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
// 3. The hand-derived backward (gated_deltanet.py _chunk_gdn_backward):
//    gdn_chunk_fwd with aux outputs recomputes R and the chunk entry
//    states, gdn_chunk_bwd_scan walks the chunks backward with dL/dState
//    in LDS, and gdn_chunk_bwd_leaf turns both into dq, dk, dv, dbeta, dg,
//    one workgroup per chunk.
// 4. Packed-document (cu_seqlens) variants of every entry point: the
//    same kernel bodies under a VARLEN template flag — one workgroup per
//    (document, head) from a zero state, conv taps clipped at the
//    document start; the leaf kernel takes a last-chunk-of-document flag.
//    cu_seqlens is validated on the host before launch.
// 5. Dk = Dv = 128 variants of the forward (with its aux outputs), the
//    reverse scan and the leaf gradients, dense and packed: 8-wave
//    workgroups, the scans with the fp32 state in registers, the leaf kernel
//    with full-size operand images in 158 KB of LDS (the `wide` sections
//    below).
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
// the non-sequential leaf gradients are gdn_chunk_bwd_leaf_kernel below.
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

// ---------------------------------------------------------------------------
// chunked gated delta rule backward LEAF GRADIENTS, Dk = Dv = 64
// ---------------------------------------------------------------------------
//
// The non-sequential half of _chunk_gdn_backward: everything after the two
// scans is local to one chunk, so one workgroup (4 waves) per (b, h, chunk)
// turns (q, k, v, dO, beta, g, R, drhs, S0, dS1) into dq, dk, dv, dbeta, dg
// of its 64 rows. dS1 is ds0 of the NEXT chunk, zero for the last chunk of a
// row (dense) or of a document (`doc_last`, packed layout of whole chunks).
// With t the row, j the column of the 64x64 chunk matrices (E = e^{gc},
// w = e^{gc_63 - gc}, ratio = tril0(e^{gc_t - gc_j}), kk = K K^T, qk = Q K^T):
//   dwK = R dS1^T            dK  = w dwK            dw = rowsum(dwK * K)
//   dEQ = dO S0^T            dQ  = E dEQ
//   G   = drhs S0^T          dK += -beta E G        (dEK = -beta G)
//   dN  = tril0(dO R^T)      dqk = dN ratio
//   dM  = -tril-1(drhs R^T)  dkk = beta dM ratio
//   dQ += dqk K              dK += dqk^T Q + dkk K + dkk^T K
//   dV  = beta drhs
//   dbeta = rowsum(dM kk ratio) + rowsum(drhs * V) - E rowsum(G * K)
//   rr  = (dN qk + beta dM kk) ratio
//   dgc = -w dw + E rowsum(dEQ * Q) - beta E rowsum(G * K)
//         + rowsum(rr) - colsum(rr);   dgc_63 += <dS1, S0> e^{gc_63} + sum(w dw)
//   dg  = reverse cumsum of dgc inside the chunk
// rowsum(drhs * P), P = V - (E K) S0, is taken as rowsum(drhs * V) -
// E rowsum(G * K): the same sum reassociated through G, so the (E K) S0
// product and a transposed image of S0 are never needed.
//
// Work split: wave w owns rows 16w..16w+15 of every product. Its A fragments
// (rows of R, dO, drhs, Q) come straight from global memory: each element
// is read by exactly one lane. B operands are shared by the four waves and
// staged once into LDS: K rows, K^T and Q^T images, and two hi/lo image
// pairs that are reused in phases (`a`: R -> dqk -> dkk; `b`: dS1 -> S0 ->
// dqk^T -> dkk^T), which keeps the workgroup at ~66 KB, two per CU. kk, qk,
// ratio, dN and dM live in accumulator registers only.
//
// Rounding: q, k, v, dO are bf16 inputs. Every fp32 operand of a product
// (R, drhs, S0, dS1, dqk, dkk) goes to the MFMA as a bf16 pair hi = bf16(x),
// lo = bf16(x - hi) with all hi/lo cross terms accumulated in fp32, i.e. it
// is truncated to ~16 significant bits (2^-17 relative) at the point where
// it is staged or written to an image; nothing is rounded once to bf16.
// All sums, decay factors and elementwise math are fp32.
constexpr int kLeafP = kGdnD + 8;   // LDS row pitch: 144 B rows spread the
                                    // 16 B fragment reads over the banks
typedef bf16_t LeafTile[kGdnC][kLeafP];

struct GdnLeafLds {
  LeafTile kc;                    // K rows        (B of kk, qk; A of kk)
  LeafTile kT;                    // K^T: kT[d][t] (B of . K; K in C layout)
  LeafTile qT;                    // Q^T: qT[d][t] (B of . Q; Q in C layout)
  LeafTile a[2];                  // hi/lo: R, then dqk, then dkk
  LeafTile b[2];                  // hi/lo: dS1, then S0, then dqk^T, dkk^T
  float gc[kGdnC];
  float beta[kGdnC];
  float dgc[kGdnC];               // row-owned part of dgc
  float db[kGdnC];                // C-layout part of dbeta
  float dbv[kGdnC];               // rowsum(drhs * V)
  float colsum[4][kGdnC];         // per-wave colsum(rr)
  float red[4];                   // per-wave part of the dgc_63 scalar
};

// The leaf kernel is built without packed fp32 VALU ops (target attribute
// below), and only force-inlined code follows a kernel's target: barrier and
// lane exchange are spelled with the builtins here.
D9D_DEVICE void leaf_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// value of `x` in lane `src` (taken mod 64) of this wave
D9D_DEVICE float leaf_shfl(float x, int src) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(src << 2, __builtin_bit_cast(int, x)));
}

D9D_DEVICE void leaf_split(float x, bf16_t& hi, bf16_t& lo) {
  hi = (bf16_t)x;
  lo = (bf16_t)(x - (float)hi);
}

D9D_DEVICE void leaf_load8(const float* __restrict__ p, float (&x)[8]) {
  const float4 x0 = *reinterpret_cast<const float4*>(p);
  const float4 x1 = *reinterpret_cast<const float4*>(p + 4);
  x[0] = x0.x; x[1] = x0.y; x[2] = x0.z; x[3] = x0.w;
  x[4] = x1.x; x[5] = x1.y; x[6] = x1.z; x[7] = x1.w;
}

D9D_DEVICE void leaf_split8(const float (&x)[8], bf16x8& hi, bf16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    bf16_t h, l;
    leaf_split(x[j], h, l);
    hi[j] = h;
    lo[j] = l;
  }
}

// acc (this wave's 16 x 64 band) += A . B^T-image: A fragments a[ks2][image]
// (NA = 2: hi/lo), B rows b[image][n][k] (NB = 2: hi/lo). Cross terms run
// smallest first.
template <int NA, int NB>
D9D_DEVICE void leaf_mma(f32x4 (&acc)[4], const bf16x8 (&a)[2][NA],
                         const LeafTile* b, int lane) {
#pragma unroll
  for (int ks2 = 0; ks2 < 2; ++ks2) {
    const int d0 = ks2 * 32 + (lane >> 4) * 8;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int brow = nt * 16 + (lane & 15);
#pragma unroll
      for (int ib = NB - 1; ib >= 0; --ib) {
        const bf16x8 bf = *reinterpret_cast<const bf16x8*>(&b[ib][brow][d0]);
#pragma unroll
        for (int ia = NA - 1; ia >= 0; --ia) {
          acc[nt] = mfma16(a[ks2][ia], bf, acc[nt]);
        }
      }
    }
  }
}

// hi/lo A fragments of row `arow` of an LDS image pair
D9D_DEVICE void leaf_afrag(bf16x8 (&a)[2][2], const LeafTile* img, int arow,
                           int lane) {
#pragma unroll
  for (int ks2 = 0; ks2 < 2; ++ks2) {
    const int d0 = ks2 * 32 + (lane >> 4) * 8;
    a[ks2][0] = *reinterpret_cast<const bf16x8*>(&img[0][arow][d0]);
    a[ks2][1] = *reinterpret_cast<const bf16x8*>(&img[1][arow][d0]);
  }
}

// This wave's band of a C-layout fp32 tile -> hi/lo images img[t][j] and
// imgT[j][t] (a lane's four rows are one 8-byte store of the transpose).
D9D_DEVICE void leaf_put(const f32x4 (&x)[4], LeafTile* img, LeafTile* imgT,
                         int tq, int lane) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int j = nt * 16 + (lane & 15);
    bf16x4 h4, l4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bf16_t h, l;
      leaf_split(x[nt][r], h, l);
      img[0][tq + r][j] = h;
      img[1][tq + r][j] = l;
      h4[r] = h;
      l4[r] = l;
    }
    *reinterpret_cast<bf16x4*>(&imgT[0][j][tq]) = h4;
    *reinterpret_cast<bf16x4*>(&imgT[1][j][tq]) = l4;
  }
}

// (built without packed fp32 VALU ops: plain v_mul / v_fma only)
__global__ __launch_bounds__(256, 2)
__attribute__((target("no-packed-fp32-ops"))) void gdn_chunk_bwd_leaf_kernel(
    const bf16_t* __restrict__ q,    // (B, H, Sp, D), Sp = 64 nc
    const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ dout,
    const float* __restrict__ beta,       // (B, H, Sp)
    const float* __restrict__ decay_log,  // (B, H, Sp)
    const float* __restrict__ r_in,       // (B, H, Sp, D)  gdn_chunk_fwd aux
    const float* __restrict__ drhs,       // (B, H, Sp, D)  reverse scan
    const float* __restrict__ s0,         // (B, H, nc, D, D)
    const float* __restrict__ ds0,        // (B, H, nc, D, D)
    float* __restrict__ dq,               // (B, H, Sp, D)
    float* __restrict__ dk,
    float* __restrict__ dv,
    float* __restrict__ dbeta,            // (B, H, Sp)
    float* __restrict__ dg,
    const int* __restrict__ doc_last,     // (nc,) packed rows only, or nullptr
    int64_t n_chunks, int64_t nc) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  GdnLeafLds& L = *reinterpret_cast<GdnLeafLds*>(smem_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int lr = lane & 15;
  const int lq = lane >> 4;
  const int64_t chunk = blockIdx.x;
  if (chunk >= n_chunks) return;
  const int64_t c = chunk % nc;
  // the last chunk of a row / document hands its state to nobody: dS1 = 0
  // (and ds0[chunk + 1] is never addressed past the end of a row)
  const bool last = (c == nc - 1) || (doc_last != nullptr && doc_last[c] != 0);
  const int64_t row0 = chunk * kGdnC;
  const int64_t tile0 = row0 * kGdnD;
  const float* s0p = s0 + chunk * (int64_t)(kGdnD * kGdnD);
  const float* ds1p = ds0 + (chunk + 1) * (int64_t)(kGdnD * kGdnD);

  // ---- stage: decay scan, K / K^T / Q^T, R and dS1 images; S0 to registers
  if (wave == 0) {
    float run = decay_log[row0 + lane];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float up = leaf_shfl(run, lane - off);
      if (lane >= off) run += up;
    }
    L.gc[lane] = run;
    L.beta[lane] = beta[row0 + lane];
  }
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = tid + u * 256;
    const int row = i >> 3;
    const int col = (i & 7) * 8;
    const bf16x8 kv =
        *reinterpret_cast<const bf16x8*>(k + tile0 + row * kGdnD + col);
    const bf16x8 qv =
        *reinterpret_cast<const bf16x8*>(q + tile0 + row * kGdnD + col);
    *reinterpret_cast<bf16x8*>(&L.kc[row][col]) = kv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      L.kT[col + j][row] = kv[j];
      L.qT[col + j][row] = qv[j];
    }
  }
  float4 s0r[4];
  float frob = 0.f;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = tid + u * 256;
    const int row = i >> 4;
    const int col = (i & 15) * 4;
    const float4 rv = *reinterpret_cast<const float4*>(
        r_in + tile0 + row * kGdnD + col);
    const float rx[4] = {rv.x, rv.y, rv.z, rv.w};
    bf16x4 h4, l4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16_t h, l;
      leaf_split(rx[j], h, l);
      h4[j] = h;
      l4[j] = l;
    }
    *reinterpret_cast<bf16x4*>(&L.a[0][row][col]) = h4;
    *reinterpret_cast<bf16x4*>(&L.a[1][row][col]) = l4;
    s0r[u] = *reinterpret_cast<const float4*>(s0p + row * kGdnD + col);
    if (!last) {
      const float4 dv4 =
          *reinterpret_cast<const float4*>(ds1p + row * kGdnD + col);
      const float dx[4] = {dv4.x, dv4.y, dv4.z, dv4.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        bf16_t h, l;
        leaf_split(dx[j], h, l);
        h4[j] = h;
        l4[j] = l;
      }
      *reinterpret_cast<bf16x4*>(&L.b[0][row][col]) = h4;
      *reinterpret_cast<bf16x4*>(&L.b[1][row][col]) = l4;
      frob += dv4.x * s0r[u].x + dv4.y * s0r[u].y + dv4.z * s0r[u].z +
              dv4.w * s0r[u].w;
    }
  }
  leaf_barrier();

  // this lane's rows in the C layout: tq .. tq+3; A fragments: row arow
  const int tq = wave * 16 + lq * 4;
  const int arow = wave * 16 + lr;
  const int64_t aoff = tile0 + arow * kGdnD + lq * 8;   // + ks2 * 32
  const float g_end = L.gc[kGdnC - 1];
  const float e_end = expf(g_end);
  float gct[4], et[4], wt[4], bt[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    gct[r] = L.gc[tq + r];
    et[r] = expf(gct[r]);
    wt[r] = expf(g_end - gct[r]);
    bt[r] = L.beta[tq + r];
  }

  f32x4 dqa[4], dka[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    dqa[nt] = {0.f, 0.f, 0.f, 0.f};
    dka[nt] = {0.f, 0.f, 0.f, 0.f};
  }
  float rowacc[4] = {0.f, 0.f, 0.f, 0.f};   // dgc partial of rows tq..tq+3
  float dbacc[4] = {0.f, 0.f, 0.f, 0.f};    // dbeta partial of the same rows
  float tot = frob * e_end;                 // dgc_63 scalar partial

  // ---- dwK = R dS1^T: dK = w dwK, dw = rowsum(dwK * K) -------------------
  if (!last) {
    bf16x8 ar[2][2];
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      float x[8];
      leaf_load8(r_in + aoff + ks2 * 32, x);
      leaf_split8(x, ar[ks2][0], ar[ks2][1]);
    }
    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
    leaf_mma<2, 2>(acc, ar, L.b, lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const bf16x4 kf =
          *reinterpret_cast<const bf16x4*>(&L.kT[nt * 16 + lr][tq]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float dkw = acc[nt][r] * wt[r];
        dka[nt][r] = dkw;
        const float p = dkw * (float)kf[r];
        rowacc[r] -= p;
        tot += p;
      }
    }
  }
  leaf_barrier();   // dS1 image consumed: S0 takes its place
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = tid + u * 256;
    const int row = i >> 4;
    const int col = (i & 15) * 4;
    const float sx[4] = {s0r[u].x, s0r[u].y, s0r[u].z, s0r[u].w};
    bf16x4 h4, l4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16_t h, l;
      leaf_split(sx[j], h, l);
      h4[j] = h;
      l4[j] = l;
    }
    *reinterpret_cast<bf16x4*>(&L.b[0][row][col]) = h4;
    *reinterpret_cast<bf16x4*>(&L.b[1][row][col]) = l4;
  }

  // A fragments of dO and drhs (kept for the R^T products); on the way
  // dV = beta drhs and rowsum(drhs * V) for dbeta
  bf16x8 ado[2][1], adr[2][2];
  {
    const float ba = L.beta[arow];
    float dot = 0.f;
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const int64_t off = aoff + ks2 * 32;
      ado[ks2][0] = *reinterpret_cast<const bf16x8*>(dout + off);
      const bf16x8 vv = *reinterpret_cast<const bf16x8*>(v + off);
      float x[8];
      leaf_load8(drhs + off, x);
      leaf_split8(x, adr[ks2][0], adr[ks2][1]);
#pragma unroll
      for (int j = 0; j < 8; ++j) dot += x[j] * (float)vv[j];
      *reinterpret_cast<f32x4*>(dv + off) =
          f32x4{ba * x[0], ba * x[1], ba * x[2], ba * x[3]};
      *reinterpret_cast<f32x4*>(dv + off + 4) =
          f32x4{ba * x[4], ba * x[5], ba * x[6], ba * x[7]};
    }
    dot += leaf_shfl(dot, lane ^ 16);
    dot += leaf_shfl(dot, lane ^ 32);
    if (lq == 0) L.dbv[arow] = dot;
  }
  leaf_barrier();

  // ---- dEQ = dO S0^T: dQ = E dEQ, dgc += E rowsum(dEQ * Q) ---------------
  {
    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
    leaf_mma<1, 2>(acc, ado, L.b, lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const bf16x4 qf =
          *reinterpret_cast<const bf16x4*>(&L.qT[nt * 16 + lr][tq]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = acc[nt][r] * et[r];
        dqa[nt][r] = e;
        rowacc[r] += e * (float)qf[r];
      }
    }
  }
  // ---- G = drhs S0^T: dK -= beta E G, dgc -= beta E rowsum(G * K),
  //      dbeta -= E rowsum(G * K) -----------------------------------------
  {
    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
    leaf_mma<2, 2>(acc, adr, L.b, lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const bf16x4 kf =
          *reinterpret_cast<const bf16x4*>(&L.kT[nt * 16 + lr][tq]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ge = acc[nt][r] * et[r];
        const float gk = ge * (float)kf[r];
        dka[nt][r] -= bt[r] * ge;
        rowacc[r] -= bt[r] * gk;
        dbacc[r] -= gk;
      }
    }
  }

  // ---- dN, dM, kk, qk in registers -> dqk (x), dkk (y), dbeta, rr sums ---
  f32x4 x[4], y[4];
  {
    f32x4 an[4], am[4], akk[4], aqk[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      an[nt] = {0.f, 0.f, 0.f, 0.f};
      am[nt] = {0.f, 0.f, 0.f, 0.f};
      akk[nt] = {0.f, 0.f, 0.f, 0.f};
      aqk[nt] = {0.f, 0.f, 0.f, 0.f};
    }
    bf16x8 ak[2][1], aq[2][1];
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      ak[ks2][0] =
          *reinterpret_cast<const bf16x8*>(&L.kc[arow][ks2 * 32 + lq * 8]);
      aq[ks2][0] = *reinterpret_cast<const bf16x8*>(q + aoff + ks2 * 32);
    }
    leaf_mma<1, 2>(an, ado, L.a, lane);
    leaf_mma<2, 2>(am, adr, L.a, lane);
    leaf_mma<1, 1>(akk, ak, &L.kc, lane);
    leaf_mma<1, 1>(aqk, aq, &L.kc, lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int j = nt * 16 + lr;
      const float gcj = L.gc[j];
      float colacc = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = tq + r;
        // decay ratio only where t >= j, so it stays <= 1
        const float ratio = (j <= t) ? expf(gct[r] - gcj) : 0.f;
        const float dn = (j <= t) ? an[nt][r] : 0.f;
        const float dm = (j < t) ? -am[nt][r] : 0.f;
        const float dkkr = dm * bt[r];
        dbacc[r] += dm * akk[nt][r] * ratio;
        const float rr = (dn * aqk[nt][r] + dkkr * akk[nt][r]) * ratio;
        rowacc[r] += rr;
        colacc += rr;
        x[nt][r] = dn * ratio;
        y[nt][r] = dkkr * ratio;
      }
      colacc += leaf_shfl(colacc, lane ^ 16);
      colacc += leaf_shfl(colacc, lane ^ 32);
      if (lq == 0) L.colsum[wave][j] = colacc;
    }
  }
  leaf_barrier();   // R and S0 images consumed

  // ---- dQ += dqk K, dK += dqk^T Q ----------------------------------------
  leaf_put(x, L.a, L.b, tq, lane);
  leaf_barrier();
  {
    bf16x8 af[2][2];
    leaf_afrag(af, L.a, arow, lane);
    leaf_mma<2, 1>(dqa, af, &L.kT, lane);
    leaf_afrag(af, L.b, arow, lane);
    leaf_mma<2, 1>(dka, af, &L.qT, lane);
  }
  leaf_barrier();

  // ---- dK += dkk K + dkk^T K ---------------------------------------------
  leaf_put(y, L.a, L.b, tq, lane);
  leaf_barrier();
  {
    bf16x8 af[2][2];
    leaf_afrag(af, L.a, arow, lane);
    leaf_mma<2, 1>(dka, af, &L.kT, lane);
    leaf_afrag(af, L.b, arow, lane);
    leaf_mma<2, 1>(dka, af, &L.kT, lane);
  }

  // ---- outputs -----------------------------------------------------------
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t off = tile0 + (tq + r) * kGdnD + nt * 16 + lr;
      dq[off] = dqa[nt][r];
      dk[off] = dka[nt][r];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      rowacc[r] += leaf_shfl(rowacc[r], lane ^ off);
      dbacc[r] += leaf_shfl(dbacc[r], lane ^ off);
    }
    if (lr == 0) {
      L.dgc[tq + r] = rowacc[r];
      L.db[tq + r] = dbacc[r];
    }
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) tot += leaf_shfl(tot, lane ^ off);
  if (lane == 0) L.red[wave] = tot;
  leaf_barrier();
  if (wave == 0) {
    const int t = lane;
    float dgc = L.dgc[t] - (L.colsum[0][t] + L.colsum[1][t] +
                            L.colsum[2][t] + L.colsum[3][t]);
    if (t == kGdnC - 1) dgc += L.red[0] + L.red[1] + L.red[2] + L.red[3];
    // gc = cumsum(g): dg_t = sum of dgc over the rows t .. 63 of the chunk
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float dn = leaf_shfl(dgc, lane + off);
      if (lane + off < 64) dgc += dn;
    }
    dg[row0 + t] = dgc;
    dbeta[row0 + t] = L.db[t] + L.dbv[t];
  }
}

// ---------------------------------------------------------------------------
// chunked gated delta rule at Dk = Dv = 128: forward (+ aux) and reverse scan
// ---------------------------------------------------------------------------
//
// The same per-chunk algebra and the same rounding points as the D = 64
// kernels above (state before K@S and Q@S, e^{gc} K, e^{gc} Q, N, R before
// N@R, K e^{gc_last - gc}, the output), laid out for twice the head width:
//
//   * Dv split: gridDim.y = 128 / DVT column slices of the state per head,
//     DVT = 64 (two slices) or 32 (four). The K-side work (KK^T, QK^T, the
//     decay scan, M, N) is repeated per slice, so four slices are only taken
//     while all of them still sit on the chip at once (launcher below).
//   * 8 waves per workgroup. Wave w = (rs = w & 3, nh = w >> 2) owns rows
//     16 rs .. 16 rs + 15 of every chunk product and half nh of its columns:
//     2 of the 4 column tiles of M and N, DVT / 32 of the v tiles, each with
//     4 contraction steps over Dk = 128. The VALU phases (staging, scaling,
//     the fp32 state update, the 128 x DVT fp32 stores) run 512 wide.
//   * The fp32 state (dL/dState in the reverse scan) lives in REGISTERS, not
//     LDS: thread (dkg, dvq) keeps the DVT/16 x 4 block at rows
//     dkg * DVT/16, columns 4 dvq, for the whole chunk loop. The rank-64
//     update reads one 16 B row piece of R and one 4-8 B piece of the scaled
//     K per chunk row for 8-16 FMAs; the bf16 transposed image for the next
//     chunk's MFMAs, s0 / ds0 and the final state are written from the
//     registers. This frees 32 KB of LDS, which pays for
//   * padded rows (+16 B) on every bf16 tile, so the 16 B fragment reads of
//     16 consecutive rows spread over the banks (a 256 B row pitch would put
//     them all on one), and two scaled-K scratch tiles instead of one, so a
//     chunk takes 6 barriers instead of 9;
//   * the triangular solves run in place (rhs -> R, dR -> drhs) with the
//     D = 64 scheme: wave owns DVT / 8 columns, lanes split j in 64 / (DVT/8)
//     groups, xor-shuffle combine.
//   * the decay scan is a 64-lane shuffle scan by one wave.
// LDS: forward 145 KB (DVT 64) / 120 KB (DVT 32), reverse scan the same;
// one workgroup per CU either way.
constexpr int kGdnW = 128;            // Dk = Dv
constexpr int kGdnWP = kGdnW + 8;     // row pitch of a Dk-wide bf16 tile
constexpr int kGdnCP = kGdnC + 8;     // row pitch of a chunk-wide bf16 tile
constexpr int kGdnWT = 512;           // threads per workgroup
constexpr int kGdnLdsMax = 160 * 1024;
typedef bf16_t WideTile[kGdnC][kGdnWP];

template <int DVT>
struct GdnWideLds {
  float M[kGdnC][kGdnC + 1];      // solve matrix (+1 pad)
  float R[kGdnC][DVT + 4];        // rhs, solved in place to R
  WideTile kc;                    // K chunk
  WideTile qc;                    // Q chunk
  WideTile ek;                    // e^{gc} K, then e^{gc} Q
  WideTile wk;                    // K e^{gc_last - gc}
  bf16_t vc[kGdnC][DVT];          // V chunk slice
  bf16_t sbT[DVT][kGdnWP];        // state^T cast to bf16: sbT[v][k]
  bf16_t nb[kGdnC][kGdnCP];       // N cast to bf16
  bf16_t rbT[DVT][kGdnCP];        // R^T cast to bf16: rbT[v][t]
  float gc[kGdnC];
  float beta[kGdnC];
};

template <int DVT>
struct GdnWideBwdLds {
  float M[kGdnC][kGdnC + 1];      // solve matrix (+1 pad)
  float dx[kGdnC][DVT + 4];       // dR, solved in place to drhs
  WideTile kc;                    // K chunk
  WideTile qc;                    // Q chunk
  WideTile wq;                    // K e^{gc_last - gc}, then e^{gc} Q
  WideTile ek;                    // e^{gc} K
  bf16_t doc[kGdnC][DVT];         // dO chunk slice
  bf16_t doT[DVT][kGdnCP];        // dO^T (B fragments of N^T @ dO)
  bf16_t dsT[DVT][kGdnWP];        // dS^T cast to bf16 (B fragments)
  bf16_t nbT[kGdnC][kGdnCP];      // N^T cast to bf16 (A fragments)
  float gc[kGdnC];
  float beta[kGdnC];
};

static_assert(sizeof(GdnWideLds<64>) <= kGdnLdsMax &&
                  sizeof(GdnWideLds<32>) <= kGdnLdsMax &&
                  sizeof(GdnWideBwdLds<64>) <= kGdnLdsMax &&
                  sizeof(GdnWideBwdLds<32>) <= kGdnLdsMax,
              "a workgroup has 160 KB of LDS");

// Rows [0, c_rows) of a (rows, 128) bf16 matrix into a padded tile, zeros in
// the rows past the end.
D9D_DEVICE void wide_stage(WideTile& dst, const bf16_t* __restrict__ src,
                           int c_rows) {
  for (int i = threadIdx.x; i < kGdnC * kGdnW / 8; i += kGdnWT) {
    const int row = i / (kGdnW / 8);
    const int col = (i % (kGdnW / 8)) * 8;
    bf16x8 x = {};
    if (row < c_rows) {
      x = *reinterpret_cast<const bf16x8*>(src + (int64_t)row * kGdnW + col);
    }
    *reinterpret_cast<bf16x8*>(&dst[row][col]) = x;
  }
}

// dst[row][:] = bf16(src[row][:] * sc(row)), sc = e^{gc_row}, or with TAIL
// e^{g_tot - gc_row} inside the chunk and 0 past its end
template <bool TAIL>
D9D_DEVICE void wide_scale(WideTile& dst, const WideTile& src, const float* gc,
                           float g_tot, int c_rows) {
  for (int i = threadIdx.x; i < kGdnC * kGdnW / 8; i += kGdnWT) {
    const int row = i / (kGdnW / 8);
    const int col = (i % (kGdnW / 8)) * 8;
    float sc = __builtin_amdgcn_exp2f((TAIL ? g_tot - gc[row] : gc[row]) *
                                      1.44269504f);
    if (TAIL && row >= c_rows) sc = 0.f;
    const bf16x8 x = *reinterpret_cast<const bf16x8*>(&src[row][col]);
    bf16x8 y;
#pragma unroll
    for (int j = 0; j < 8; ++j) y[j] = (bf16_t)((float)x[j] * sc);
    *reinterpret_cast<bf16x8*>(&dst[row][col]) = y;
  }
}

// gc = cumsum(g) (constant past the end) and beta (zero past the end) of
// one chunk, by ONE whole wave: lane t owns row t.
D9D_DEVICE void wide_gates(const float* __restrict__ gp,
                           const float* __restrict__ bp, int c_rows,
                           float* gc, float* beta) {
  const int t = threadIdx.x & 63;
  float run = (t < c_rows) ? gp[t] : 0.f;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const float up = leaf_shfl(run, t - off);
    if (t >= off) run += up;
  }
  gc[t] = run;
  beta[t] = (t < c_rows) ? bp[t] : 0.f;
}

// acc[nt] += A[arow][0 : 32 KS] . B[brow0 + 16 nt + (lane & 15)][0 : 32 KS]
template <int NT, int KS, int PA, int PB>
D9D_DEVICE void wide_mma(f32x4 (&acc)[NT], bf16_t (*a)[PA], int arow,
                         bf16_t (*b)[PB], int brow0, int lane) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int d0 = ks * 32 + (lane >> 4) * 8;
    const bf16x8 af = *reinterpret_cast<const bf16x8*>(&a[arow][d0]);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int brow = brow0 + nt * 16 + (lane & 15);
      const bf16x8 bf = *reinterpret_cast<const bf16x8*>(&b[brow][d0]);
      acc[nt] = mfma16(af, bf, acc[nt]);
    }
  }
}

// bf16 transposed image of this thread's TK x 4 block of the fp32 state:
// img[dv0 + b][dk0 + a] = bf16(st[a][b])
template <int TK>
D9D_DEVICE void wide_state_image(bf16_t (*img)[kGdnWP], const float (&st)[TK][4],
                                 int dk0, int dv0) {
#pragma unroll
  for (int b = 0; b < 4; ++b) {
#pragma unroll
    for (int a = 0; a < TK; ++a) img[dv0 + b][dk0 + a] = (bf16_t)st[a][b];
  }
}

// rows dk0 .. dk0 + TK of a (128, 128) fp32 matrix, columns col .. col + 3
template <int TK>
D9D_DEVICE void wide_state_store(float* __restrict__ dst, const float (&st)[TK][4],
                                 int dk0, int col) {
#pragma unroll
  for (int a = 0; a < TK; ++a) {
    *reinterpret_cast<float4*>(dst + (int64_t)(dk0 + a) * kGdnW + col) =
        make_float4(st[a][0], st[a][1], st[a][2], st[a][3]);
  }
}

// (built without packed fp32 VALU ops, like the leaf kernel)
template <int DVT, bool VARLEN>
__global__ __launch_bounds__(kGdnWT, 1)
__attribute__((target("no-packed-fp32-ops"))) void gdn_chunk_fwd_wide_kernel(
    const bf16_t* __restrict__ q,   // (B, H, S, 128)
    const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v,
    const float* __restrict__ beta,      // (B, H, S)
    const float* __restrict__ decay_log, // (B, H, S)
    bf16_t* __restrict__ out,            // (B, H, S, 128) or nullptr
    float* __restrict__ final_state,     // (n_wg, 128, 128) or nullptr
    float* __restrict__ r_out,           // (B, H, S, 128) fp32 or nullptr
    float* __restrict__ s0_out,          // (B, H, nc, 128, 128) fp32 or nullptr
    int64_t n_wg, int64_t S,
    const int* __restrict__ cu,          // varlen only (see GdnSpan)
    const int* __restrict__ chunk_off,   // varlen only
    int H, int64_t nc_total) {           // varlen only
  constexpr int NTV = DVT / 32;        // v tiles per wave
  constexpr int TK = DVT / 16;         // state rows per thread
  constexpr int NV4 = DVT / 4;         // 4-column groups of the slice
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  GdnWideLds<DVT>& L = *reinterpret_cast<GdnWideLds<DVT>*>(smem_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int rs = wave & 3;             // row strip
  const int nh = wave >> 2;            // column half
  const int arow = rs * 16 + (lane & 15);        // A fragment row
  const int crow = rs * 16 + (lane >> 4) * 4;    // first C layout row
  const int ccol = lane & 15;                    // C layout column in a tile
  const int dk0 = (tid / NV4) * TK;    // this thread's state block
  const int dv0 = (tid % NV4) * 4;
  const int64_t bh = blockIdx.x;
  const int v0 = blockIdx.y * DVT;     // this block's Dv slice
  if (bh >= n_wg) return;

  const GdnSpan span = gdn_span<VARLEN>(bh, S, cu, chunk_off, H, nc_total);
  const int64_t len = span.len;
  const bf16_t* qp = q + span.row0 * kGdnW;
  const bf16_t* kp = k + span.row0 * kGdnW;
  const bf16_t* vp = v + span.row0 * kGdnW + v0;
  const float* bp = beta + span.row0;
  const float* gp = decay_log + span.row0;

  float st[TK][4];
#pragma unroll
  for (int a = 0; a < TK; ++a) {
#pragma unroll
    for (int b = 0; b < 4; ++b) st[a][b] = 0.f;
  }

  const float kLog2eG = 1.44269504f;
  const int n_chunks = (int)((len + kGdnC - 1) / kGdnC);
  for (int ch = 0; ch < n_chunks; ++ch) {
    const int s0 = ch * kGdnC;
    const int c_rows = min((int)(len - (int64_t)s0), kGdnC);

    // ---- stage chunk tiles (zero-pad past c_rows), state^T bf16, gates ---
    wide_stage(L.kc, kp + (int64_t)s0 * kGdnW, c_rows);
    wide_stage(L.qc, qp + (int64_t)s0 * kGdnW, c_rows);
    for (int i = tid; i < kGdnC * DVT / 8; i += kGdnWT) {
      const int row = i / (DVT / 8);
      const int col = (i % (DVT / 8)) * 8;
      bf16x8 x = {};
      if (row < c_rows) {
        x = *reinterpret_cast<const bf16x8*>(
            vp + (int64_t)(s0 + row) * kGdnW + col);
      }
      *reinterpret_cast<bf16x8*>(&L.vc[row][col]) = x;
    }
    wide_state_image<TK>(L.sbT, st, dk0, dv0);
    if (wave == 0) wide_gates(gp + s0, bp + s0, c_rows, L.gc, L.beta);
    if (s0_out != nullptr) {
      wide_state_store<TK>(
          s0_out + (span.chunk0 + ch) * (int64_t)kGdnW * kGdnW, st, dk0,
          v0 + dv0);
    }
    leaf_barrier();

    // ---- M = tril(beta * KK^T * ratio, -1); e^{gc} K and w K scratch -----
    const float g_tot = L.gc[c_rows - 1];
    {
      f32x4 acc[2];
      acc[0] = acc[1] = {0.f, 0.f, 0.f, 0.f};
      wide_mma<2, 4>(acc, L.kc, arow, L.kc, nh * 32, lane);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = crow + r;
          const int j = nh * 32 + nt * 16 + ccol;
          float m = 0.f;
          if (j < t) {
            m = L.beta[t] * acc[nt][r] *
                __builtin_amdgcn_exp2f((L.gc[t] - L.gc[j]) * kLog2eG);
          }
          L.M[t][j] = m;
        }
      }
    }
    wide_scale<false>(L.ek, L.kc, L.gc, g_tot, c_rows);
    wide_scale<true>(L.wk, L.kc, L.gc, g_tot, c_rows);
    leaf_barrier();

    // ---- rhs = diag(beta) (V - (e^{gc} K) @ S) ---------------------------
    {
      f32x4 acc[NTV];
#pragma unroll
      for (int nt = 0; nt < NTV; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
      wide_mma<NTV, 4>(acc, L.ek, arow, L.sbT, nh * (DVT / 2), lane);
#pragma unroll
      for (int nt = 0; nt < NTV; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = crow + r;
          const int vcol = nh * (DVT / 2) + nt * 16 + ccol;
          L.R[t][vcol] = L.beta[t] * ((float)L.vc[t][vcol] - acc[nt][r]);
        }
      }
    }
    leaf_barrier();

    // ---- forward substitution: (I + M) R = rhs, in place -----------------
    // wave w owns Dv columns [w CPW, (w+1) CPW); lane = qj * CPW + c: each
    // lane partial-sums its j-group of M[t,:] * R[:,col], xor-shuffles
    // combine the JG partials and the qj == 0 lane writes R[t][col] (+ the
    // bf16 R^T copy). DVT 64: 8 cols x 8 groups; DVT 32: 4 cols x 16.
    {
      constexpr int CPW = DVT / 8;
      constexpr int JG = 64 / CPW;
      constexpr int jspan = kGdnC / JG;
      const int qj = lane / CPW;
      const int col = wave * CPW + lane % CPW;
      for (int t = 0; t < kGdnC; ++t) {
        float part = 0.f;
        const int jend = min(t, (qj + 1) * jspan);
        for (int j = qj * jspan; j < jend; ++j) {
          part += L.M[t][j] * L.R[j][col];
        }
        // all 64 lanes active and convergent
#pragma unroll
        for (int off = CPW; off < 64; off <<= 1) {
          part += leaf_shfl(part, lane ^ off);
        }
        const float r_t = L.R[t][col] - part;
        if (qj == 0) {
          L.R[t][col] = r_t;
          L.rbT[col][t] = (bf16_t)r_t;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    leaf_barrier();

    if (r_out != nullptr) {
      for (int i = tid; i < kGdnC * NV4; i += kGdnWT) {
        const int t = i / NV4;
        const int c4 = (i % NV4) * 4;
        if (t < c_rows) {
          *reinterpret_cast<float4*>(
              r_out + (span.row0 + s0 + t) * kGdnW + v0 + c4) =
              *reinterpret_cast<const float4*>(&L.R[t][c4]);
        }
      }
    }

    // ---- N (bf16) and O = (e^{gc} Q) @ S + N @ R -------------------------
    // (skipped when out == nullptr: the backward recompute only needs the
    // solve results and chunk states)
    if (out != nullptr) {
      wide_scale<false>(L.ek, L.qc, L.gc, g_tot, c_rows);
      {
        f32x4 acc[2];
        acc[0] = acc[1] = {0.f, 0.f, 0.f, 0.f};
        wide_mma<2, 4>(acc, L.qc, arow, L.kc, nh * 32, lane);
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int t = crow + r;
            const int j = nh * 32 + nt * 16 + ccol;
            float n = 0.f;
            if (j <= t) {
              n = acc[nt][r] *
                  __builtin_amdgcn_exp2f((L.gc[t] - L.gc[j]) * kLog2eG);
            }
            L.nb[t][j] = (bf16_t)n;
          }
        }
      }
      leaf_barrier();
      f32x4 acc[NTV];
#pragma unroll
      for (int nt = 0; nt < NTV; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
      wide_mma<NTV, 4>(acc, L.ek, arow, L.sbT, nh * (DVT / 2), lane);
      wide_mma<NTV, 2>(acc, L.nb, arow, L.rbT, nh * (DVT / 2), lane);
      bf16_t* op = out + (span.row0 + s0) * kGdnW + v0;
#pragma unroll
      for (int nt = 0; nt < NTV; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = crow + r;
          const int vcol = nh * (DVT / 2) + nt * 16 + ccol;
          if (t < c_rows) op[(int64_t)t * kGdnW + vcol] = (bf16_t)acc[nt][r];
        }
      }
    }

    // ---- state = e^{gc_last} S + (K e^{gc_last - gc})^T @ R, in registers
    {
      const float e_tot = __builtin_amdgcn_exp2f(g_tot * kLog2eG);
#pragma unroll
      for (int a = 0; a < TK; ++a) {
#pragma unroll
        for (int b = 0; b < 4; ++b) st[a][b] *= e_tot;
      }
      for (int t = 0; t < c_rows; ++t) {
        const float4 rv = *reinterpret_cast<const float4*>(&L.R[t][dv0]);
        const float r4[4] = {rv.x, rv.y, rv.z, rv.w};
#pragma unroll
        for (int a = 0; a < TK; ++a) {
          const float kv = (float)L.wk[t][dk0 + a];
#pragma unroll
          for (int b = 0; b < 4; ++b) st[a][b] += kv * r4[b];
        }
      }
    }
    leaf_barrier();
  }

  if (final_state != nullptr) {
    wide_state_store<TK>(final_state + bh * kGdnW * kGdnW, st, dk0, v0 + dv0);
  }
}

// Reverse scan at D = 128: the algebra of gdn_chunk_bwd_scan_kernel in the
// layout of the forward kernel above, dL/dState in registers.
template <int DVT, bool VARLEN>
__global__ __launch_bounds__(kGdnWT, 1)
__attribute__((target("no-packed-fp32-ops"))) void gdn_chunk_bwd_scan_wide_kernel(
    const bf16_t* __restrict__ q,    // (B, H, S, 128)
    const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ dout, // (B, H, S, 128)
    const float* __restrict__ beta,
    const float* __restrict__ decay_log,
    float* __restrict__ drhs_out,    // (B, H, S, 128)
    float* __restrict__ ds0_out,     // (B, H, nc, 128, 128)
    int64_t n_wg, int64_t S,
    const int* __restrict__ cu,          // varlen only (see GdnSpan)
    const int* __restrict__ chunk_off,   // varlen only
    int H, int64_t nc_total) {           // varlen only
  constexpr int NTV = DVT / 32;
  constexpr int TK = DVT / 16;
  constexpr int NV4 = DVT / 4;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  GdnWideBwdLds<DVT>& L = *reinterpret_cast<GdnWideBwdLds<DVT>*>(smem_raw);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int rs = wave & 3;
  const int nh = wave >> 2;
  const int arow = rs * 16 + (lane & 15);
  const int crow = rs * 16 + (lane >> 4) * 4;
  const int ccol = lane & 15;
  const int dk0 = (tid / NV4) * TK;
  const int dv0 = (tid % NV4) * 4;
  const int64_t bh = blockIdx.x;
  const int v0 = blockIdx.y * DVT;
  if (bh >= n_wg) return;

  const GdnSpan span = gdn_span<VARLEN>(bh, S, cu, chunk_off, H, nc_total);
  const int64_t len = span.len;
  const bf16_t* qp = q + span.row0 * kGdnW;
  const bf16_t* kp = k + span.row0 * kGdnW;
  const bf16_t* dop = dout + span.row0 * kGdnW + v0;
  const float* bp = beta + span.row0;
  const float* gp = decay_log + span.row0;

  float dS[TK][4];
#pragma unroll
  for (int a = 0; a < TK; ++a) {
#pragma unroll
    for (int b = 0; b < 4; ++b) dS[a][b] = 0.f;
  }

  const float kLog2eG = 1.44269504f;
  const int n_chunks = (int)((len + kGdnC - 1) / kGdnC);
  for (int ch = n_chunks - 1; ch >= 0; --ch) {
    const int s0 = ch * kGdnC;
    const int c_rows = min((int)(len - (int64_t)s0), kGdnC);

    // ---- stage chunk tiles (zero-pad), dO and dO^T, dS^T, gates ----------
    wide_stage(L.kc, kp + (int64_t)s0 * kGdnW, c_rows);
    wide_stage(L.qc, qp + (int64_t)s0 * kGdnW, c_rows);
    for (int i = tid; i < kGdnC * DVT / 8; i += kGdnWT) {
      const int row = i / (DVT / 8);
      const int col = (i % (DVT / 8)) * 8;
      bf16x8 x = {};
      if (row < c_rows) {
        x = *reinterpret_cast<const bf16x8*>(
            dop + (int64_t)(s0 + row) * kGdnW + col);
      }
      *reinterpret_cast<bf16x8*>(&L.doc[row][col]) = x;
#pragma unroll
      for (int j = 0; j < 8; ++j) L.doT[col + j][row] = x[j];
    }
    wide_state_image<TK>(L.dsT, dS, dk0, dv0);
    if (wave == 0) wide_gates(gp + s0, bp + s0, c_rows, L.gc, L.beta);
    leaf_barrier();

    // ---- M (fp32, solve matrix), N^T (bf16), w K and e^{gc} K ------------
    const float g_tot = L.gc[c_rows - 1];
    {
      f32x4 accm[2], accn[2];
      accm[0] = accm[1] = accn[0] = accn[1] = {0.f, 0.f, 0.f, 0.f};
      wide_mma<2, 4>(accm, L.kc, arow, L.kc, nh * 32, lane);
      wide_mma<2, 4>(accn, L.qc, arow, L.kc, nh * 32, lane);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = crow + r;
          const int j = nh * 32 + nt * 16 + ccol;
          const float ratio =
              __builtin_amdgcn_exp2f((L.gc[t] - L.gc[j]) * kLog2eG);
          L.M[t][j] = (j < t) ? L.beta[t] * accm[nt][r] * ratio : 0.f;
          L.nbT[j][t] = (bf16_t)((j <= t) ? accn[nt][r] * ratio : 0.f);
        }
      }
    }
    wide_scale<true>(L.wq, L.kc, L.gc, g_tot, c_rows);
    wide_scale<false>(L.ek, L.kc, L.gc, g_tot, c_rows);
    leaf_barrier();

    // ---- dR = wK @ dS + N^T @ dO  (fp32 into L.dx) -----------------------
    {
      f32x4 acc[NTV];
#pragma unroll
      for (int nt = 0; nt < NTV; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
      wide_mma<NTV, 4>(acc, L.wq, arow, L.dsT, nh * (DVT / 2), lane);
      wide_mma<NTV, 2>(acc, L.nbT, arow, L.doT, nh * (DVT / 2), lane);
#pragma unroll
      for (int nt = 0; nt < NTV; ++nt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          L.dx[crow + r][nh * (DVT / 2) + nt * 16 + ccol] = acc[nt][r];
        }
      }
    }
    leaf_barrier();

    // ---- backward substitution: (I + M)^T drhs = dR, in place ------------
    // drhs[t] = dR[t] - sum_{j > t} M[j][t] * drhs[j]; the forward solve's
    // column / j-group split, t walked downward.
    {
      constexpr int CPW = DVT / 8;
      constexpr int JG = 64 / CPW;
      constexpr int jspan = kGdnC / JG;
      const int qj = lane / CPW;
      const int col = wave * CPW + lane % CPW;
      for (int t = kGdnC - 2; t >= 0; --t) {
        float part = 0.f;
        const int jlo = max(t + 1, qj * jspan);
        const int jhi = (qj + 1) * jspan;
        for (int j = jlo; j < jhi; ++j) {
          part += L.M[j][t] * L.dx[j][col];
        }
#pragma unroll
        for (int off = CPW; off < 64; off <<= 1) {
          part += leaf_shfl(part, lane ^ off);
        }
        if (qj == 0) {
          L.dx[t][col] -= part;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    leaf_barrier();

    // drhs out (fp32)
    for (int i = tid; i < kGdnC * NV4; i += kGdnWT) {
      const int t = i / NV4;
      const int c4 = (i % NV4) * 4;
      if (t < c_rows) {
        *reinterpret_cast<float4*>(
            drhs_out + (span.row0 + s0 + t) * kGdnW + v0 + c4) =
            *reinterpret_cast<const float4*>(&L.dx[t][c4]);
      }
    }

    // ---- dS = e^{g_tot} dS + EK^T @ (-beta drhs) + EQ^T @ dO, in registers
    wide_scale<false>(L.wq, L.qc, L.gc, g_tot, c_rows);
    {
      const float e_tot = __builtin_amdgcn_exp2f(g_tot * kLog2eG);
#pragma unroll
      for (int a = 0; a < TK; ++a) {
#pragma unroll
        for (int b = 0; b < 4; ++b) dS[a][b] *= e_tot;
      }
      for (int t = 0; t < c_rows; ++t) {
        const float bt = L.beta[t];
        const float4 xv = *reinterpret_cast<const float4*>(&L.dx[t][dv0]);
        const float x4[4] = {bt * xv.x, bt * xv.y, bt * xv.z, bt * xv.w};
#pragma unroll
        for (int a = 0; a < TK; ++a) {
          const float kv = (float)L.ek[t][dk0 + a];
#pragma unroll
          for (int b = 0; b < 4; ++b) dS[a][b] -= kv * x4[b];
        }
      }
    }
    leaf_barrier();
    for (int t = 0; t < c_rows; ++t) {
      const bf16x4 dv4 = *reinterpret_cast<const bf16x4*>(&L.doc[t][dv0]);
#pragma unroll
      for (int a = 0; a < TK; ++a) {
        const float qv = (float)L.wq[t][dk0 + a];
#pragma unroll
        for (int b = 0; b < 4; ++b) dS[a][b] += qv * (float)dv4[b];
      }
    }
    wide_state_store<TK>(ds0_out + (span.chunk0 + ch) * (int64_t)kGdnW * kGdnW,
                         dS, dk0, v0 + dv0);
    leaf_barrier();
  }
}

// ---------------------------------------------------------------------------
// chunked gated delta rule backward LEAF GRADIENTS at Dk = Dv = 128
// ---------------------------------------------------------------------------
//
// The algebra, the rowsum(drhs * P) reassociation through G and every
// rounding point of gdn_chunk_bwd_leaf_kernel (comment above GdnLeafLds), one
// workgroup per (b, h, chunk) of 64 rows; only the feature dims double: the
// D-wide products (dwK, dEQ, G, dqk K, dqk^T Q, dkk K, dkk^T K) are 64 x 128,
// the contractions over D (dwK, dEQ, G, dN, dM, kk, qk) 128 long, and the
// 64 x 64 matrices keep their size. Laid out for that:
//
//   * 8 waves, wave w = (rs = w & 3, nh = w >> 2) as in the kernels above:
//     rows 16 rs .. 16 rs + 15 of every product, column half nh. A wave keeps
//     16 x 64 of dq and dk (32 accumulator registers) and a 16 x 32 half of
//     dN, dM, kk, qk (2 column tiles each), which never leave registers.
//   * B operands are full-size images at the padded pitches, 158 KB with the
//     small vectors, one workgroup per CU: K rows, K^T and Q^T, and two hi/lo
//     pairs reused in phases. `a`: R (64 x 128) -> dqk -> dkk (64 x 64);
//     `b`: dS1 (128 x 128) -> S0 -> dqk^T -> dkk^T.
//   * S0 is loaded with dS1 (the <dS1, S0> term wants both) and waits in
//     32 registers per thread until the dwK product has consumed the dS1
//     image, then takes its place.
//   * A fragments: R rows come from the `a` image and K rows from the K tile
//     (both are staged anyway). dO, drhs and Q rows are read from global
//     memory by the two waves of a row band: the LDS has no room for a third
//     image pair, and the second read hits the cache. dV and rowsum(drhs * V)
//     are split between the two by contraction step, so each dv element is
//     written once.
//   * rowsums end in two per-column-half slots, colsum(rr) in one slot per
//     row band (a (band, column) pair belongs to one wave), the dgc_63 scalar
//     in eight; wave 0 adds them up and runs the in-chunk reverse cumsum.
struct GdnWideLeafLds {
  WideTile kc;                    // K rows        (B of kk, qk; A of kk)
  bf16_t kT[kGdnW][kGdnCP];       // K^T: kT[d][t] (B of . K; K in C layout)
  bf16_t qT[kGdnW][kGdnCP];       // Q^T: qT[d][t] (B of . Q; Q in C layout)
  WideTile a[2];                  // hi/lo: R, then dqk, then dkk
  bf16_t b[2][kGdnW][kGdnWP];     // hi/lo: dS1, then S0, then dqk^T, dkk^T
  float gc[kGdnC];
  float beta[kGdnC];
  float dgc[2][kGdnC];            // row-owned part of dgc, per column half
  float db[2][kGdnC];             // C-layout part of dbeta, per column half
  float dbv[2][kGdnC];            // rowsum(drhs * V), per contraction half
  float colsum[4][kGdnC];         // colsum(rr), per row band
  float red[8];                   // per-wave part of the dgc_63 scalar
};
static_assert(sizeof(GdnWideLeafLds) <= kGdnLdsMax,
              "a workgroup has 160 KB of LDS");
constexpr int kWleafA = kGdnC * kGdnWP;   // elements between the `a` images
constexpr int kWleafB = kGdnW * kGdnWP;   // elements between the `b` images

// acc[nt] += A . B^T-image over KS contraction steps of 32: A fragments
// a[ks][image] (NA = 2: hi/lo), B rows brow0 + 16 nt + (lane & 15) of NB
// images `bimg` elements apart at row pitch PB. Cross terms run smallest
// first.
template <int NT, int KS, int NA, int NB, int PB>
D9D_DEVICE void wleaf_mma(f32x4 (&acc)[NT], const bf16x8 (&a)[KS][NA],
                          const bf16_t* b, int bimg, int brow0, int lane) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int d0 = ks * 32 + (lane >> 4) * 8;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int brow = brow0 + nt * 16 + (lane & 15);
#pragma unroll
      for (int ib = NB - 1; ib >= 0; --ib) {
        const bf16x8 bf =
            *reinterpret_cast<const bf16x8*>(b + ib * bimg + brow * PB + d0);
#pragma unroll
        for (int ia = NA - 1; ia >= 0; --ia) {
          acc[nt] = mfma16(a[ks][ia], bf, acc[nt]);
        }
      }
    }
  }
}

// hi/lo A fragments of row `arow` of an image pair at pitch kGdnWP
template <int KS>
D9D_DEVICE void wleaf_afrag(bf16x8 (&a)[KS][2], const bf16_t* img, int aimg,
                            int arow, int lane) {
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const bf16_t* p = img + arow * kGdnWP + ks * 32 + (lane >> 4) * 8;
    a[ks][0] = *reinterpret_cast<const bf16x8*>(p);
    a[ks][1] = *reinterpret_cast<const bf16x8*>(p + aimg);
  }
}

// four fp32 values -> hi/lo bf16x4 at p and p + img
D9D_DEVICE void wleaf_put4(bf16_t* p, int img, const float4& x) {
  const float xs[4] = {x.x, x.y, x.z, x.w};
  bf16x4 h4, l4;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    bf16_t h, l;
    leaf_split(xs[j], h, l);
    h4[j] = h;
    l4[j] = l;
  }
  *reinterpret_cast<bf16x4*>(p) = h4;
  *reinterpret_cast<bf16x4*>(p + img) = l4;
}

// This wave's 16 x 32 block (rows tq .., columns j0 ..) of a C-layout fp32
// tile -> hi/lo images a[t][j] and b[j][t] (a lane's four rows are one
// 8-byte store of the transpose).
D9D_DEVICE void wleaf_put(const f32x4 (&x)[2], GdnWideLeafLds& L, int tq,
                          int j0, int lane) {
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int j = j0 + nt * 16 + (lane & 15);
    bf16x4 h4, l4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      bf16_t h, l;
      leaf_split(x[nt][r], h, l);
      L.a[0][tq + r][j] = h;
      L.a[1][tq + r][j] = l;
      h4[r] = h;
      l4[r] = l;
    }
    *reinterpret_cast<bf16x4*>(&L.b[0][j][tq]) = h4;
    *reinterpret_cast<bf16x4*>(&L.b[1][j][tq]) = l4;
  }
}

// (built without packed fp32 VALU ops, like the D = 64 leaf kernel)
__global__ __launch_bounds__(kGdnWT, 1)
__attribute__((target("no-packed-fp32-ops"))) void gdn_chunk_bwd_leaf_wide_kernel(
    const bf16_t* __restrict__ q,    // (B, H, Sp, 128), Sp = 64 nc
    const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ dout,
    const float* __restrict__ beta,       // (B, H, Sp)
    const float* __restrict__ decay_log,  // (B, H, Sp)
    const float* __restrict__ r_in,       // (B, H, Sp, 128)  gdn_chunk_fwd aux
    const float* __restrict__ drhs,       // (B, H, Sp, 128)  reverse scan
    const float* __restrict__ s0,         // (B, H, nc, 128, 128)
    const float* __restrict__ ds0,        // (B, H, nc, 128, 128)
    float* __restrict__ dq,               // (B, H, Sp, 128)
    float* __restrict__ dk,
    float* __restrict__ dv,
    float* __restrict__ dbeta,            // (B, H, Sp)
    float* __restrict__ dg,
    const int* __restrict__ doc_last,     // (nc,) packed rows only, or nullptr
    int64_t n_chunks, int64_t nc) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  GdnWideLeafLds& L = *reinterpret_cast<GdnWideLeafLds*>(smem_raw);
  const bf16_t* La = &L.a[0][0][0];
  const bf16_t* Lb = &L.b[0][0][0];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int rs = wave & 3;             // row band
  const int nh = wave >> 2;            // column half
  const int lr = lane & 15;
  const int lq = lane >> 4;
  const int64_t chunk = blockIdx.x;
  if (chunk >= n_chunks) return;
  const int64_t c = chunk % nc;
  // the last chunk of a row / document hands its state to nobody: dS1 = 0
  // (and ds0[chunk + 1] is never addressed past the end of a row)
  const bool last = (c == nc - 1) || (doc_last != nullptr && doc_last[c] != 0);
  const int64_t row0 = chunk * kGdnC;
  const int64_t tile0 = row0 * kGdnW;
  const float* s0p = s0 + chunk * (int64_t)(kGdnW * kGdnW);
  const float* ds1p = ds0 + (chunk + 1) * (int64_t)(kGdnW * kGdnW);

  // ---- stage: decay scan, K / K^T / Q^T, R and dS1 images; S0 to registers
  if (wave == 0) wide_gates(decay_log + row0, beta + row0, kGdnC, L.gc, L.beta);
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int i = tid + u * kGdnWT;
    const int row = i >> 4;
    const int col = (i & 15) * 8;
    const bf16x8 kv =
        *reinterpret_cast<const bf16x8*>(k + tile0 + row * kGdnW + col);
    const bf16x8 qv =
        *reinterpret_cast<const bf16x8*>(q + tile0 + row * kGdnW + col);
    *reinterpret_cast<bf16x8*>(&L.kc[row][col]) = kv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      L.kT[col + j][row] = kv[j];
      L.qT[col + j][row] = qv[j];
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = tid + u * kGdnWT;
    const int row = i >> 5;
    const int col = (i & 31) * 4;
    wleaf_put4(&L.a[0][row][col], kWleafA,
               *reinterpret_cast<const float4*>(r_in + tile0 + row * kGdnW + col));
  }
  float4 s0r[8];
  float frob = 0.f;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int i = tid + u * kGdnWT;
    const int row = i >> 5;
    const int col = (i & 31) * 4;
    s0r[u] = *reinterpret_cast<const float4*>(s0p + row * kGdnW + col);
    if (!last) {
      const float4 d4 =
          *reinterpret_cast<const float4*>(ds1p + row * kGdnW + col);
      wleaf_put4(&L.b[0][row][col], kWleafB, d4);
      frob += d4.x * s0r[u].x + d4.y * s0r[u].y + d4.z * s0r[u].z +
              d4.w * s0r[u].w;
    }
  }
  leaf_barrier();

  // this lane's rows in the C layout: tq .. tq+3; A fragments: row arow;
  // D-wide products: columns cb + 16 nt + lr; 64 x 64 ones: jb + 16 nt + lr
  const int tq = rs * 16 + lq * 4;
  const int arow = rs * 16 + lr;
  const int cb = nh * 64;
  const int jb = nh * 32;
  const int64_t aoff = tile0 + arow * kGdnW + lq * 8;   // + ks * 32
  const float g_end = L.gc[kGdnC - 1];
  const float e_end = expf(g_end);
  float gct[4], et[4], wt[4], bt[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    gct[r] = L.gc[tq + r];
    et[r] = expf(gct[r]);
    wt[r] = expf(g_end - gct[r]);
    bt[r] = L.beta[tq + r];
  }

  f32x4 dqa[4], dka[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    dqa[nt] = {0.f, 0.f, 0.f, 0.f};
    dka[nt] = {0.f, 0.f, 0.f, 0.f};
  }
  float rowacc[4] = {0.f, 0.f, 0.f, 0.f};   // dgc partial of rows tq..tq+3
  float dbacc[4] = {0.f, 0.f, 0.f, 0.f};    // dbeta partial of the same rows
  float tot = frob * e_end;                 // dgc_63 scalar partial

  // ---- dwK = R dS1^T: dK = w dwK, dw = rowsum(dwK * K) -------------------
  if (!last) {
    bf16x8 ar[4][2];
    wleaf_afrag<4>(ar, La, kWleafA, arow, lane);
    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
    wleaf_mma<4, 4, 2, 2, kGdnWP>(acc, ar, Lb, kWleafB, cb, lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const bf16x4 kf =
          *reinterpret_cast<const bf16x4*>(&L.kT[cb + nt * 16 + lr][tq]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float dkw = acc[nt][r] * wt[r];
        dka[nt][r] = dkw;
        const float p = dkw * (float)kf[r];
        rowacc[r] -= p;
        tot += p;
      }
    }
  }
  leaf_barrier();   // dS1 image consumed: S0 takes its place
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int i = tid + u * kGdnWT;
    wleaf_put4(&L.b[0][i >> 5][(i & 31) * 4], kWleafB, s0r[u]);
  }

  // A fragments of dO and drhs (kept for the R^T products); on the way
  // dV = beta drhs and rowsum(drhs * V) for dbeta, steps 2 nh and 2 nh + 1
  bf16x8 ado[4][1], adr[4][2];
  {
    const float ba = L.beta[arow];
    float dot = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int64_t off = aoff + ks * 32;
      ado[ks][0] = *reinterpret_cast<const bf16x8*>(dout + off);
      float x[8];
      leaf_load8(drhs + off, x);
      leaf_split8(x, adr[ks][0], adr[ks][1]);
      if ((ks >> 1) == nh) {
        const bf16x8 vv = *reinterpret_cast<const bf16x8*>(v + off);
#pragma unroll
        for (int j = 0; j < 8; ++j) dot += x[j] * (float)vv[j];
        *reinterpret_cast<f32x4*>(dv + off) =
            f32x4{ba * x[0], ba * x[1], ba * x[2], ba * x[3]};
        *reinterpret_cast<f32x4*>(dv + off + 4) =
            f32x4{ba * x[4], ba * x[5], ba * x[6], ba * x[7]};
      }
    }
    dot += leaf_shfl(dot, lane ^ 16);
    dot += leaf_shfl(dot, lane ^ 32);
    if (lq == 0) L.dbv[nh][arow] = dot;
  }
  leaf_barrier();

  // ---- dEQ = dO S0^T: dQ = E dEQ, dgc += E rowsum(dEQ * Q) ---------------
  {
    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
    wleaf_mma<4, 4, 1, 2, kGdnWP>(acc, ado, Lb, kWleafB, cb, lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const bf16x4 qf =
          *reinterpret_cast<const bf16x4*>(&L.qT[cb + nt * 16 + lr][tq]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = acc[nt][r] * et[r];
        dqa[nt][r] = e;
        rowacc[r] += e * (float)qf[r];
      }
    }
  }
  // ---- G = drhs S0^T: dK -= beta E G, dgc -= beta E rowsum(G * K),
  //      dbeta -= E rowsum(G * K) -----------------------------------------
  {
    f32x4 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
    wleaf_mma<4, 4, 2, 2, kGdnWP>(acc, adr, Lb, kWleafB, cb, lane);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const bf16x4 kf =
          *reinterpret_cast<const bf16x4*>(&L.kT[cb + nt * 16 + lr][tq]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float ge = acc[nt][r] * et[r];
        const float gk = ge * (float)kf[r];
        dka[nt][r] -= bt[r] * ge;
        rowacc[r] -= bt[r] * gk;
        dbacc[r] -= gk;
      }
    }
  }

  // ---- this wave's half of dN, dM, kk, qk in registers -> dqk (x), dkk (y),
  //      dbeta, rr sums ------------------------------------------------------
  f32x4 x[2], y[2];
  {
    f32x4 an[2], am[2], akk[2], aqk[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      an[nt] = {0.f, 0.f, 0.f, 0.f};
      am[nt] = {0.f, 0.f, 0.f, 0.f};
      akk[nt] = {0.f, 0.f, 0.f, 0.f};
      aqk[nt] = {0.f, 0.f, 0.f, 0.f};
    }
    bf16x8 ak[4][1], aq[4][1];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      ak[ks][0] =
          *reinterpret_cast<const bf16x8*>(&L.kc[arow][ks * 32 + lq * 8]);
      aq[ks][0] = *reinterpret_cast<const bf16x8*>(q + aoff + ks * 32);
    }
    wleaf_mma<2, 4, 1, 2, kGdnWP>(an, ado, La, kWleafA, jb, lane);
    wleaf_mma<2, 4, 2, 2, kGdnWP>(am, adr, La, kWleafA, jb, lane);
    wleaf_mma<2, 4, 1, 1, kGdnWP>(akk, ak, &L.kc[0][0], 0, jb, lane);
    wleaf_mma<2, 4, 1, 1, kGdnWP>(aqk, aq, &L.kc[0][0], 0, jb, lane);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int j = jb + nt * 16 + lr;
      const float gcj = L.gc[j];
      float colacc = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int t = tq + r;
        // decay ratio only where t >= j, so it stays <= 1
        const float ratio = (j <= t) ? expf(gct[r] - gcj) : 0.f;
        const float dn = (j <= t) ? an[nt][r] : 0.f;
        const float dm = (j < t) ? -am[nt][r] : 0.f;
        const float dkkr = dm * bt[r];
        dbacc[r] += dm * akk[nt][r] * ratio;
        const float rr = (dn * aqk[nt][r] + dkkr * akk[nt][r]) * ratio;
        rowacc[r] += rr;
        colacc += rr;
        x[nt][r] = dn * ratio;
        y[nt][r] = dkkr * ratio;
      }
      colacc += leaf_shfl(colacc, lane ^ 16);
      colacc += leaf_shfl(colacc, lane ^ 32);
      if (lq == 0) L.colsum[rs][j] = colacc;
    }
  }
  leaf_barrier();   // R and S0 images consumed

  // ---- dQ += dqk K, dK += dqk^T Q ----------------------------------------
  wleaf_put(x, L, tq, jb, lane);
  leaf_barrier();
  {
    bf16x8 af[2][2];
    wleaf_afrag<2>(af, La, kWleafA, arow, lane);
    wleaf_mma<4, 2, 2, 1, kGdnCP>(dqa, af, &L.kT[0][0], 0, cb, lane);
    wleaf_afrag<2>(af, Lb, kWleafB, arow, lane);
    wleaf_mma<4, 2, 2, 1, kGdnCP>(dka, af, &L.qT[0][0], 0, cb, lane);
  }
  leaf_barrier();

  // ---- dK += dkk K + dkk^T K ---------------------------------------------
  wleaf_put(y, L, tq, jb, lane);
  leaf_barrier();
  {
    bf16x8 af[2][2];
    wleaf_afrag<2>(af, La, kWleafA, arow, lane);
    wleaf_mma<4, 2, 2, 1, kGdnCP>(dka, af, &L.kT[0][0], 0, cb, lane);
    wleaf_afrag<2>(af, Lb, kWleafB, arow, lane);
    wleaf_mma<4, 2, 2, 1, kGdnCP>(dka, af, &L.kT[0][0], 0, cb, lane);
  }

  // ---- outputs -----------------------------------------------------------
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t off = tile0 + (tq + r) * kGdnW + cb + nt * 16 + lr;
      dq[off] = dqa[nt][r];
      dk[off] = dka[nt][r];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      rowacc[r] += leaf_shfl(rowacc[r], lane ^ off);
      dbacc[r] += leaf_shfl(dbacc[r], lane ^ off);
    }
    if (lr == 0) {
      L.dgc[nh][tq + r] = rowacc[r];
      L.db[nh][tq + r] = dbacc[r];
    }
  }
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) tot += leaf_shfl(tot, lane ^ off);
  if (lane == 0) L.red[wave] = tot;
  leaf_barrier();
  if (wave == 0) {
    const int t = lane;
    float dgc = L.dgc[0][t] + L.dgc[1][t] -
                (L.colsum[0][t] + L.colsum[1][t] + L.colsum[2][t] +
                 L.colsum[3][t]);
    if (t == kGdnC - 1) {
#pragma unroll
      for (int w = 0; w < 8; ++w) dgc += L.red[w];
    }
    // gc = cumsum(g): dg_t = sum of dgc over the rows t .. 63 of the chunk
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float dn = leaf_shfl(dgc, lane + off);
      if (lane + off < 64) dgc += dn;
    }
    dg[row0 + t] = dgc;
    dbeta[row0 + t] = L.db[0][t] + L.db[1][t] + L.dbv[0][t] + L.dbv[1][t];
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

// D = 128: a workgroup takes a whole CU (120-145 KB of LDS). Four Dv slices
// of 32 repeat the K-side work four times per head, so they are only taken
// while 4 n_wg workgroups still run in one pass over the 256 CUs; beyond
// that two slices of 64 do less work in the same number of passes.
bool gdn_wide_quarter_dv(int64_t n_wg) { return n_wg * 4 <= 256; }

template <int DVT, bool VARLEN, class... Args>
void gdn_fwd_wide_launch(int64_t n_wg, Args... args) {
  auto kern = &d9d::gdn_chunk_fwd_wide_kernel<DVT, VARLEN>;
  static bool attr_set = false;   // one per instantiation
  if (!attr_set) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                        hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)sizeof(d9d::GdnWideLds<DVT>));
    attr_set = true;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)n_wg, d9d::kGdnW / DVT),
                     dim3(d9d::kGdnWT), sizeof(d9d::GdnWideLds<DVT>),
                     at::hip::getCurrentHIPStream(), args...);
}

template <int DVT, bool VARLEN, class... Args>
void gdn_bwd_scan_wide_launch(int64_t n_wg, Args... args) {
  auto kern = &d9d::gdn_chunk_bwd_scan_wide_kernel<DVT, VARLEN>;
  static bool attr_set = false;   // one per instantiation
  if (!attr_set) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                        hipFuncAttributeMaxDynamicSharedMemorySize,
                        (int)sizeof(d9d::GdnWideBwdLds<DVT>));
    attr_set = true;
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)n_wg, d9d::kGdnW / DVT),
                     dim3(d9d::kGdnWT), sizeof(d9d::GdnWideBwdLds<DVT>),
                     at::hip::getCurrentHIPStream(), args...);
}

template <bool VARLEN>
void gdn_fwd_launch(int64_t n_wg, int64_t S, const torch::Tensor& q,
                    const torch::Tensor& k, const torch::Tensor& v,
                    const torch::Tensor& beta, const torch::Tensor& g,
                    __bf16* out, float* fs, float* r, float* s0,
                    const int* cu, const int* chunk_off, int H, int64_t nc) {
  if (q.size(-1) == d9d::kGdnW) {
    if (n_wg == 0) return;
    auto qp = reinterpret_cast<const __bf16*>(q.data_ptr());
    auto kp = reinterpret_cast<const __bf16*>(k.data_ptr());
    auto vp = reinterpret_cast<const __bf16*>(v.data_ptr());
    if (gdn_wide_quarter_dv(n_wg)) {
      gdn_fwd_wide_launch<32, VARLEN>(
          n_wg, qp, kp, vp, beta.data_ptr<float>(), g.data_ptr<float>(), out,
          fs, r, s0, n_wg, S, cu, chunk_off, H, nc);
    } else {
      gdn_fwd_wide_launch<64, VARLEN>(
          n_wg, qp, kp, vp, beta.data_ptr<float>(), g.data_ptr<float>(), out,
          fs, r, s0, n_wg, S, cu, chunk_off, H, nc);
    }
    return;
  }
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
  if (q.size(-1) == d9d::kGdnW) {
    if (n_wg == 0) return;
    auto qp = reinterpret_cast<const __bf16*>(q.data_ptr());
    auto kp = reinterpret_cast<const __bf16*>(k.data_ptr());
    auto dp = reinterpret_cast<const __bf16*>(dout.data_ptr());
    if (gdn_wide_quarter_dv(n_wg)) {
      gdn_bwd_scan_wide_launch<32, VARLEN>(
          n_wg, qp, kp, dp, beta.data_ptr<float>(), g.data_ptr<float>(), drhs,
          ds0, n_wg, S, cu, chunk_off, H, nc);
    } else {
      gdn_bwd_scan_wide_launch<64, VARLEN>(
          n_wg, qp, kp, dp, beta.data_ptr<float>(), g.data_ptr<float>(), drhs,
          ds0, n_wg, S, cu, chunk_off, H, nc);
    }
    return;
  }
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

// head dims the chunk kernels are built for: 64, and 128 where `wide` (the
// forward and the reverse scan; the leaf kernel is D = 64 only)
bool gdn_head_dim_ok(const torch::Tensor& q, bool wide) {
  return q.dim() == 4 &&
         (q.size(-1) == 64 || (wide && q.size(-1) == d9d::kGdnW));
}

// dense entry points: (B, H, S, D) bf16 rows + (B, H, S) gates
void gdn_dense_checks(const char* who, const torch::Tensor& q,
                      const torch::Tensor& k, const torch::Tensor& v,
                      const torch::Tensor& beta,
                      const torch::Tensor& decay_log, bool wide = false) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == torch::kBFloat16, who,
              ": q must be a bf16 device tensor");
  TORCH_CHECK(k.is_cuda() && k.scalar_type() == torch::kBFloat16, who,
              ": k must be a bf16 device tensor");
  TORCH_CHECK(v.is_cuda() && v.scalar_type() == torch::kBFloat16, who,
              ": v / dout must be a bf16 device tensor");
  TORCH_CHECK(gdn_head_dim_ok(q, wide), who,
              wide ? " supports (B, H, S, 64) and (B, H, S, 128)"
                   : " supports (B, H, S, 64)");
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes(), who,
              ": q, k, v / dout must share one (B, H, S, D) shape");
  TORCH_CHECK(beta.is_cuda() && decay_log.is_cuda(), who,
              ": beta and decay_log must be device tensors");
  TORCH_CHECK(beta.dim() == 3 && beta.size(0) == q.size(0) &&
                  beta.size(1) == q.size(1) && beta.size(2) == q.size(2) &&
                  decay_log.sizes() == beta.sizes(),
              who, ": beta and decay_log must be (B, H, S)");
}

// (1, H, T, D) bf16 rows + (1, H, T) gates of one packed row
void gdn_varlen_checks(const char* who, const torch::Tensor& q,
                       const torch::Tensor& k, const torch::Tensor& v,
                       const torch::Tensor& beta,
                       const torch::Tensor& decay_log, bool wide = false) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(k.is_cuda() && k.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(v.is_cuda() && v.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(gdn_head_dim_ok(q, wide), who,
              wide ? " supports (1, H, T, 64) and (1, H, T, 128)"
                   : " supports (1, H, T, 64)");
  TORCH_CHECK(k.sizes() == q.sizes() && v.sizes() == q.sizes(), who,
              ": q, k, v / dout must share one (1, H, T, D) shape");
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
  gdn_dense_checks("gdn_chunk_bwd_scan", q, k, dout, beta, decay_log,
                   /*wide=*/true);
  auto qc = q.contiguous();
  auto kc = k.contiguous();
  auto dc = dout.contiguous();
  auto bc = beta.to(torch::kFloat32).contiguous();
  auto gc = decay_log.to(torch::kFloat32).contiguous();
  const int64_t B = qc.size(0), H = qc.size(1), S = qc.size(2);
  const int64_t D = qc.size(3);
  const int64_t nc = (S + 63) / 64;
  auto f32 = torch::dtype(torch::kFloat32).device(q.device());
  auto drhs = torch::empty({B, H, S, D}, f32);
  auto ds0 = torch::empty({B, H, nc, D, D}, f32);
  gdn_bwd_scan_launch<false>(B * H, S, qc, kc, dc, bc, gc,
                             drhs.data_ptr<float>(), ds0.data_ptr<float>(),
                             nullptr, nullptr, 0, 0);
  return {drhs, ds0};
}

std::vector<torch::Tensor> gdn_chunk_bwd_scan_varlen(
    torch::Tensor q, torch::Tensor k, torch::Tensor dout,
    torch::Tensor beta, torch::Tensor decay_log, torch::Tensor cu_seqlens) {
  gdn_varlen_checks("gdn_chunk_bwd_scan_varlen", q, k, dout, beta, decay_log,
                    /*wide=*/true);
  const int64_t H = q.size(1), T = q.size(2), D = q.size(3);
  auto docs = gdn_check_docs(cu_seqlens, q.size(0), T, q.device(),
                             /*with_chunks=*/true);
  auto qc = q.contiguous();
  auto kc = k.contiguous();
  auto dc = dout.contiguous();
  auto bc = beta.to(torch::kFloat32).contiguous();
  auto gc = decay_log.to(torch::kFloat32).contiguous();
  auto f32 = torch::dtype(torch::kFloat32).device(q.device());
  auto drhs = torch::empty({1, H, T, D}, f32);
  auto ds0 = torch::empty({1, H, docs.nc, D, D}, f32);
  gdn_bwd_scan_launch<true>(docs.nseq * H, T, qc, kc, dc, bc, gc,
                            drhs.data_ptr<float>(), ds0.data_ptr<float>(),
                            docs.cu_dev.data_ptr<int>(),
                            docs.chunk_off_dev.data_ptr<int>(), (int)H,
                            docs.nc);
  return {drhs, ds0};
}

namespace {

// Leaf-gradient stage shared by the dense and packed entry points at both
// head dims: checks the four scan products against q's (B, H, Sp, D),
// allocates the five outputs and launches one workgroup per chunk, the D = 64
// kernel or the wide one. `doc_last` is the (nc,) int32
// last-chunk-of-a-document flag on the device, or undefined (dense).
std::vector<torch::Tensor> gdn_bwd_leaf_impl(
    const char* who, const torch::Tensor& q, const torch::Tensor& k,
    const torch::Tensor& v, const torch::Tensor& dout,
    const torch::Tensor& beta, const torch::Tensor& decay_log,
    const torch::Tensor& r, const torch::Tensor& drhs,
    const torch::Tensor& s0, const torch::Tensor& ds0,
    const torch::Tensor& doc_last) {
  const int64_t B = q.size(0), H = q.size(1), S = q.size(2), D = q.size(3);
  const int64_t nc = S / 64;
  TORCH_CHECK(dout.is_cuda() && dout.scalar_type() == torch::kBFloat16 &&
                  dout.sizes() == q.sizes(),
              who, ": dout must be a bf16 device tensor shaped like q");
  for (const torch::Tensor* t : {&r, &drhs}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 &&
                    t->is_contiguous() && t->sizes() == q.sizes(),
                who, ": r and drhs must be contiguous fp32 (B, H, S, ", D, ")");
  }
  for (const torch::Tensor* t : {&s0, &ds0}) {
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == torch::kFloat32 &&
                    t->is_contiguous() && t->dim() == 5 && t->size(0) == B &&
                    t->size(1) == H && t->size(2) == nc &&
                    t->size(3) == D && t->size(4) == D,
                who, ": s0 and ds0 must be contiguous fp32 (B, H, S / 64, ", D,
                ", ", D, ")");
  }
  auto qc = q.contiguous();
  auto kc = k.contiguous();
  auto vc = v.contiguous();
  auto dc = dout.contiguous();
  auto bc = beta.to(torch::kFloat32).contiguous();
  auto gc = decay_log.to(torch::kFloat32).contiguous();
  auto f32 = torch::dtype(torch::kFloat32).device(q.device());
  auto dq = torch::empty({B, H, S, D}, f32);
  auto dk = torch::empty({B, H, S, D}, f32);
  auto dv = torch::empty({B, H, S, D}, f32);
  auto dbeta = torch::empty({B, H, S}, f32);
  auto dg = torch::empty({B, H, S}, f32);
  const int64_t n_chunks = B * H * nc;
  if (n_chunks == 0) return {dq, dk, dv, dbeta, dg};
  TORCH_CHECK(n_chunks < (int64_t)1 << 31, who, ": too many chunks for one grid");

  const bool wide = D == d9d::kGdnW;
  auto kern = wide ? &d9d::gdn_chunk_bwd_leaf_wide_kernel
                   : &d9d::gdn_chunk_bwd_leaf_kernel;
  const size_t lds =
      wide ? sizeof(d9d::GdnWideLeafLds) : sizeof(d9d::GdnLeafLds);
  static bool attr_set[2] = {false, false};   // one per kernel
  if (!attr_set[wide]) {
    hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set[wide] = true;
  }
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(kern, dim3((unsigned)n_chunks),
                     dim3(wide ? d9d::kGdnWT : 256), lds, stream,
                     reinterpret_cast<const __bf16*>(qc.data_ptr()),
                     reinterpret_cast<const __bf16*>(kc.data_ptr()),
                     reinterpret_cast<const __bf16*>(vc.data_ptr()),
                     reinterpret_cast<const __bf16*>(dc.data_ptr()),
                     bc.data_ptr<float>(), gc.data_ptr<float>(),
                     r.data_ptr<float>(), drhs.data_ptr<float>(),
                     s0.data_ptr<float>(), ds0.data_ptr<float>(),
                     dq.data_ptr<float>(), dk.data_ptr<float>(),
                     dv.data_ptr<float>(), dbeta.data_ptr<float>(),
                     dg.data_ptr<float>(),
                     doc_last.defined() ? doc_last.data_ptr<int>() : nullptr,
                     n_chunks, nc);
  return {dq, dk, dv, dbeta, dg};
}

// Packed documents in the chunk-aligned layout the backward gathers into:
// every cu_seqlens entry is a multiple of 64. Returns the (T / 64,) int32
// flags of the chunks that end a document, on q's device.
torch::Tensor gdn_leaf_doc_last(const char* who, const torch::Tensor& q,
                                const torch::Tensor& cu_seqlens) {
  const int64_t T = q.size(2);
  auto docs = gdn_check_docs(cu_seqlens, q.size(0), T, q.device(),
                             /*with_chunks=*/false);
  auto cu_cpu = cu_seqlens.cpu().contiguous();
  const int* cu = cu_cpu.data_ptr<int>();
  auto last = torch::zeros({T / 64}, torch::dtype(torch::kInt32));
  int* lp = last.data_ptr<int>();
  for (int64_t i = 0; i <= docs.nseq; ++i) {
    TORCH_CHECK(cu[i] % 64 == 0, who, ": cu_seqlens[", i, "] = ", cu[i],
                " is not a multiple of 64");
    if (i > 0 && cu[i] > cu[i - 1]) lp[cu[i] / 64 - 1] = 1;
  }
  return last.to(q.device());
}

// head dim exactly 128, for the wide leaf entry points (after the shared
// checks have established that q is 4-d)
void gdn_leaf_wide_check(const char* who, const torch::Tensor& q) {
  TORCH_CHECK(q.size(3) == d9d::kGdnW, who, " supports head dim 128, got ",
              q.size(3));
  TORCH_CHECK(q.size(2) % 64 == 0, who, ": S must be a multiple of 64, got ",
              q.size(2));
}

}  // namespace

// Per-chunk leaf gradients of the hand-derived backward: (dq, dk, dv) fp32
// (B, H, S, 64) and (dbeta, dg) fp32 (B, H, S) from the forward aux (r, s0)
// and the reverse scan's (drhs, ds0). S must be a multiple of 64.
std::vector<torch::Tensor> gdn_chunk_bwd_leaf(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor dout,
    torch::Tensor beta, torch::Tensor decay_log, torch::Tensor r,
    torch::Tensor drhs, torch::Tensor s0, torch::Tensor ds0) {
  gdn_dense_checks("gdn_chunk_bwd_leaf", q, k, v, beta, decay_log);
  TORCH_CHECK(q.size(2) % 64 == 0,
              "gdn_chunk_bwd_leaf: S must be a multiple of 64, got ", q.size(2));
  return gdn_bwd_leaf_impl("gdn_chunk_bwd_leaf", q, k, v, dout, beta,
                           decay_log, r, drhs, s0, ds0, torch::Tensor());
}

// Packed documents: the last chunk of each document takes dS1 = 0 instead of
// the next document's ds0.
std::vector<torch::Tensor> gdn_chunk_bwd_leaf_varlen(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor dout,
    torch::Tensor beta, torch::Tensor decay_log, torch::Tensor r,
    torch::Tensor drhs, torch::Tensor s0, torch::Tensor ds0,
    torch::Tensor cu_seqlens) {
  const char* who = "gdn_chunk_bwd_leaf_varlen";
  gdn_varlen_checks(who, q, k, v, beta, decay_log);
  return gdn_bwd_leaf_impl(who, q, k, v, dout, beta, decay_log, r, drhs, s0,
                           ds0, gdn_leaf_doc_last(who, q, cu_seqlens));
}

// The same two at head dim 128 (gdn_chunk_bwd_leaf_wide_kernel): (dq, dk, dv)
// fp32 (B, H, S, 128), r and drhs (B, H, S, 128), s0 and ds0
// (B, H, S / 64, 128, 128).
std::vector<torch::Tensor> gdn_chunk_bwd_leaf_wide(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor dout,
    torch::Tensor beta, torch::Tensor decay_log, torch::Tensor r,
    torch::Tensor drhs, torch::Tensor s0, torch::Tensor ds0) {
  const char* who = "gdn_chunk_bwd_leaf_wide";
  gdn_dense_checks(who, q, k, v, beta, decay_log, /*wide=*/true);
  gdn_leaf_wide_check(who, q);
  return gdn_bwd_leaf_impl(who, q, k, v, dout, beta, decay_log, r, drhs, s0,
                           ds0, torch::Tensor());
}

std::vector<torch::Tensor> gdn_chunk_bwd_leaf_wide_varlen(
    torch::Tensor q, torch::Tensor k, torch::Tensor v, torch::Tensor dout,
    torch::Tensor beta, torch::Tensor decay_log, torch::Tensor r,
    torch::Tensor drhs, torch::Tensor s0, torch::Tensor ds0,
    torch::Tensor cu_seqlens) {
  const char* who = "gdn_chunk_bwd_leaf_wide_varlen";
  gdn_varlen_checks(who, q, k, v, beta, decay_log, /*wide=*/true);
  gdn_leaf_wide_check(who, q);
  return gdn_bwd_leaf_impl(who, q, k, v, dout, beta, decay_log, r, drhs, s0,
                           ds0, gdn_leaf_doc_last(who, q, cu_seqlens));
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
  const int64_t D = qc.size(3);
  auto out = skip_out ? torch::Tensor() : torch::empty_like(vc);
  __bf16* out_ptr =
      skip_out ? nullptr : reinterpret_cast<__bf16*>(out.data_ptr());
  auto f32 = torch::dtype(torch::kFloat32).device(q.device());
  torch::Tensor fs;
  float* fs_ptr = nullptr;
  if (return_state) {
    fs = torch::empty({state_lead[0], state_lead[1], D, D}, f32);
    fs_ptr = fs.data_ptr<float>();
  }
  // aux outputs for the hand-derived backward: per-row solve results R and
  // the per-chunk entry states S0
  torch::Tensor r_aux, s0_aux;
  float* r_ptr = nullptr;
  float* s0_ptr = nullptr;
  if (return_aux) {
    r_aux = torch::empty({B, H, S, D}, f32);
    s0_aux = torch::empty({B, H, nc, D, D}, f32);
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
  gdn_dense_checks("gdn_chunk_fwd", q, k, v, beta, decay_log, /*wide=*/true);
  return gdn_chunk_fwd_impl<false>(
      q, k, v, beta, decay_log, return_state, return_aux, skip_out,
      {q.size(0), q.size(1)}, (q.size(2) + 63) / 64, nullptr, nullptr);
}

// Packed documents: q, k, v (1, H, T, D), D = 64 or 128, one workgroup per
// (document, head), zero state at each document start. Final state
// (nseq, H, D, D); aux r (1, H, T, D) by packed row, s0 (1, H, NC, D, D) by
// chunk_off[doc] + local chunk.
std::vector<torch::Tensor> gdn_chunk_fwd_varlen(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor beta, torch::Tensor decay_log, torch::Tensor cu_seqlens,
    bool return_state, bool return_aux, bool skip_out) {
  gdn_varlen_checks("gdn_chunk_fwd_varlen", q, k, v, beta, decay_log,
                    /*wide=*/true);
  auto docs = gdn_check_docs(cu_seqlens, q.size(0), q.size(2), q.device(),
                             /*with_chunks=*/true);
  return gdn_chunk_fwd_impl<true>(
      q, k, v, beta, decay_log, return_state, return_aux, skip_out,
      {docs.nseq, q.size(1)}, docs.nc, docs.cu_dev.data_ptr<int>(),
      docs.chunk_off_dev.data_ptr<int>());
}
