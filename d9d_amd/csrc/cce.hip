// Fused linear + cross-entropy for CDNA4 (gfx950): forward, and the
// tile-skipping backward.
//
// Replaces the cut-cross-entropy forward (reference: d9d/kernel/cce/cce.py
// cce_lse_forward_kernel): per token, lse over the full vocab and the target
// logit, WITHOUT materializing the (T, V) logits. The (T,V) GEMM runs on
// MFMA inside the kernel with an online logsumexp.
//
// Geometry: one block = 64 token rows (4 waves x 16-row m-tile). The token
// block's embeddings (64 x K bf16) live in LDS for the whole sweep; the
// classifier streams as (64 vocab x 64 k) tiles, T14-staged (loads issued a
// tile early into registers, written to the alternate LDS buffer after the
// MFMAs). All resident blocks sweep the vocab in the same order, so the
// classifier is served from L2/L3 after the first wavefront of blocks.
//
// K (hidden) is a runtime dim; K <= 1024 fits the 160 KiB LDS (the host
// falls back to the chunked rocBLAS path above that).
//
// BACKWARD (second half of this file). The logits of a row chunk are
// recomputed by the library GEMM and turned into dlogits in place. With the
// gradient filter on, a non-target dlogit with p < eps is exactly 0, so most
// 64-row x 128-column tiles of the chunk hold nothing but zeros.
// cce_dlogits_mask_ records which tiles do not (one byte per tile), and
// cce_bwd_de / cce_bwd_dc form de = d @ c and dc += d^T @ e from the set
// tiles alone. Dense chunks keep the library GEMMs; cce.py picks the route
// from the tile density of the previous backward.
#include "common.h"
#include "mfma.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace d9d {

constexpr float kLog2eC = 1.44269504088896340736f;

// KT = k-tile width (128 when K % 128 == 0): wider k-tiles double the MFMA
// work between barriers (16 vs 8 per wave); the classifier tile is
// single-buffered with T14 register staging (the registers are the second
// buffer), like the grouped-GEMM kernels.
template <int KT>
__global__ __launch_bounds__(512, 2) void cce_fwd_kernel(
    const bf16_t* __restrict__ e,   // (T, K)
    const bf16_t* __restrict__ c,   // (V, K)
    const int64_t* __restrict__ targets,  // (T,)
    float* __restrict__ lse_out,          // (T,)
    float* __restrict__ tgt_out,          // (T,) target logit or -inf
    float* __restrict__ lse_bf_out,       // (T,) lse of the bf16-ROUNDED logits
    int T, int V, int K) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* e_lds = reinterpret_cast<bf16_t*>(smem);       // [64][K] swizzled
  bf16_t* c_lds = e_lds + 64 * K;                        // [128][KT] swizzled
  // XOR swizzles must stay inside their LDS row. The classifier tile has
  // KT*2-byte rows. The e rows are K*2 bytes: a multiple of 256 when
  // K % 128 == 0 (always the case at KT == 128), but only of 128 otherwise,
  // where a 4-bit XOR would spill into the next row (and, from row 63, into
  // the classifier tile). So e_lds and c_lds both swizzle with kSwz: 3 bits
  // at KT == 64, 4 bits at KT == 128.
  constexpr int kSwz = (KT == 64) ? 7 : 15;

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;   // 8 waves: (vocab half) x (4 m-tiles)
  const int m_tile = wave & 3;
  const int vhalf = wave >> 2;
  const int t0 = blockIdx.x * 64;

  const int n_vtiles = (V + 127) / 128;  // 128-wide vocab tiles (2 x 64 halves)
  const int n_ktiles = K / KT;
  const int total_iters = n_vtiles * n_ktiles;

  constexpr int kCRegs = KT / 32;  // (128 * KT) / (512 threads * 8)
  bf16x8 c_reg[kCRegs];
  auto load_c = [&](int it_lin) {
    const int vt = it_lin / n_ktiles;
    const int kt = it_lin % n_ktiles;
#pragma unroll
    for (int i = 0; i < kCRegs; ++i) {
      const int idx = (threadIdx.x + i * 512) * 8;
      const int vrow = idx / KT;
      const int col = idx % KT;
      const int g_v = min(vt * 128 + vrow, V - 1);
      c_reg[i] = *reinterpret_cast<const bf16x8*>(
          c + (int64_t)g_v * K + kt * KT + col);
    }
  };
  auto store_c = [&]() {
#pragma unroll
    for (int i = 0; i < kCRegs; ++i) {
      const int idx = (threadIdx.x + i * 512) * 8;
      const int vrow = idx / KT;
      const int col = idx % KT;
      const int byte = (col * 2) ^ ((vrow & kSwz) << 4);
      *reinterpret_cast<bf16x8*>(
          reinterpret_cast<char*>(c_lds) + vrow * (KT * 2) + byte) = c_reg[i];
    }
  };

  // ---- stage e block (row-major [64][K], ((row&kSwz)<<4) swizzle) and the
  // first classifier tile; ONE barrier covers both ---------------------------
  for (int idx = threadIdx.x * 8; idx < 64 * K; idx += 512 * 8) {
    const int row = idx / K;
    const int col = idx % K;
    const int g_row = min(t0 + row, T - 1);
    const bf16x8 val = *reinterpret_cast<const bf16x8*>(e + (int64_t)g_row * K + col);
    const int byte = (col * 2) ^ ((row & kSwz) << 4);
    *reinterpret_cast<bf16x8*>(
        reinterpret_cast<char*>(e_lds) + row * (K * 2) + byte) = val;
  }
  load_c(0);
  store_c();
  __syncthreads();

  const int my_row_local = m_tile * 16 + (lane & 15);

  // lb_run: what the online sum gains when every logit z is rounded to bf16
  // (zb), to first order: sum exp(z - m) * (zb - z); exp(zb - z) - 1 - (zb - z)
  // is below (2^-9 z)^2 / 2: 5e-4 at |z| < 16 and 2e-3 at |z| < 32 (under the
  // 4e-3 bf16 step of the dlogits), 8e-3 at |z| < 64. The form assumes
  // |z| < 64; at |z| >= 128 the rounding step is 0.5 and it no longer holds. The backward recomputes the logits as a bf16
  // GEMM output, and exp(bf16 logit - lse) only sums to 1 over a row against
  // the lse of the ROUNDED logits: against the fp32 one every p is off by the
  // rounding of its own logit (up to 3% at |logit| in [8, 16)).
  float m_run[4], l_run[4], lb_run[4], tgt[4];
  int tg_row[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = -1e30f;
    l_run[r] = 0.f;
    lb_run[r] = 0.f;
    tgt[r] = -1e30f;
    tg_row[r] = (int)targets[min(t0 + m_tile * 16 + (lane >> 4) * 4 + r, T - 1)];
  }

  f32x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};

  for (int it = 0; it < total_iters; ++it) {
    const int vt = it / n_ktiles;
    const int kt = it % n_ktiles;
    if (it + 1 < total_iters) load_c(it + 1);  // issue early, store late

    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < KT / 32; ++ks) {
      const int kk = kt * KT + ks * 32 + (lane >> 4) * 8;
      const int ebyte = (kk * 2) ^ ((my_row_local & kSwz) << 4);
      const bf16x8 ea = *reinterpret_cast<const bf16x8*>(
          reinterpret_cast<char*>(e_lds) + my_row_local * (K * 2) + ebyte);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int vrow = vhalf * 64 + nt * 16 + (lane & 15);
        const int cbyte =
            ((ks * 32 + (lane >> 4) * 8) * 2) ^ ((vrow & kSwz) << 4);
        const bf16x8 cb = *reinterpret_cast<const bf16x8*>(
            reinterpret_cast<const char*>(c_lds) + vrow * (KT * 2) + cbyte);
        acc[nt] = mfma16(ea, cb, acc[nt]);
      }
    }
    __builtin_amdgcn_s_setprio(0);

    if (kt == n_ktiles - 1) {
      // Logits tile complete. PER-LANE online lse over this lane's own 4
      // columns — the 16-lane merge happens ONCE after the sweep, so the
      // hot epilogue has NO cross-lane shuffles (they were ~2/3 of the
      // per-tile VALU work: 96 shfl_xor per vocab tile).
      float vals[4][4];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int col = vt * 128 + vhalf * 64 + nt * 16 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          vals[nt][r] = (col < V) ? acc[nt][r] : -1e30f;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int col = vt * 128 + vhalf * 64 + nt * 16 + (lane & 15);
          if (col == (int)tg_row[r]) tgt[r] = fmaxf(tgt[r], vals[nt][r]);
        }
        const float mx = fmaxf(fmaxf(vals[0][r], vals[1][r]),
                               fmaxf(vals[2][r], vals[3][r]));
        const float m_new = fmaxf(m_run[r], mx);
        float add = 0.f, add_bf = 0.f;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const float ex =
              __builtin_amdgcn_exp2f((vals[nt][r] - m_new) * kLog2eC);
          add += ex;
          // native RNE convert on gfx950
          const float vb = static_cast<float>(static_cast<bf16_t>(vals[nt][r]));
          add_bf = fmaf(ex, vb - vals[nt][r], add_bf);
        }
        const float rescale =
            __builtin_amdgcn_exp2f((m_run[r] - m_new) * kLog2eC);
        l_run[r] = l_run[r] * rescale + add;
        lb_run[r] = lb_run[r] * rescale + add_bf;
        m_run[r] = m_new;
      }
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};
    }

    __syncthreads();
    if (it + 1 < total_iters) {
      store_c();
      __syncthreads();
    }
  }

  // ---- merge this wave's 16 col-lanes (once per kernel), then the two
  // vocab halves; write lse + target logit ----------------------------------
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int off = 1; off < 16; off <<= 1) {
      const float mo = __shfl_xor(m_run[r], off, 64);
      const float lo = __shfl_xor(l_run[r], off, 64);
      const float lbo = __shfl_xor(lb_run[r], off, 64);
      const float m2 = fmaxf(m_run[r], mo);
      const float sa = __builtin_amdgcn_exp2f((m_run[r] - m2) * kLog2eC);
      const float sb = __builtin_amdgcn_exp2f((mo - m2) * kLog2eC);
      l_run[r] = l_run[r] * sa + lo * sb;
      lb_run[r] = lb_run[r] * sa + lbo * sb;
      m_run[r] = m2;
      tgt[r] = fmaxf(tgt[r], __shfl_xor(tgt[r], off, 64));
    }
  }
  // scratch (reuses c_lds): per half, per row: lse, tgt and rounded lse.
  float* half_lse = reinterpret_cast<float*>(c_lds);          // [2][64]
  float* half_tgt = half_lse + 2 * 64;                        // [2][64]
  float* half_lbf = half_tgt + 2 * 64;                        // [2][64]
  __syncthreads();
  if ((lane & 15) == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row_l = m_tile * 16 + (lane >> 4) * 4 + r;
      half_lse[vhalf * 64 + row_l] = m_run[r] + __logf(fmaxf(l_run[r], 1e-30f));
      half_tgt[vhalf * 64 + row_l] = tgt[r];
      half_lbf[vhalf * 64 + row_l] =
          m_run[r] + __logf(fmaxf(l_run[r] + lb_run[r], 1e-30f));
    }
  }
  __syncthreads();
  if (vhalf == 0 && (lane & 15) == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row_l = m_tile * 16 + (lane >> 4) * 4 + r;
      const int row_g = t0 + row_l;
      if (row_g < T) {
        const float a = half_lse[row_l];
        const float b = half_lse[64 + row_l];
        const float mx = fmaxf(a, b);
        lse_out[row_g] = mx + __logf(
            __builtin_amdgcn_exp2f((a - mx) * kLog2eC) +
            __builtin_amdgcn_exp2f((b - mx) * kLog2eC));
        tgt_out[row_g] = fmaxf(half_tgt[row_l], half_tgt[64 + row_l]);
        const float ab = half_lbf[row_l];
        const float bb = half_lbf[64 + row_l];
        const float mb = fmaxf(ab, bb);
        lse_bf_out[row_g] = mb + __logf(
            __builtin_amdgcn_exp2f((ab - mb) * kLog2eC) +
            __builtin_amdgcn_exp2f((bb - mb) * kLog2eC));
      }
    }
  }
}

}  // namespace d9d

std::vector<torch::Tensor> cce_fwd(
    torch::Tensor e, torch::Tensor c, torch::Tensor targets) {
  TORCH_CHECK(e.is_cuda() && e.scalar_type() == torch::kBFloat16 && e.is_contiguous());
  TORCH_CHECK(c.scalar_type() == torch::kBFloat16 && c.is_contiguous());
  TORCH_CHECK(targets.scalar_type() == torch::kInt64);
  const int T = e.size(0), K = e.size(1), V = c.size(0);
  TORCH_CHECK(K % 64 == 0, "cce_fwd requires hidden % 64 == 0");
  const bool wide = (K % 128 == 0) &&
      (size_t)(64 * K + 128 * 128) * sizeof(__bf16) <= 160 * 1024;
  const size_t smem =
      (size_t)(64 * K + 128 * (wide ? 128 : 64)) * sizeof(__bf16);
  TORCH_CHECK(smem <= 160 * 1024, "cce_fwd: hidden too large for LDS: ", K);

  auto lse = torch::empty({T}, e.options().dtype(torch::kFloat32));
  auto tgt = torch::empty({T}, e.options().dtype(torch::kFloat32));
  auto lse_bf = torch::empty({T}, e.options().dtype(torch::kFloat32));
  if (T == 0) return {lse, tgt, lse_bf};
  auto stream = at::hip::getCurrentHIPStream();
  auto tgts = targets.contiguous();
#define LAUNCH_CCE(KT)                                                        \
  hipLaunchKernelGGL(d9d::cce_fwd_kernel<KT>, dim3((T + 63) / 64), dim3(512), \
                     smem, stream,                                            \
                     reinterpret_cast<const __bf16*>(e.data_ptr()),           \
                     reinterpret_cast<const __bf16*>(c.data_ptr()),           \
                     tgts.data_ptr<int64_t>(), lse.data_ptr<float>(),         \
                     tgt.data_ptr<float>(), lse_bf.data_ptr<float>(), T, V, K)
  if (wide) LAUNCH_CCE(128); else LAUNCH_CCE(64);
#undef LAUNCH_CCE
  return {lse, tgt, lse_bf};
}

namespace d9d {

// In-place CCE backward dlogits: p = exp(logit - lse) (fp32 math), minus the
// one-hot target, scaled by the per-row upstream grad -- replaces a 4-pass
// torch chain (sub, exp_, scatter_add_, mul_) over the (Tc, V) chunk with
// one read+write.
// One dlogit, bf16 bits in and out. Both dlogits kernels go through this, so
// the masked kernel's values are the plain kernel's bit for bit.
D9D_DEVICE ushort cce_dlogit_bits(ushort logit, float l, float g, float gp,
                                  bool is_tgt, float filter_eps) {
  float p = __builtin_amdgcn_exp2f((bf16_bits_to_f32(logit) - l) * 1.44269504089f);
  if (p < filter_eps && !is_tgt) p = 0.f;
  float out = p * gp - (is_tgt ? g : 0.f);
  return f32_to_bf16_rne(out);
}

__global__ void cce_dlogits_kernel(
    ushort* __restrict__ logits,       // (R, V) bf16, in/out
    const float* __restrict__ lse,     // (R,)
    const int64_t* __restrict__ targets,  // (R,) GLOBAL vocab ids (or ignore)
    const float* __restrict__ dl,      // (R,) upstream grad (0 for ignored)
    const float* __restrict__ dlse,    // (R,) upstream lse grad, or nullptr
    int64_t R, int64_t V, int64_t vocab_start, int64_t ignore_index,
    float filter_eps) {  // zero non-target dlogits with p < eps (<=0: off)
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 8;
  for (int64_t row = blockIdx.y; row < R; row += gridDim.y) {
  const float l = lse[row];
  const float g = dl[row];
  // d(lse)/d(logit) = p: a differentiable lse output simply adds its grad
  // to the softmax term's scale (loss term keeps -onehot * g).
  const float gp = g + (dlse ? dlse[row] : 0.f);
  const int64_t tgt_global = targets[row];
  const int64_t tgt =
      (tgt_global == ignore_index) ? -1 : tgt_global - vocab_start;
  ushort* rowp = logits + row * V;

  for (int64_t base = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
       base < V; base += stride) {
    if (base + 8 <= V) {
      Bf16x8 x;
      x.u = *reinterpret_cast<const ushort8v*>(rowp + base);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        x.s[j] = cce_dlogit_bits(x.s[j], l, g, gp, base + j == tgt, filter_eps);
      }
      *reinterpret_cast<ushort8v*>(rowp + base) = x.u;
    } else {
      for (int64_t i = base; i < V; ++i) {
        rowp[i] = cce_dlogit_bits(rowp[i], l, g, gp, i == tgt, filter_eps);
      }
    }
  }
  }
}

}  // namespace d9d

torch::Tensor cce_dlogits_(torch::Tensor logits, torch::Tensor lse,
                           torch::Tensor targets, torch::Tensor dl,
                           c10::optional<torch::Tensor> dlse,
                           int64_t vocab_start, int64_t ignore_index,
                           double filter_eps) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == torch::kBFloat16 &&
              logits.is_contiguous());
  const int64_t R = logits.size(0), V = logits.size(1);
  if (R == 0) return logits;
  const int gx = (int)std::min<int64_t>((V + 256 * 8 - 1) / (256 * 8), 128);
  const unsigned gy = (unsigned)std::min<int64_t>(R, 4096 / gx + 1);
  auto stream = at::hip::getCurrentHIPStream();
  torch::Tensor dlse_c;
  const float* dlse_ptr = nullptr;
  if (dlse.has_value()) {
    dlse_c = dlse->contiguous();
    dlse_ptr = dlse_c.data_ptr<float>();
  }
  hipLaunchKernelGGL(d9d::cce_dlogits_kernel, dim3(gx, gy), dim3(256),
                     0, stream,
                     reinterpret_cast<ushort*>(logits.data_ptr()),
                     lse.contiguous().data_ptr<float>(),
                     targets.contiguous().data_ptr<int64_t>(),
                     dl.contiguous().data_ptr<float>(), dlse_ptr,
                     R, V, vocab_start,
                     ignore_index, (float)filter_eps);
  return logits;
}

// ===========================================================================
// Tile-skipping backward
// ===========================================================================

namespace d9d {

constexpr int kMaskRows = 64;    // mask tile: 64 rows x 128 vocab columns
constexpr int kMaskCols = 128;

// cce_dlogits_kernel's values plus the tile mask. One block owns 64 rows x
// 512 columns (four mask tiles): wave w takes rows w, w + 4, ..., a lane one
// 8-column group of each, all sixteen loaded before the first is used. A tile
// owned by one block is what lets WRITE_ZEROS == false skip whole tiles: the
// block knows that a tile is all zero before it writes any of it. (Skipping
// single all-zero groups would leave the logits they held inside tiles that
// the consumers do read.) Every mask byte is written, 0 or 1, so the mask
// needs no clearing.
template <bool WRITE_ZEROS>
__global__ __launch_bounds__(256) void cce_dlogits_mask_kernel(
    ushort* __restrict__ logits,          // (R, V) bf16, in/out
    const float* __restrict__ lse,        // (R,)
    const int64_t* __restrict__ targets,  // (R,) GLOBAL vocab ids (or ignore)
    const float* __restrict__ dl,         // (R,)
    const float* __restrict__ dlse,       // (R,) or nullptr
    uint8_t* __restrict__ mask,           // (ceil(R/64), n_vt)
    int64_t R, int64_t V, int64_t n_vt, int64_t vocab_start,
    int64_t ignore_index, float filter_eps) {
  __shared__ int tile_nz[4];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.y * kMaskRows;
  const int64_t base = (int64_t)blockIdx.x * 512 + lane * 8;
  // columns of this lane's group that exist: 8, 0, or the row's tail
  const int nvalid = (int)max((int64_t)0, min((int64_t)8, V - base));
  if (threadIdx.x < 4) tile_nz[threadIdx.x] = 0;
  __syncthreads();

  Bf16x8 x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int64_t row = r0 + wave + 4 * i;
#pragma unroll
    for (int j = 0; j < 8; ++j) x[i].s[j] = 0;
    if (row < R) {
      const ushort* src = logits + row * V + base;
      if (nvalid == 8) {
        x[i].u = *reinterpret_cast<const ushort8v*>(src);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          if (j < nvalid) x[i].s[j] = src[j];
        }
      }
    }
  }

  bool nz = false;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int64_t row = r0 + wave + 4 * i;
    if (row < R) {
      const float l = lse[row];
      const float g = dl[row];
      const float gp = g + (dlse ? dlse[row] : 0.f);
      const int64_t tgt_global = targets[row];
      const int64_t tgt =
          (tgt_global == ignore_index) ? -1 : tgt_global - vocab_start;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (j < nvalid) {
          x[i].s[j] =
              cce_dlogit_bits(x[i].s[j], l, g, gp, base + j == tgt, filter_eps);
          nz |= (x[i].s[j] & 0x7fff) != 0;  // -0 is a zero
        }
      }
    }
  }
  if (nz) tile_nz[lane >> 4] = 1;
  __syncthreads();

  if (nvalid > 0 && (WRITE_ZEROS || tile_nz[lane >> 4])) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int64_t row = r0 + wave + 4 * i;
      if (row < R) {
        ushort* dst = logits + row * V + base;
        if (nvalid == 8) {
          *reinterpret_cast<ushort8v*>(dst) = x[i].u;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            if (j < nvalid) dst[j] = x[i].s[j];
          }
        }
      }
    }
  }
  if (threadIdx.x < 4) {
    const int64_t vt = (int64_t)blockIdx.x * 4 + threadIdx.x;
    if (vt < n_vt) {
      mask[(int64_t)blockIdx.y * n_vt + vt] = (uint8_t)tile_nz[threadIdx.x];
    }
  }
}

// 16 bytes of a dlogits row, zeros where the row or the columns do not exist.
D9D_DEVICE ushort8v cce_load_d8(const ushort* __restrict__ d, int64_t row,
                                int64_t col, int64_t R, int64_t V) {
  Bf16x8 x;
#pragma unroll
  for (int j = 0; j < 8; ++j) x.s[j] = 0;
  if (row < R && col < V) {
    const ushort* src = d + row * V + col;
    if (col + 8 <= V) {
      x.u = *reinterpret_cast<const ushort8v*>(src);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (col + j < V) x.s[j] = src[j];
      }
    }
  }
  return x.u;
}

// 16 bytes of row `row` of a (rows, K) matrix at column `col`, or zeros.
// K % 8 == 0, so a group is inside the row or outside it.
D9D_DEVICE ushort8v cce_load_row8(const ushort* __restrict__ m, int64_t row,
                                  int col, int64_t rows, int K) {
  Bf16x8 x;
#pragma unroll
  for (int j = 0; j < 8; ++j) x.s[j] = 0;
  if (row < rows && col < K) {
    x.u = *reinterpret_cast<const ushort8v*>(m + row * K + col);
  }
  return x.u;
}

constexpr int kDeKS = 128;        // hidden columns per cce_bwd_de block
constexpr int kDeLd = 128 + 8;    // LDS row pitch (elements): 16-byte aligned
                                  // rows 4 banks apart for the fragment reads

// de[64 rows, 128 hidden] = sum over the SET vocab tiles of the row block of
// d_tile (64 x 128) @ c_tile (128 x 128). 8 waves: (4 m-tiles) x (2 halves of
// the hidden slice). The A fragment (8 consecutive vocab columns of one row)
// is read straight from the row-major d tile; the B fragment (8 consecutive
// vocab rows of one hidden column) needs c transposed, which the staging does
// with two-byte LDS stores: lanes 0..31 of a wave take 32 vocab rows, so the
// stores of one j land in 32 different banks.
__global__ __launch_bounds__(512) void cce_bwd_de_kernel(
    const ushort* __restrict__ d,      // (R, V) bf16 dlogits
    const ushort* __restrict__ c,      // (V, K) bf16
    const uint8_t* __restrict__ mask,  // (n_rb, n_vt)
    ushort* __restrict__ de,           // (R, K) bf16
    int64_t R, int64_t V, int K, int n_vt) {
  __shared__ __attribute__((aligned(16))) ushort d_lds[64 * kDeLd];
  __shared__ __attribute__((aligned(16))) ushort ct_lds[kDeKS * kDeLd];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int m_tile = wave & 3;
  const int nh = wave >> 2;
  const int64_t r0 = (int64_t)blockIdx.x * 64;
  const int k0 = blockIdx.y * kDeKS;

  f32x4 acc[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};

  const uint8_t* mrow = mask + (int64_t)blockIdx.x * n_vt;
  for (int vt0 = 0; vt0 < n_vt; vt0 += 64) {
    const uint8_t mb = (vt0 + lane < n_vt) ? mrow[vt0 + lane] : (uint8_t)0;
    unsigned long long bits = __ballot(mb != 0);  // same in all 8 waves
    while (bits) {
      const int vt = vt0 + __builtin_ctzll(bits);
      bits &= bits - 1;
      __syncthreads();  // the previous tile's fragment reads are done
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int idx = threadIdx.x + i * 512;
        const int row = idx >> 4, g = idx & 15;
        *reinterpret_cast<ushort8v*>(&d_lds[row * kDeLd + g * 8]) =
            cce_load_d8(d, r0 + row, (int64_t)vt * 128 + g * 8, R, V);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int unit = wave * 4 + i;  // 32 units: (4 x 32 vocab) x (8 x 16 hidden)
        const int v = (unit & 3) * 32 + (lane & 31);
        const int h = (unit >> 2) * 16 + (lane >> 5) * 8;
        Bf16x8 x;
        x.u = cce_load_row8(c, (int64_t)vt * 128 + v, k0 + h, V, K);
#pragma unroll
        for (int j = 0; j < 8; ++j) ct_lds[(h + j) * kDeLd + v] = x.s[j];
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const int kk = ks * 32 + (lane >> 4) * 8;
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(
            &d_lds[(m_tile * 16 + (lane & 15)) * kDeLd + kk]);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(
              &ct_lds[(nh * 64 + nt * 16 + (lane & 15)) * kDeLd + kk]);
          acc[nt] = mfma16(a, b, acc[nt]);
        }
      }
    }
  }

  // a row block with no set tile writes zeros: de is not cleared by the host
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int col = k0 + nh * 64 + nt * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = r0 + m_tile * 16 + (lane >> 4) * 4 + r;
      if (row < R && col < K) de[row * K + col] = f32_to_bf16_rne(acc[nt][r]);
    }
  }
}

constexpr int kDcKS = 256;      // hidden columns per cce_bwd_dc block
constexpr int kDcLd = 64 + 8;   // LDS row pitch (elements), as kDeLd

enum { kDcWriteBf16 = 0, kDcInitF32 = 1, kDcAddF32 = 2 };

// part[128 vocab, 256 hidden] = sum over the SET row blocks of the vocab tile
// of d_tile^T (128 x 64) @ e_block (64 x 256). The reduction runs over rows,
// the slow dimension of both d and e, so both operands are staged transposed
// (lane = row: the two-byte stores of one j land in 32 banks). 8 waves, one
// 16-row m-tile of the vocab tile each, 16 n-tiles. One block owns its
// outputs: no atomics, and the row blocks are summed in order.
// MODE: write the bf16 result; or round it to bf16 and initialise / add to
// the fp32 accumulator (the rounding the chunked GEMM path has).
template <int MODE>
__global__ __launch_bounds__(512) void cce_bwd_dc_kernel(
    const ushort* __restrict__ d,      // (R, V) bf16 dlogits
    const ushort* __restrict__ e,      // (R, K) bf16
    const uint8_t* __restrict__ mask,  // (n_rb, n_vt)
    void* __restrict__ out,            // (V, K) bf16 or fp32
    int64_t R, int64_t V, int K, int n_rb, int n_vt) {
  __shared__ __attribute__((aligned(16))) ushort dt_lds[128 * kDcLd];
  __shared__ __attribute__((aligned(16))) ushort et_lds[kDcKS * kDcLd];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int vt = blockIdx.x;
  const int k0 = blockIdx.y * kDcKS;

  f32x4 acc[16];
#pragma unroll
  for (int nt = 0; nt < 16; ++nt) acc[nt] = {0.f, 0.f, 0.f, 0.f};

  bool any = false;
  for (int rb0 = 0; rb0 < n_rb; rb0 += 64) {
    const uint8_t mb = (rb0 + lane < n_rb)
        ? mask[(int64_t)(rb0 + lane) * n_vt + vt] : (uint8_t)0;
    unsigned long long bits = __ballot(mb != 0);  // same in all 8 waves
    while (bits) {
      const int rb = rb0 + __builtin_ctzll(bits);
      bits &= bits - 1;
      any = true;
      const int64_t row = (int64_t)rb * 64 + lane;
      __syncthreads();  // the previous block's fragment reads are done
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int g = wave * 2 + i;  // 16 groups of 8 vocab columns
        Bf16x8 x;
        x.u = cce_load_d8(d, row, (int64_t)vt * 128 + g * 8, R, V);
#pragma unroll
        for (int j = 0; j < 8; ++j) dt_lds[(g * 8 + j) * kDcLd + lane] = x.s[j];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int h = (wave * 4 + i) * 8;  // 32 groups of 8 hidden columns
        Bf16x8 x;
        x.u = cce_load_row8(e, row, k0 + h, R, K);
#pragma unroll
        for (int j = 0; j < 8; ++j) et_lds[(h + j) * kDcLd + lane] = x.s[j];
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int kk = ks * 32 + (lane >> 4) * 8;
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(
            &dt_lds[(wave * 16 + (lane & 15)) * kDcLd + kk]);
#pragma unroll
        for (int nt = 0; nt < 16; ++nt) {
          const bf16x8 b = *reinterpret_cast<const bf16x8*>(
              &et_lds[(nt * 16 + (lane & 15)) * kDcLd + kk]);
          acc[nt] = mfma16(a, b, acc[nt]);
        }
      }
    }
  }

  if (MODE == kDcAddF32 && !any) return;  // adds nothing
#pragma unroll
  for (int nt = 0; nt < 16; ++nt) {
    const int col = k0 + nt * 16 + (lane & 15);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t v = (int64_t)vt * 128 + wave * 16 + (lane >> 4) * 4 + r;
      if (v < V && col < K) {
        const ushort b = f32_to_bf16_rne(acc[nt][r]);
        if (MODE == kDcWriteBf16) {
          static_cast<ushort*>(out)[v * K + col] = b;
        } else if (MODE == kDcInitF32) {
          static_cast<float*>(out)[v * K + col] = bf16_bits_to_f32(b);
        } else {
          static_cast<float*>(out)[v * K + col] += bf16_bits_to_f32(b);
        }
      }
    }
  }
}

}  // namespace d9d

namespace {

void cce_check_mask(const torch::Tensor& mask, const torch::Tensor& d,
                    const char* op) {
  const int64_t R = d.size(0), V = d.size(1);
  TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == torch::kUInt8 &&
                  mask.is_contiguous(),
              op, ": mask must be a contiguous uint8 tensor on the GPU");
  TORCH_CHECK(mask.dim() == 2 &&
                  mask.size(0) == (R + d9d::kMaskRows - 1) / d9d::kMaskRows &&
                  mask.size(1) == (V + d9d::kMaskCols - 1) / d9d::kMaskCols,
              op, ": mask must be (ceil(R/64), ceil(V/128)) = (",
              (R + 63) / 64, ", ", (V + 127) / 128, "), got ", mask.sizes());
}

void cce_check_bf16_2d(const torch::Tensor& t, const char* op,
                       const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                  t.dim() == 2 && t.is_contiguous(),
              op, ": ", name, " must be a contiguous 2-d bf16 tensor on the GPU");
}

void cce_check_f32_rows(const torch::Tensor& t, int64_t R, const char* op,
                        const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 &&
                  t.dim() == 1 && t.size(0) == R && t.is_contiguous(),
              op, ": ", name, " must be a contiguous fp32 (R,) tensor on the GPU");
}

}  // namespace

torch::Tensor cce_dlogits_mask_(torch::Tensor logits, torch::Tensor lse,
                                torch::Tensor targets, torch::Tensor dl,
                                c10::optional<torch::Tensor> dlse,
                                torch::Tensor mask, int64_t vocab_start,
                                int64_t ignore_index, double filter_eps,
                                bool write_zeros) {
  const char* op = "cce_dlogits_mask_";
  cce_check_bf16_2d(logits, op, "logits");
  const int64_t R = logits.size(0), V = logits.size(1);
  cce_check_f32_rows(lse, R, op, "lse");
  cce_check_f32_rows(dl, R, op, "dl");
  if (dlse.has_value()) cce_check_f32_rows(*dlse, R, op, "dlse");
  TORCH_CHECK(targets.is_cuda() && targets.scalar_type() == torch::kInt64 &&
                  targets.dim() == 1 && targets.size(0) == R &&
                  targets.is_contiguous(),
              op, ": targets must be a contiguous int64 (R,) tensor on the GPU");
  cce_check_mask(mask, logits, op);
  if (R == 0 || V == 0) return logits;
  const int64_t n_vt = mask.size(1);
  TORCH_CHECK(mask.size(0) <= 65535, op, ": too many rows: ", R);
  const dim3 grid((unsigned)((V + 511) / 512), (unsigned)mask.size(0));
  auto stream = at::hip::getCurrentHIPStream();
#define LAUNCH_DLM(WZ)                                                        \
  hipLaunchKernelGGL(d9d::cce_dlogits_mask_kernel<WZ>, grid, dim3(256), 0,    \
                     stream, reinterpret_cast<ushort*>(logits.data_ptr()),    \
                     lse.data_ptr<float>(), targets.data_ptr<int64_t>(),      \
                     dl.data_ptr<float>(),                                    \
                     dlse.has_value() ? dlse->data_ptr<float>() : nullptr,    \
                     mask.data_ptr<uint8_t>(), R, V, n_vt, vocab_start,       \
                     ignore_index, (float)filter_eps)
  if (write_zeros) LAUNCH_DLM(true); else LAUNCH_DLM(false);
#undef LAUNCH_DLM
  return logits;
}

void cce_bwd_de(torch::Tensor d, torch::Tensor c, torch::Tensor mask,
                torch::Tensor de) {
  const char* op = "cce_bwd_de";
  cce_check_bf16_2d(d, op, "d");
  cce_check_bf16_2d(c, op, "c");
  cce_check_bf16_2d(de, op, "de");
  const int64_t R = d.size(0), V = d.size(1), K = c.size(1);
  TORCH_CHECK(c.size(0) == V, op, ": c must have V = ", V, " rows");
  TORCH_CHECK(de.size(0) == R && de.size(1) == K, op, ": de must be (R, K)");
  TORCH_CHECK(K % 64 == 0 && K >= 64 && K <= 1024, op,
              ": hidden must be a multiple of 64 up to 1024, got ", K);
  cce_check_mask(mask, d, op);
  if (R == 0) return;
  const dim3 grid((unsigned)mask.size(0), (unsigned)((K + d9d::kDeKS - 1) / d9d::kDeKS));
  hipLaunchKernelGGL(d9d::cce_bwd_de_kernel, grid, dim3(512), 0,
                     at::hip::getCurrentHIPStream(),
                     reinterpret_cast<const ushort*>(d.data_ptr()),
                     reinterpret_cast<const ushort*>(c.data_ptr()),
                     mask.data_ptr<uint8_t>(),
                     reinterpret_cast<ushort*>(de.data_ptr()), R, V, (int)K,
                     (int)mask.size(1));
}

void cce_bwd_dc(torch::Tensor d, torch::Tensor e, torch::Tensor mask,
                torch::Tensor dc, bool accumulate) {
  const char* op = "cce_bwd_dc";
  cce_check_bf16_2d(d, op, "d");
  cce_check_bf16_2d(e, op, "e");
  const int64_t R = d.size(0), V = d.size(1), K = e.size(1);
  TORCH_CHECK(e.size(0) == R, op, ": e must have R = ", R, " rows");
  TORCH_CHECK(K % 64 == 0 && K >= 64 && K <= 1024, op,
              ": hidden must be a multiple of 64 up to 1024, got ", K);
  const bool f32 = dc.scalar_type() == torch::kFloat32;
  TORCH_CHECK(dc.is_cuda() && dc.is_contiguous() && dc.dim() == 2 &&
                  dc.size(0) == V && dc.size(1) == K &&
                  (f32 || dc.scalar_type() == torch::kBFloat16),
              op, ": dc must be a contiguous (V, K) bf16 or fp32 tensor on the GPU");
  TORCH_CHECK(f32 || !accumulate, op, ": accumulation needs an fp32 dc");
  cce_check_mask(mask, d, op);
  if (V == 0) return;
  const dim3 grid((unsigned)mask.size(1), (unsigned)((K + d9d::kDcKS - 1) / d9d::kDcKS));
  auto stream = at::hip::getCurrentHIPStream();
#define LAUNCH_DC(MODE)                                                       \
  hipLaunchKernelGGL(d9d::cce_bwd_dc_kernel<MODE>, grid, dim3(512), 0, stream,\
                     reinterpret_cast<const ushort*>(d.data_ptr()),           \
                     reinterpret_cast<const ushort*>(e.data_ptr()),           \
                     mask.data_ptr<uint8_t>(), dc.data_ptr(), R, V, (int)K,   \
                     (int)mask.size(0), (int)mask.size(1))
  if (!f32) LAUNCH_DC(d9d::kDcWriteBf16);
  else if (accumulate) LAUNCH_DC(d9d::kDcAddF32);
  else LAUNCH_DC(d9d::kDcInitF32);
#undef LAUNCH_DC
}
