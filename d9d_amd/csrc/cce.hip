// Fused linear + cross-entropy for CDNA4 (gfx950): forward, and the
// tile-skipping backward.
//
// Replaces the cut-cross-entropy forward (reference: d9d/kernel/cce/cce.py
// cce_lse_forward_kernel): per token, lse over the full vocab and the target
// logit, WITHOUT materializing the (T, V) logits. The (T,V) GEMM runs on
// MFMA inside the kernel with an online logsumexp.
//
// FORWARD. The GEMM is e (T, K) against c (V, K), both k-contiguous: the
// grouped GEMM's (E, N, K) case with one expert, and cce_fwd_tiled_kernel
// runs it on that kernel's loop (gmm_8phase_kernel<256, false>, gmm.hip):
// 256 token rows x 256 vocab columns per tile, 64-wide k-tiles staged by
// global_load_lds into two 64 KB LDS slots behind counted vmcnt waits, 8 waves
// as 2 x 4 with a 128 x 64 accumulator each. A block keeps one row tile and
// walks a contiguous span of vocab tiles; the k-tile pipeline runs straight
// through the vocab-tile boundaries. When a tile's logits are complete each
// wave folds its 128 x 64 of them into a running (m, l, lb) per row, kept in
// LDS per column quarter, and picks up the target logit by column compare.
// Each block writes its rows' partial (m, l, lb, tgt) to a workspace and
// cce_fwd_merge_kernel combines the spans of a row in span order: no atomics,
// the same bits on every launch.
//
// K (hidden) is a runtime dim, a multiple of 64.
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
#include "glds_tile.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace d9d {

constexpr float kLog2eC = 1.44269504088896340736f;

constexpr int kFwdTile = 256;                // token rows = vocab columns per tile
constexpr int kFwdSlot = (256 + 256) * 128;  // one k-tile: A 32 KB + B 32 KB
// Row tiles that run side by side on one XCD. Work ids go row tile fastest
// inside a group of this many, then span, then group (see the kernel), and
// xcd_remap hands an XCD consecutive ids: its 32 CUs hold 8 row tiles x 4
// spans, so 8 e tiles (3 MB at K = 768) stay in its 4 MB L2 and each
// classifier k-tile it fetches serves 8 blocks.
constexpr int kFwdRowGroup = 8;
// LDS behind the two slots: (m, l, lb) per column quarter and row, the target
// logit and the target column per row.
constexpr int kFwdStateFloats = 3 * 4 * kFwdTile + 2 * kFwdTile;
constexpr int kFwdLds = 2 * kFwdSlot + kFwdStateFloats * 4;

// A lane's value as seen from another lane of its 16-lane DPP row.
template <int CTRL>
D9D_DEVICE float dpp_row(float v) {
  const int x = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, true));
}
// Reductions over the 16 lanes that share lane >> 4 (the 16 columns of one
// accumulator subtile): quad_perm [1,0,3,2], quad_perm [2,3,0,1],
// row_half_mirror, row_mirror. After the two quad steps a quad is uniform,
// so the mirrors bring in the other quad and then the other half. The order
// is fixed, and every lane ends with the same bits.
D9D_DEVICE float row16_max(float v) {
  v = fmaxf(v, dpp_row<0xB1>(v));
  v = fmaxf(v, dpp_row<0x4E>(v));
  v = fmaxf(v, dpp_row<0x141>(v));
  return fmaxf(v, dpp_row<0x140>(v));
}
D9D_DEVICE float row16_sum(float v) {
  v += dpp_row<0xB1>(v);
  v += dpp_row<0x4E>(v);
  v += dpp_row<0x141>(v);
  return v + dpp_row<0x140>(v);
}

// gmm_8phase_kernel's stage_a (gmm.hip) as a function. One thread's two glds
// of a 128-row half (16 KB) of a 256-row, k-contiguous A tile: rows
// row0 + half * 128 .. of the (rows, K) matrix `a` at k offset k0, into a_slot + half * 16 KB. The tile is [256][kBK] row-major with the
// row-keyed swizzle, produced by PRE-SWIZZLING the per-lane global source
// address (glds writes linearly: wave-uniform base + lane*16). Rows at or past
// row_end are clamped to row_end - 1.
D9D_DEVICE void stage_a_half(const bf16_t* __restrict__ a, char* a_slot,
                             int k0, int row0, int row_end, int K, int half,
                             int wave, int lane) {
  char* base = a_slot + half * (16 * 1024);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int chunk = wave + i * 8;           // 16 chunks of 1 KB
    const int l = chunk * 1024 + lane * 16;   // linear LDS byte in half
    const int arow = half * 128 + (l >> 7);   // tile row (128-B rows)
    const int colb = (l & 127) ^ ((arow & 7) << 4);  // source pre-swizzle
    const int64_t sr = min(row0 + arow, row_end - 1);
    glds16(reinterpret_cast<const char*>(a) + (sr * (int64_t)K + k0) * 2 + colb,
           base + l);
  }
}

// Forward main kernel: partial (m, l, lb, tgt) of one 256-row tile over one
// span of vocab tiles. The loop is gmm_8phase_kernel<256, false>'s (gmm.hip)
// with the linear iteration `it` over (vocab tile, k-tile) in place of kt:
// same slots (parity of it), same staging order, same counted waits, same raw
// barriers; see the schedule written out above that kernel. A(it) is the e
// k-tile it % n_ktiles, B(it) the classifier k-tile of its vocab tile, so the
// staging of the next vocab tile is in flight while a tile's epilogue runs.
// Every logit accumulates its 32-wide k-steps in ascending order in one chain.
__global__ __launch_bounds__(512, 1) void cce_fwd_tiled_kernel(
    const bf16_t* __restrict__ e,         // (T, K)
    const bf16_t* __restrict__ c,         // (V, K)
    const int64_t* __restrict__ targets,  // (T,) local column, or outside [0, V)
    float* __restrict__ ws,               // (4, n_spans, T): m, l, lb, tgt
    int T, int V, int K, int n_rt, int n_spans) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* st_m = reinterpret_cast<float*>(smem + 2 * kFwdSlot);  // [4][256]
  float* st_l = st_m + 4 * kFwdTile;                            // [4][256]
  float* st_lb = st_l + 4 * kFwdTile;                           // [4][256]
  float* tgt_lds = st_lb + 4 * kFwdTile;                        // [256]
  int* tg_lds = reinterpret_cast<int*>(tgt_lds + kFwdTile);     // [256]

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 2;   // row half: 128 rows
  const int wn = wave & 3;    // column quarter: 64 columns

  // work id -> (row tile, span): row tile fastest within a group of
  // kFwdRowGroup row tiles (the last group may be smaller), then span.
  const int wid = xcd_remap(blockIdx.x, gridDim.x);
  const int per_group = kFwdRowGroup * n_spans;
  const int rg = wid / per_group;
  const int gs = min(kFwdRowGroup, n_rt - rg * kFwdRowGroup);
  const int rem = wid - rg * per_group;
  const int span = rem / gs;
  const int row0 = (rg * kFwdRowGroup + rem % gs) * kFwdTile;

  const int n_vt = (V + kFwdTile - 1) / kFwdTile;
  const int vt_lo = (int)((int64_t)span * n_vt / n_spans);
  const int vt_hi = (int)((int64_t)(span + 1) * n_vt / n_spans);
  const int n_ktiles = K / kBK;
  const int n_it = (vt_hi - vt_lo) * n_ktiles;

  // lb: what the online sum gains when every logit z is rounded to bf16
  // (zb), to first order: sum exp(z - m) * (zb - z); exp(zb - z) - 1 - (zb - z)
  // is below (2^-9 z)^2 / 2: 5e-4 at |z| < 16 and 2e-3 at |z| < 32 (under the
  // 4e-3 bf16 step of the dlogits), 8e-3 at |z| < 64. The form assumes
  // |z| < 64; at |z| >= 128 the rounding step is 0.5 and it no longer holds.
  // The backward recomputes the logits as a bf16 GEMM output, and
  // exp(bf16 logit - lse) only sums to 1 over a row against
  // the lse of the ROUNDED logits: against the fp32 one every p is off by the
  // rounding of its own logit (up to 3% at |logit| in [8, 16)).
  for (int i = threadIdx.x; i < 4 * kFwdTile; i += 512) {
    st_m[i] = -1e30f;
    st_l[i] = 0.f;
    st_lb[i] = 0.f;
  }
  if (threadIdx.x < kFwdTile) {
    tgt_lds[threadIdx.x] = -1e30f;
    tg_lds[threadIdx.x] = (int)targets[min(row0 + (int)threadIdx.x, T - 1)];
  }
  __syncthreads();  // before the first glds: the counted waits start clean
  // two of this wave's 128 rows per lane, for the per-tile target test
  const int tg_a = tg_lds[wm * 128 + lane];
  const int tg_b = tg_lds[wm * 128 + 64 + lane];

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  auto stage_a = [&](int it_x, int kt_x, int half) {
    stage_a_half(e, smem + (size_t)(it_x & 1) * kFwdSlot, kt_x * kBK, row0, T,
                 K, half, wave, lane);
  };
  auto stage_b = [&](int it_x, int vt_x, int kt_x, int chunk) {
    Tile8BNK<256>::stage(c, smem + (size_t)(it_x & 1) * kFwdSlot + 32 * 1024,
                         kt_x * kBK, vt_x * kFwdTile, K, V, chunk, wave, lane);
  };
  auto advance = [&](int& vt_x, int& kt_x) {
    if (++kt_x == n_ktiles) { kt_x = 0; ++vt_x; }
  };

  // Logits of vocab tile vt are complete in acc: fold this wave's 128 rows x
  // 64 columns into the rows' running state of column quarter wn. Only this
  // wave touches that state, so the epilogue needs no barrier.
  auto epilogue = [&](int vt) {
    const int col_lo = vt * kFwdTile + wn * 64;
    const int lcol = col_lo + (lane & 15);  // column of subtile j: lcol + 16 j
    if (col_lo + 64 > V) {  // padded columns (the last tile only)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (lcol + j * 16 >= V) {
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[i][j] = {-1e30f, -1e30f, -1e30f, -1e30f};
        }
      }
    }
    // Target by column compare, only where one of the wave's rows has its
    // target among these 64 columns. One (row, column) has one owner in the
    // whole grid, so a plain store does it. A target at or past V (another
    // shard's) is left at -1e30.
    const bool hit = (unsigned)(tg_a - col_lo) < 64u || (unsigned)(tg_b - col_lo) < 64u;
    // (rbase goes through an empty asm so that the addresses derived from it
    // are formed here, as base + immediate, and not kept in registers across
    // the main loop, where they spill.)
    int rbase = wm * 128 + (lane >> 4) * 4;  // row of subtile i, register r: rbase + 16 i + r
    asm volatile("" : "+v"(rbase));
    if (__ballot(hit)) {
      const int* tg_p = tg_lds + rbase;
      float* tgt_p = tgt_lds + rbase;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int tg = tg_p[i * 16 + r];
          const int d = tg - lcol;
          float val = acc[i][0][r];
#pragma unroll
          for (int j = 1; j < 4; ++j) val = (d == j * 16) ? acc[i][j][r] : val;
          if ((d & ~48) == 0 && tg < V) tgt_p[i * 16 + r] = val;
        }
      }
    }
    float* st_p = st_m + wn * kFwdTile + rbase;  // l and lb: 4 and 8 * kFwdTile on
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      // one row subtile at a time: scheduled together, the eight subtiles'
      // state and temporaries do not fit beside the accumulators
      __builtin_amdgcn_sched_barrier(0);
      f32x4 m4 = *reinterpret_cast<const f32x4*>(st_p + i * 16);
      f32x4 l4 = *reinterpret_cast<const f32x4*>(st_p + 4 * kFwdTile + i * 16);
      f32x4 lb4 = *reinterpret_cast<const f32x4*>(st_p + 8 * kFwdTile + i * 16);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float mx = row16_max(fmaxf(fmaxf(acc[i][0][r], acc[i][1][r]),
                                         fmaxf(acc[i][2][r], acc[i][3][r])));
        const float m_new = fmaxf(m4[r], mx);
        float add = 0.f, add_bf = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = acc[i][j][r];
          const float ex = __builtin_amdgcn_exp2f((v - m_new) * kLog2eC);
          add += ex;
          // native RNE convert on gfx950
          const float vb = static_cast<float>(static_cast<bf16_t>(v));
          add_bf = fmaf(ex, vb - v, add_bf);
        }
        add = row16_sum(add);
        add_bf = row16_sum(add_bf);
        const float rescale = __builtin_amdgcn_exp2f((m4[r] - m_new) * kLog2eC);
        l4[r] = l4[r] * rescale + add;
        lb4[r] = lb4[r] * rescale + add_bf;
        m4[r] = m_new;
      }
      if ((lane & 15) == 0) {
        *reinterpret_cast<f32x4*>(st_p + i * 16) = m4;
        *reinterpret_cast<f32x4*>(st_p + 4 * kFwdTile + i * 16) = l4;
        *reinterpret_cast<f32x4*>(st_p + 8 * kFwdTile + i * 16) = lb4;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
    }
  };

  // (vocab tile, k-tile) of iterations it, it + 1 and it + 2
  int vt0 = vt_lo, kt0 = 0;
  int vt1 = vt0, kt1 = kt0;
  advance(vt1, kt1);
  int vt2 = vt1, kt2 = kt1;
  advance(vt2, kt2);

  // Prologue: issue order matches the steady-state boundary count.
#pragma unroll
  for (int ch = 0; ch < 4; ++ch) stage_b(0, vt0, kt0, ch);
  stage_a(0, kt0, 0); stage_a(0, kt0, 1);
  if (n_it > 1) {
#pragma unroll
    for (int ch = 0; ch < 4; ++ch) stage_b(1, vt1, kt1, ch);
  }

  for (int it = 0; it < n_it; ++it) {
    const char* a_base = smem + (size_t)(it & 1) * kFwdSlot;
    const char* b_base = a_base + 32 * 1024;

    // Boundary: this iteration's staging landed. In steady state the 4 newer
    // loads are B(it + 1); on the last iteration the newest outstanding loads
    // are this one's A halves, so drain fully.
    if (it + 1 < n_it) {
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();

    bf16x8 b_frag[4][2];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      bf16x8 a_frag[2][2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int kk = ks * 32 + (lane >> 4) * 8;
#pragma unroll
        for (int il = 0; il < 2; ++il) {
          const int row = wm * 128 + (2 * p + il) * 16 + (lane & 15);
          a_frag[il][ks] = lds_frag(a_base, row, kk, row);
        }
        if (p == 0) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            b_frag[j][ks] = Tile8BNK<256>::frag(b_base, kk, wn * 64 + j * 16, lane);
        }
      }
      // stage upcoming tiles into dead rows
      if (p == 0) {
        if (it + 1 < n_it) stage_a(it + 1, kt1, 0);
      } else if (p == 1) {
        if (it + 1 < n_it) stage_a(it + 1, kt1, 1);
        if (it + 2 < n_it) { stage_b(it + 2, vt2, kt2, 0); stage_b(it + 2, vt2, kt2, 1); }
      } else if (p == 2) {
        if (it + 2 < n_it) { stage_b(it + 2, vt2, kt2, 2); stage_b(it + 2, vt2, kt2, 3); }
      }
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int il = 0; il < 2; ++il)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            acc[2 * p + il][j] =
                mfma16(a_frag[il][ks], b_frag[j][ks], acc[2 * p + il][j]);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_s_barrier();
    }

    if (kt0 == n_ktiles - 1) epilogue(vt0);
    vt0 = vt1; kt0 = kt1;
    vt1 = vt2; kt1 = kt2;
    advance(vt2, kt2);
  }

  // The four column quarters of a row, merged in quarter order.
  __syncthreads();
  const int t = threadIdx.x;
  if (t < kFwdTile && row0 + t < T) {
    float m = st_m[t];
#pragma unroll
    for (int q = 1; q < 4; ++q) m = fmaxf(m, st_m[q * kFwdTile + t]);
    float l = 0.f, lb = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float w =
          __builtin_amdgcn_exp2f((st_m[q * kFwdTile + t] - m) * kLog2eC);
      l += st_l[q * kFwdTile + t] * w;
      lb += st_lb[q * kFwdTile + t] * w;
    }
    const size_t plane = (size_t)n_spans * T;
    float* out = ws + (size_t)span * T + row0 + t;
    out[0] = m;
    out[plane] = l;
    out[2 * plane] = lb;
    out[3 * plane] = tgt_lds[t];
  }
}

// lse, target logit and rounded lse of a row from its spans' partials, in
// span order.
__global__ __launch_bounds__(256) void cce_fwd_merge_kernel(
    const float* __restrict__ ws,    // (4, n_spans, T)
    float* __restrict__ lse_out,     // (T,)
    float* __restrict__ tgt_out,     // (T,) target logit, -1e30 without one
    float* __restrict__ lse_bf_out,  // (T,) lse of the bf16-ROUNDED logits
    int T, int n_spans) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= T) return;
  const size_t plane = (size_t)n_spans * T;
  float m = -1e30f;
  for (int s = 0; s < n_spans; ++s) m = fmaxf(m, ws[(size_t)s * T + row]);
  float l = 0.f, lb = 0.f, tg = -1e30f;
  for (int s = 0; s < n_spans; ++s) {
    const float* p = ws + (size_t)s * T + row;
    const float w = __builtin_amdgcn_exp2f((p[0] - m) * kLog2eC);
    l += p[plane] * w;
    lb += p[2 * plane] * w;
    tg = fmaxf(tg, p[3 * plane]);
  }
  lse_out[row] = m + __logf(fmaxf(l, 1e-30f));
  tgt_out[row] = tg;
  lse_bf_out[row] = m + __logf(fmaxf(l + lb, 1e-30f));
}

}  // namespace d9d

// n_spans: into how many spans of vocab tiles a row tile's sweep is cut (one
// block each); 0 chooses, and any value is capped at the number of tiles.
std::vector<torch::Tensor> cce_fwd(
    torch::Tensor e, torch::Tensor c, torch::Tensor targets, int64_t n_spans) {
  TORCH_CHECK(e.is_cuda() && e.scalar_type() == torch::kBFloat16 &&
              e.dim() == 2 && e.is_contiguous());
  TORCH_CHECK(c.is_cuda() && c.scalar_type() == torch::kBFloat16 &&
              c.dim() == 2 && c.is_contiguous());
  TORCH_CHECK(targets.is_cuda() && targets.scalar_type() == torch::kInt64);
  const int64_t T = e.size(0), K = e.size(1), V = c.size(0);
  TORCH_CHECK(c.size(1) == K, "cce_fwd: c must be (V, ", K, ")");
  TORCH_CHECK(targets.numel() == T, "cce_fwd: one target per row of e");
  TORCH_CHECK(K % 64 == 0 && K >= 64, "cce_fwd requires hidden % 64 == 0");
  TORCH_CHECK(V >= 1, "cce_fwd: empty classifier");
  TORCH_CHECK(n_spans >= 0, "cce_fwd: n_spans must be >= 0, got ", n_spans);
  TORCH_CHECK(T < (1 << 30) && V < (1 << 30), "cce_fwd: T or V too large");

  auto lse = torch::empty({T}, e.options().dtype(torch::kFloat32));
  auto tgt = torch::empty({T}, e.options().dtype(torch::kFloat32));
  auto lse_bf = torch::empty({T}, e.options().dtype(torch::kFloat32));
  if (T == 0) return {lse, tgt, lse_bf};

  const int64_t n_rt = (T + d9d::kFwdTile - 1) / d9d::kFwdTile;
  const int64_t n_vt = (V + d9d::kFwdTile - 1) / d9d::kFwdTile;
  // about four rounds of the 256 CUs (one block per CU)
  if (n_spans == 0) n_spans = std::max<int64_t>(1, 1024 / n_rt);
  n_spans = std::min(n_spans, n_vt);
  auto ws = torch::empty({4, n_spans, T}, e.options().dtype(torch::kFloat32));

  static const bool attr_set = [] {
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(&d9d::cce_fwd_tiled_kernel),
        hipFuncAttributeMaxDynamicSharedMemorySize, d9d::kFwdLds);
    return true;
  }();
  (void)attr_set;
  auto stream = at::hip::getCurrentHIPStream();
  auto tgts = targets.contiguous();
  hipLaunchKernelGGL(d9d::cce_fwd_tiled_kernel, dim3((unsigned)(n_rt * n_spans)),
                     dim3(512), d9d::kFwdLds, stream,
                     reinterpret_cast<const __bf16*>(e.data_ptr()),
                     reinterpret_cast<const __bf16*>(c.data_ptr()),
                     tgts.data_ptr<int64_t>(), ws.data_ptr<float>(), (int)T,
                     (int)V, (int)K, (int)n_rt, (int)n_spans);
  hipLaunchKernelGGL(d9d::cce_fwd_merge_kernel, dim3((unsigned)((T + 255) / 256)),
                     dim3(256), 0, stream, ws.data_ptr<float>(),
                     lse.data_ptr<float>(), tgt.data_ptr<float>(),
                     lse_bf.data_ptr<float>(), (int)T, (int)n_spans);
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
