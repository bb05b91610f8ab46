// CDNA4 (gfx950) flash attention: forward + backward, bf16, causal, GQA, LSE.
//
// Replaces the reference's external flash-attn wheels
// (d9d/kernel/flash_attn/function.py). MI355X-first design:
//   * MFMA v_mfma_f32_16x16x32_bf16 tiles, wave64.
//   * Forward: workgroup = 4 waves x 32 q-rows (two 16-row m-tiles per wave,
//     q block 128), KV tiles of 64 staged with the T14 issue-early/write-late
//     split — K row-major with an XOR swizzle (conflict-free ds_read_b128
//     fragments), V transposed with vectorized 8-byte LDS writes. It
//     computes the transposed products S^T = K Q^T and O^T = V^T P^T, so a
//     lane's values all belong to one q row: online softmax in fp32 per
//     lane, P stays in registers. s_setprio(1) around MFMA clusters; LSE
//     written for context-parallel merging.
//   * Backward: FA2 decomposition; workgroup = 8 waves owning a 128-row KV
//     tile, looping q tiles (Q/dO prefetched into registers under the MFMAs,
//     transposed images derived LDS-to-LDS); dK/dV accumulate in registers,
//     dQ via fp32 global atomics; delta = rowsum(dO*O) precomputed.
//
// Layouts: q (B,Sq,Hq,D), k/v (B,Skv,Hkv,D), out (B,Sq,Hq,D), lse (B,Hq,Sq).
// D (head_dim) templated in {32, 64, 96, 128}; host pads other sizes.
#include "common.h"
#include "mfma.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <type_traits>

namespace d9d {

constexpr int kFwdQ = 128;   // forward: q rows per workgroup (4 waves x 32)
constexpr int kFwdKv = 64;   // forward: kv rows per staged K/V tile
constexpr int kBwdQ = 64;    // backward: q rows per staged Q/dO tile
constexpr int kBwdKv = 128;  // backward: kv rows per workgroup (8 waves x 16)
constexpr int kBwdThreads = 512;
constexpr float kLog2e = 1.44269504088896340736f;

// XOR swizzles keep ds_read_b128 bank-conflict-free (guide G4). The XOR moves
// 16-byte units and must stay inside the LDS row: a mask of m bits needs rows
// that are a multiple of 16 << m bytes. Row-major [rows][D] tiles (D*2-byte
// rows) use swz_rm_mask<D>() -- D = 96 has 192-byte rows, a multiple of 64
// only, so it takes the 2-bit mask; transposed [D][ROWS] tiles use mask 7.
template <int D>
constexpr int swz_rm_mask() {
  constexpr int mask = D == 128 ? 15 : (D == 64 ? 7 : 3);
  static_assert((D * 2) % (16 * (mask + 1)) == 0, "swizzle leaves its LDS row");
  return mask;
}

// Address of element (row, col) in a swizzled row-major [rows][D] tile (Byte
// is char or const char). Row term and in-row term are added to the tile one
// after the other so a constant part of `row` folds into the LDS instruction.
template <int D, typename Byte>
D9D_DEVICE Byte* swz_rm_at(Byte* tile, int row, int col) {
  return tile + row * (D * 2) + ((col * 2) ^ ((row & swz_rm_mask<D>()) << 4));
}

// Address of element (d, r) in a swizzled transposed [D][ROWS] tile.
template <int ROWS, typename Byte>
D9D_DEVICE Byte* swz_t_at(Byte* tile, int d, int r) {
  static_assert((ROWS * 2) % (16 << 3) == 0, "swizzle leaves its LDS row");
  return tile + d * (ROWS * 2) + ((r * 2) ^ ((d & 7) << 4));
}

// Transpose a swizzled row-major [64][D] LDS image into a swizzled [D][64]
// LDS image using 4B LDS reads + 8B LDS writes.
template <int D, int BLOCK = 256>
D9D_DEVICE void transpose_lds_tile(bf16_t* dst, const bf16_t* src_rm, int tid) {
  // Work mapping: consecutive threads take consecutive ROW-quads of the
  // same d-pair, so the two b64 writes of a 16-thread group land on one
  // [d][64] row contiguously (128 B span, conflict-free). The b32 source
  // reads pay a 4-way conflict instead of the old mapping's 8-way b64
  // write conflict (rows 256 B apart XOR-spread only 4 ways per group).
  for (int idx = tid; idx < (64 / 4) * (D / 2); idx += BLOCK) {
    const int d0 = (idx / 16) * 2;
    const int rb = (idx % 16) * 4;
    bf16x4_bits c0, c1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t pair = *reinterpret_cast<const uint32_t*>(
          swz_rm_at<D>(reinterpret_cast<const char*>(src_rm), rb + i, d0));
      c0.s[i] = (ushort)(pair & 0xffffu);
      c1.s[i] = (ushort)(pair >> 16);
    }
    *reinterpret_cast<uint64_t*>(
        swz_t_at<64>(reinterpret_cast<char*>(dst), d0, rb)) = c0.u;
    *reinterpret_cast<uint64_t*>(
        swz_t_at<64>(reinterpret_cast<char*>(dst), d0 + 1, rb)) = c1.u;
  }
}

// Staging a (ROWS x D) global tile TRANSPOSED into a swizzled [D][ROWS] LDS
// image with 8B LDS writes; work item idx covers a (4 rows x 2 cols) block.
// The load half fills packed registers (rows row0.. of the sequence starting
// at row_lo, clamped to row_clamp), the store half writes them to LDS.
template <int D>
D9D_DEVICE void load_transposed_block(
    bf16x4_bits& c0, bf16x4_bits& c1, const bf16_t* src, int64_t row_stride,
    int row_lo, int row0, int row_clamp, int idx) {
  const int d0 = (idx % (D / 2)) * 2;
  const int rb = (idx / (D / 2)) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int g_row = row_lo + min(row0 + rb + i, row_clamp);
    const uint32_t pair = *reinterpret_cast<const uint32_t*>(
        src + (int64_t)g_row * row_stride + d0);
    c0.s[i] = (ushort)(pair & 0xffffu);
    c1.s[i] = (ushort)(pair >> 16);
  }
}

// Which kv row of a 64-row tile LDS row p of the forward's K tile holds. The
// forward feeds the C registers of S^T = K Q^T straight back as the B operand
// of O^T = V^T P^T: B slot (g, j) of PV k-step b (32 kv) is filled from C
// register j & 3 of lane group g of score tile 2b + (j >> 2), i.e. from K
// tile row p = 32b + 16(j >> 2) + 4g + (j & 3), and must carry
// kv = 32b + 8g + j, the kv that V^T presents there in its natural order.
// So row p = 32b + 16h + 4g + i is loaded with kv row 32b + 8g + 4h + i.
constexpr int pv_pos(int p) {
  return (p & ~31) | ((p & 12) << 1) | ((p & 16) >> 2) | (p & 3);
}

constexpr bool pv_pos_is_unit_permutation() {
  bool seen[64] = {};
  for (int p = 0; p < 64; ++p) {
    const int kv = pv_pos(p);
    if (kv < 0 || kv >= 64 || seen[kv]) return false;
    seen[kv] = true;
    // aligned 4-row groups map to aligned 4-row groups, in order
    if (kv != pv_pos(p & ~3) + (p & 3) || pv_pos(p & ~3) % 4 != 0) return false;
    // B slot (g, j) of k-step b, packed from row p's C register, carries kv
    const int b = kv >> 5, g = (kv >> 3) & 3, j = kv & 7;
    if (p != 32 * b + 16 * (j >> 2) + 4 * g + (j & 3)) return false;
  }
  return true;
}
static_assert(pv_pos_is_unit_permutation(),
              "pv_pos must permute 0..63 in aligned 4-row units");

template <int D, int ROWS>
D9D_DEVICE void store_transposed_block(
    bf16_t* dst, const bf16x4_bits& c0, const bf16x4_bits& c1, int idx) {
  const int d0 = (idx % (D / 2)) * 2;
  const int rb = (idx / (D / 2)) * 4;
  *reinterpret_cast<uint64_t*>(
      swz_t_at<ROWS>(reinterpret_cast<char*>(dst), d0, rb)) = c0.u;
  *reinterpret_cast<uint64_t*>(
      swz_t_at<ROWS>(reinterpret_cast<char*>(dst), d0 + 1, rb)) = c1.u;
}

template <int D, int ROWS, int BLOCK>
D9D_DEVICE void stage_transposed_tile(
    bf16_t* dst, const bf16_t* src, int64_t row_stride,
    int row_lo, int row0, int row_clamp, int tid) {
  for (int idx = tid; idx < (ROWS / 4) * (D / 2); idx += BLOCK) {
    bf16x4_bits c0, c1;
    load_transposed_block<D>(c0, c1, src, row_stride, row_lo, row0, row_clamp, idx);
    store_transposed_block<D, ROWS>(dst, c0, c1, idx);
  }
}

// ---- tile location and masking -------------------------------------------------

// Which (batch, head, tile) a workgroup owns, and its sequence's row ranges.
struct TileLoc {
  int b, h, tile;
  int q_lo, Sq_loc, kv_lo, Skv_loc;  // sequence start and length, q and kv
  int causal_off;  // kv position aligned with q row 0
  bool valid;      // the tile starts inside the tiled extent
};

// The grid tiles q (forward, TILE_KV = false) or kv (backward) in TILE rows.
// Varlen (packed sequences): grid = (per-sequence tiles, heads); binary search
// the tile prefix for our sequence, then work in LOCAL coordinates. Causal
// masking aligns the END of q with the END of kv (flash-attn convention).
// Otherwise grid = (tiles, B * Hq), regrouped so that one (b, h)'s tiles,
// which share that head's streamed operands, run on one XCD.
template <int TILE, bool TILE_KV>
D9D_DEVICE TileLoc locate_tile(
    const int* __restrict__ cu_q, const int* __restrict__ cu_k,
    const int* __restrict__ tile_pref, int nseq,
    int Sq, int Skv, int Hq, int q_offset) {
  TileLoc t;
  if (cu_q != nullptr) {
    t.h = blockIdx.y;
    int lo = 0, hi = nseq - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (tile_pref[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    t.b = 0;
    t.tile = blockIdx.x - tile_pref[lo];
    t.q_lo = cu_q[lo];
    t.Sq_loc = cu_q[lo + 1] - t.q_lo;
    t.kv_lo = cu_k[lo];
    t.Skv_loc = cu_k[lo + 1] - t.kv_lo;
    t.causal_off = t.Skv_loc - t.Sq_loc + q_offset;
    t.valid = t.tile * TILE < (TILE_KV ? t.Skv_loc : t.Sq_loc);
  } else {
    const int wid = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x,
                              gridDim.x * gridDim.y);
    const int bh = wid / gridDim.x;
    t.b = bh / Hq;
    t.h = bh % Hq;
    // Heavy first: a causal q-tile's work grows with its index (the forward)
    // and shrinks with its kv-tile's (the backward), so the forward walks
    // its tiles backwards and no XCD ends on a head's longest tiles.
    t.tile = TILE_KV ? wid % gridDim.x : gridDim.x - 1 - wid % gridDim.x;
    t.q_lo = 0; t.Sq_loc = Sq; t.kv_lo = 0; t.Skv_loc = Skv;
    t.causal_off = q_offset;
    t.valid = true;
  }
  return t;
}

// Extends the caller's bounds mask by the causal / sliding-window part; q_pos
// is the q row's ALIGNED position (row + causal_off) on the kv axis.
D9D_DEVICE bool causal_window_masked(bool masked, int q_pos, int kv_pos,
                                     int causal, int window_left) {
  if (causal) masked |= kv_pos > q_pos;
  if (window_left >= 0) masked |= kv_pos < q_pos - window_left;
  return masked;
}

// ---------------------------------------------------------------------------
// Forward
// ---------------------------------------------------------------------------

template <int D>
__global__ __launch_bounds__(256, 2) void flash_fwd_kernel(
    const bf16_t* __restrict__ q,   // (B,Sq,Hq,D)
    const bf16_t* __restrict__ k,   // (B,Skv,Hkv,D)
    const bf16_t* __restrict__ v,   // (B,Skv,Hkv,D)
    bf16_t* __restrict__ out,       // (B,Sq,Hq,D)
    float* __restrict__ lse,        // (B,Hq,Sq)
    const float* __restrict__ sinks,  // (Hq,) raw sink logits, or nullptr
    const int* __restrict__ cu_q,     // (nseq+1,) packed-seq bounds, or nullptr
    const int* __restrict__ cu_k,
    const int* __restrict__ qtile_pref,  // (nseq+1,) prefix of ceil(len_q/kFwdQ)
    int nseq,
    int B, int Sq, int Skv, int Hq, int Hkv,
    float scale, int causal, int window_left, int q_offset) {
  constexpr int kNT = D / 16;   // n-tiles over head dim
  constexpr int kKS = D / 32;   // k-steps over head dim

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // [kFwdKv][D] swizzled, row p = kv row pv_pos(p); fwd_smem_bytes() is this
  // carve-up
  bf16_t* k_lds = reinterpret_cast<bf16_t*>(smem);
  bf16_t* vt_lds = k_lds + kFwdKv * D;               // [D][kFwdKv] transposed

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lrow = lane & 15;  // the q row (of a 16-row sub-tile) this lane owns
  const int lgrp = lane >> 4;
  const bool upper = lane >= 32;

  // one (b, h)'s q-tiles share its KV stream (XCD grouping)
  const TileLoc loc = locate_tile<kFwdQ, false>(
      cu_q, cu_k, qtile_pref, nseq, Sq, Skv, Hq, q_offset);
  if (!loc.valid) return;
  const int b = loc.b, h = loc.h, q_tile = loc.tile, causal_off = loc.causal_off;
  const int q_lo = loc.q_lo, Sq_loc = loc.Sq_loc, kv_lo = loc.kv_lo, Skv_loc = loc.Skv_loc;
  const int hkv = h / (Hq / Hkv);

  const int64_t q_base = ((int64_t)b * Sq * Hq + h) * D;
  const int64_t kv_base = ((int64_t)b * Skv * Hkv + hkv) * D;
  const int64_t q_row_stride = (int64_t)Hq * D;
  const int64_t kv_row_stride = (int64_t)Hkv * D;

  // ---- load this wave's 32 q rows (2 sub-tiles) into fragments -------------
  // The kernel computes the TRANSPOSED products S^T = K Q^T and
  // O^T = V^T P^T: Q is the B operand, and in the C layout of S^T and O^T
  // every value a lane holds belongs to ONE q row (lane & 15). The row
  // statistics are then per lane, and the S^T registers are already a legal
  // B operand for PV (see pv_pos): P never leaves the registers.
  bf16x8 q_frag[2][kKS];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int q_row_local = q_tile * kFwdQ + wave * 32 + m * 16 + lrow;
    const int safe_row = q_lo + min(q_row_local, Sq_loc - 1);
    const bf16_t* qp = q + q_base + (int64_t)safe_row * q_row_stride;
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      q_frag[m][ks] = *reinterpret_cast<const bf16x8*>(qp + ks * 32 + lgrp * 8);
    }
  }

  // A learnable "sink" is one virtual softmax column per head with logit
  // sinks[h] and no value row: seed the running max/sum with it and the
  // online softmax (and the LSE the backward reads) absorbs it for free.
  const float m_init = sinks ? sinks[h] : -1e30f;
  // l is kept as partial sums per kv column class (see the loop), merged at
  // the epilogue: seed the sink's column on class 0 only
  const float l_init = (sinks && lgrp == 0) ? 1.f : 0.f;
  float m_run[2], l_run[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    m_run[m] = m_init;
#pragma unroll
    for (int r = 0; r < 4; ++r) l_run[m][r] = r == 0 ? l_init : 0.f;
  }
  f32x4 o_acc[2][kNT];  // O^T: lane holds O[q = lrow][d = nt*16 + lgrp*4 + r]
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt) o_acc[m][nt] = {0.f, 0.f, 0.f, 0.f};

  const int q_tile_last_row = min(q_tile * kFwdQ + kFwdQ - 1, Sq_loc - 1);
  int kv_end = Skv_loc;
  if (causal) kv_end = min(Skv_loc, q_tile_last_row + causal_off + 1);
  const int num_kv_tiles = (kv_end + kFwdKv - 1) / kFwdKv;
  if (num_kv_tiles <= 0) return;

  // T14 split staging: next tile's K rows and V (4x2 transpose blocks) are
  // loaded into registers while the current tile's MFMAs run; LDS writes and
  // their vmcnt waits land after the compute barrier.
  constexpr int kKIters = (kFwdKv * D) / (256 * 8);
  constexpr int kVIters = (kFwdKv / 4) * (D / 2) / 256;
  bf16x8 k_reg[kKIters];
  bf16x4_bits v_c0[kVIters], v_c1[kVIters];

  auto load_regs = [&](int kt) {
    const int kv0 = kt * kFwdKv;
#pragma unroll
    for (int it = 0; it < kKIters; ++it) {
      const int idx = (threadIdx.x + it * 256) * 8;
      const int row = idx / D;
      const int col = idx % D;
      const int g_row = kv_lo + min(kv0 + pv_pos(row), Skv_loc - 1);
      k_reg[it] = *reinterpret_cast<const bf16x8*>(
          k + kv_base + (int64_t)g_row * kv_row_stride + col);
    }
#pragma unroll
    for (int it = 0; it < kVIters; ++it) {
      load_transposed_block<D>(v_c0[it], v_c1[it], v + kv_base, kv_row_stride,
                               kv_lo, kv0, Skv_loc - 1, threadIdx.x + it * 256);
    }
  };

  auto store_lds = [&]() {
#pragma unroll
    for (int it = 0; it < kKIters; ++it) {
      const int idx = (threadIdx.x + it * 256) * 8;
      *reinterpret_cast<bf16x8*>(
          swz_rm_at<D>(reinterpret_cast<char*>(k_lds), idx / D, idx % D)) =
          k_reg[it];
    }
#pragma unroll
    for (int it = 0; it < kVIters; ++it) {
      store_transposed_block<D, kFwdKv>(vt_lds, v_c0[it], v_c1[it],
                                        threadIdx.x + it * 256);
    }
  };

  load_regs(0);
  store_lds();
  __syncthreads();

  for (int kt = 0; kt < num_kv_tiles; ++kt) {
    const int kv0 = kt * kFwdKv;
    if (kt + 1 < num_kv_tiles) load_regs(kt + 1);  // issue early

    // ---- S^T = K Q^T for both q sub-tiles; each K fragment is read once ----
    // lane holds S[q = lrow][kv = kv0 + pv_pos(nt*16 + lgrp*4 + r)] in
    // st[m][nt][r]
    f32x4 st[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) st[m][nt] = {0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int kv_row = nt * 16 + lrow;
#pragma unroll
      for (int ks = 0; ks < kKS; ++ks) {
        const int d0 = ks * 32 + lgrp * 8;
        const bf16x8 ka = *reinterpret_cast<const bf16x8*>(
            swz_rm_at<D>(reinterpret_cast<char*>(k_lds), kv_row, d0));
#pragma unroll
        for (int m = 0; m < 2; ++m) st[m][nt] = mfma16(ka, q_frag[m][ks], st[m][nt]);
      }
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- per-lane online softmax; P^T packed as PV's B operand -------------
    bf16x8 pb[2][2];  // [m][ks2]
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int my_q_row = q_tile * kFwdQ + wave * 32 + m * 16;
      // Tile-level mask skip: most KV tiles sit fully below the causal
      // diagonal and inside the window for every row of this sub-tile -- the
      // per-element mask chain (3 compares + select x16) only runs on the
      // diagonal/edge tiles (wave-uniform branch).
      const int row_lo = my_q_row + causal_off;
      const bool any_mask =
          (kv0 + kFwdKv > kv_end) ||
          (causal && kv0 + kFwdKv - 1 > row_lo) ||
          (window_left >= 0 && kv0 < row_lo + 15 - window_left);
      if (any_mask) {
        const int row = row_lo + lrow;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int col = kv0 + pv_pos(nt * 16 + lgrp * 4 + r);
            const bool masked = causal_window_masked(
                col >= kv_end, row, col, causal, window_left);
            st[m][nt][r] = masked ? -1e30f : st[m][nt][r] * scale;
          }
        }
      } else {
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) st[m][nt][r] = st[m][nt][r] * scale;
      }
      // row max: 16 values in the lane, then the row's 3 other lanes
      float mx = st[m][0][0];
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[m][nt][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      const float m_new = fmaxf(m_run[m], mx);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          st[m][nt][r] = __builtin_amdgcn_exp2f((st[m][nt][r] - m_new) * kLog2e);
      // l accumulates per kv column class c = kv & 15, its 4 columns of the
      // tile added in kv order: the partial sums of the S = Q K^T layout,
      // where a lane owned one column of each 16-wide tile, so l (and with
      // it out and lse) keeps its bits. Column c + 16 n sits on lane group
      // (c >> 3) + 2 (n & 1) in st[2 (n >> 1) + ((c >> 2) & 1)][c & 3]: the
      // lower lane of a pair (lane ^ 32) sums the classes with c & 4 == 0,
      // the upper one the others, after one exchange of the halves.
      float l_add[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float give0 = upper ? st[m][0][r] : st[m][1][r];
        const float give1 = upper ? st[m][2][r] : st[m][3][r];
        const float got0 = __shfl_xor(give0, 32, 64);
        const float got1 = __shfl_xor(give1, 32, 64);
        const float own0 = upper ? st[m][1][r] : st[m][0][r];
        const float a2 = upper ? got1 : st[m][2][r];
        const float a3 = upper ? st[m][3][r] : got1;
        l_add[r] = ((own0 + got0) + a2) + a3;  // n = 0 + 1 commutes
      }
      // Lazy rescale: after the first few KV tiles the running max rarely
      // moves, so alpha == 1 for every row of the wave most of the time --
      // skip the exp2 and the kNT*4 accumulator multiplies (wave-uniform
      // branch).
      if (__all(m_new == m_run[m])) {
#pragma unroll
        for (int r = 0; r < 4; ++r) l_run[m][r] += l_add[r];
      } else {
        const float alpha = __builtin_amdgcn_exp2f((m_run[m] - m_new) * kLog2e);
#pragma unroll
        for (int r = 0; r < 4; ++r) l_run[m][r] = l_run[m][r] * alpha + l_add[r];
        m_run[m] = m_new;
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) o_acc[m][nt][r] *= alpha;
      }
      // B slot (lgrp, j) of PV k-step ks2 takes kv = 32 ks2 + 8 lgrp + j: the
      // registers of st[2 ks2] then st[2 ks2 + 1] (see pv_pos)
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          pb[m][ks2][j] = (bf16_t)st[m][2 * ks2][j];
          pb[m][ks2][4 + j] = (bf16_t)st[m][2 * ks2 + 1][j];
        }
    }

    // ---- O^T += V^T P^T; each V^T fragment is read once for both sub-tiles --
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks2 = 0; ks2 < 2; ++ks2) {
      const int kv_off = ks2 * 32 + lgrp * 8;
#pragma unroll
      for (int nt = 0; nt < kNT; ++nt) {
        const int d = nt * 16 + lrow;
        const bf16x8 va = *reinterpret_cast<const bf16x8*>(
            swz_t_at<kFwdKv>(reinterpret_cast<char*>(vt_lds), d, kv_off));
#pragma unroll
        for (int m = 0; m < 2; ++m) o_acc[m][nt] = mfma16(va, pb[m][ks2], o_acc[m][nt]);
      }
    }
    __builtin_amdgcn_s_setprio(0);

    __syncthreads();
    if (kt + 1 < num_kv_tiles) {
      store_lds();
      __syncthreads();
    }
  }

  // ---- epilogue: merge the per-lane l across each row's 4 lanes (once),
  // then O /= l; stage in LDS; coalesced 16B stores; LSE --------------------
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    // butterfly over the 16 column classes in the order c ^ 1, 2, 4, 8
    l_run[m][0] = (l_run[m][0] + l_run[m][1]) + (l_run[m][2] + l_run[m][3]);
    l_run[m][0] += __shfl_xor(l_run[m][0], 32, 64);
    l_run[m][0] += __shfl_xor(l_run[m][0], 16, 64);
  }
  {
    // reuse: swizzled [64][D], staged twice (two 64-row halves)
    char* o_lds = reinterpret_cast<char*>(k_lds);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      __syncthreads();
      // waves 0,1 hold q rows 0..63 of the tile; waves 2,3 rows 64..127
      if ((wave >> 1) == half) {
#pragma unroll
        for (int m = 0; m < 2; ++m) {
          const float inv_l = (l_run[m][0] > 0.f) ? 1.f / l_run[m][0] : 0.f;
          const int row = (wave & 1) * 32 + m * 16 + lrow;
#pragma unroll
          for (int nt = 0; nt < kNT; ++nt) {
            bf16x4_bits o4;  // 4 consecutive d of one row
#pragma unroll
            for (int r = 0; r < 4; ++r)
              o4.s[r] = bf16_bits((bf16_t)(o_acc[m][nt][r] * inv_l));
            *reinterpret_cast<uint64_t*>(
                swz_rm_at<D>(o_lds, row, nt * 16 + lgrp * 4)) = o4.u;
          }
        }
      }
      __syncthreads();
      constexpr int elems = 64 * D;
      for (int idx = threadIdx.x * 8; idx < elems; idx += 256 * 8) {
        const int row = idx / D;
        const int col = idx % D;
        const int rg = q_tile * kFwdQ + half * 64 + row;
        if (rg < Sq_loc) {
          *reinterpret_cast<bf16x8*>(
              out + q_base + (int64_t)(q_lo + rg) * q_row_stride + col) =
              *reinterpret_cast<const bf16x8*>(swz_rm_at<D>(o_lds, row, col));
        }
      }
    }
    if (lgrp == 0) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const int rg = q_tile * kFwdQ + wave * 32 + m * 16 + lrow;
        if (rg < Sq_loc) {
          // regular: (B,Hq,Sq); varlen: (Hq,total) with b == 0
          lse[((int64_t)b * Hq + h) * Sq + q_lo + rg] =
              m_run[m] + __logf(fmaxf(l_run[m][0], 1e-30f));
        }
      }
    }
  }
}

// K tile + V^T tile (the kernel's LDS carve-up).
template <int D>
constexpr size_t fwd_smem_bytes() {
  return sizeof(bf16_t) * (kFwdKv * D + D * kFwdKv);
}

// ---------------------------------------------------------------------------
// Backward
// ---------------------------------------------------------------------------

// delta[b,h,q] = sum_d dO * O  (fp32)
__global__ void attn_delta_kernel(
    const bf16_t* __restrict__ dout,  // (B,Sq,Hq,D)
    const bf16_t* __restrict__ out,
    float* __restrict__ delta,        // (B,Hq,Sq)
    int B, int Sq, int Hq, int D) {
  const int64_t row = blockIdx.x;  // over B*Sq*Hq
  if (row >= (int64_t)B * Sq * Hq) return;
  const int h = row % Hq;
  const int s = (row / Hq) % Sq;
  const int b = row / ((int64_t)Hq * Sq);
  const bf16_t* dp = dout + row * D;
  const bf16_t* op = out + row * D;
  float acc = 0.f;
  for (int i = threadIdx.x; i < D; i += 64) {
    acc += (float)dp[i] * (float)op[i];
  }
  acc = wave_reduce_sum(acc);
  if (threadIdx.x == 0) {
    delta[((int64_t)b * Hq + h) * Sq + s] = acc;
  }
}

// P / dS images: kBwdKv / 16 blocks of 128 B per 4-q row, stride padded +32 B.
constexpr int kBwdXStride = (kBwdKv / 16) * 128 + 32;

// Q, dO, dO^T, Q^T tiles + K^T + the P and dS images.
template <int D>
constexpr size_t bwd_smem_bytes() {
  return sizeof(bf16_t) * (4 * kBwdQ * D + D * kBwdKv) + 2 * (kBwdQ / 4) * kBwdXStride;
}

template <int D>
__global__ __launch_bounds__(512, 1) void flash_bwd_kernel(
    const bf16_t* __restrict__ q,
    const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ dout,
    const float* __restrict__ lse,    // (B,Hq,Sq)
    const float* __restrict__ delta,  // (B,Hq,Sq)
    float* __restrict__ dq,           // (B,Sq,Hq,D) fp32 accum
    float* __restrict__ dk,           // (B,Skv,Hkv,D) fp32 accum
    float* __restrict__ dv,           // (B,Skv,Hkv,D) fp32 accum
    const int* __restrict__ cu_q,     // packed-seq bounds, or nullptr
    const int* __restrict__ cu_k,
    const int* __restrict__ kvtile_pref,  // prefix of ceil(len_k/kBwdKv)
    int nseq,
    int B, int Sq, int Skv, int Hq, int Hkv,
    float scale, int causal, int window_left, int q_offset) {
  constexpr int kNT = D / 16;
  constexpr int kKS = D / 32;
  static_assert(kNT >= 2 && kNT % 2 == 0, "dQ splits the head dim in halves");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // Separate buffers for every staged operand: the three MFMA phases
  // (dV, dK, dQ) then run back-to-back with NO barrier between them, and the
  // whole q-tile iteration needs 4 __syncthreads instead of 8 (PMC showed
  // ~50% of bwd wave cycles parked on barriers with the shared-buffer
  // schedule). 149 KB LDS at D=128 -- one workgroup per CU, which this
  // kernel is at anyway.
  // bwd_smem_bytes() is this carve-up.
  bf16_t* q_lds = reinterpret_cast<bf16_t*>(smem);   // [64][D] swizzled rows
  bf16_t* do_lds = q_lds + kBwdQ * D;                // [64][D]
  bf16_t* tdo_lds = do_lds + kBwdQ * D;              // [D][64]: dO^T
  bf16_t* tq_lds = tdo_lds + D * kBwdQ;              // [D][64]: Q^T
  bf16_t* kt_lds = tq_lds + D * kBwdQ;               // [D][kBwdKv]
  // P and dS live in ONE q-major blocked image each: [4 q][16 kv] 128-B
  // tr16 blocks at (q>>2, kv>>4), qb stride padded +32 B so the packed
  // b64 stores of 4 kv values per (q, nt) are bank-spread. dV/dK read
  // their kv-major A fragments via ds_read_b64_tr_b16 pairs; dQ reads its
  // q-major fragments as plain 16-B rows of the SAME dS image — the old
  // third (q-major) copy and 48 scalar stores per wave are gone.
  constexpr int kXqStride = kBwdXStride;             // bytes per q-block row
  char* x1_lds = reinterpret_cast<char*>(kt_lds + D * kBwdKv);  // P image
  char* x2_lds = x1_lds + (kBwdQ / 4) * kXqStride;              // dS image

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;   // 8 waves x 16 kv rows = 128 kv/block

  // one (b, h)'s kv-tiles share its Q/dO/lse streams (XCD grouping)
  const TileLoc loc = locate_tile<kBwdKv, true>(
      cu_q, cu_k, kvtile_pref, nseq, Sq, Skv, Hq, q_offset);
  if (!loc.valid || loc.Sq_loc <= 0) return;
  const int b = loc.b, h = loc.h, kv_tile = loc.tile, causal_off = loc.causal_off;
  const int q_lo = loc.q_lo, Sq_loc = loc.Sq_loc, kv_lo = loc.kv_lo, Skv_loc = loc.Skv_loc;
  const int hkv = h / (Hq / Hkv);

  const int64_t q_base = ((int64_t)b * Sq * Hq + h) * D;
  const int64_t kv_base = ((int64_t)b * Skv * Hkv + hkv) * D;
  const int64_t q_row_stride = (int64_t)Hq * D;
  const int64_t kv_row_stride = (int64_t)Hkv * D;
  const float* lse_row = lse + ((int64_t)b * Hq + h) * Sq + q_lo;
  const float* delta_row = delta + ((int64_t)b * Hq + h) * Sq + q_lo;

  const int kv0 = kv_tile * kBwdKv;

  // This wave's 16 kv rows: K and V A-fragments in registers.
  const int kv_row_local = lane & 15;
  const int kv_row_global =
      kv_lo + min(kv0 + wave * 16 + kv_row_local, Skv_loc - 1);
  bf16x8 k_frag[kKS], v_frag[kKS];
  {
    const bf16_t* kp = k + kv_base + (int64_t)kv_row_global * kv_row_stride;
    const bf16_t* vp = v + kv_base + (int64_t)kv_row_global * kv_row_stride;
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      const int d0 = ks * 32 + (lane >> 4) * 8;
      k_frag[ks] = *reinterpret_cast<const bf16x8*>(kp + d0);
      v_frag[ks] = *reinterpret_cast<const bf16x8*>(vp + d0);
    }
  }

  // Stage K^T once (for dQ's B fragments).
  stage_transposed_tile<D, kBwdKv, kBwdThreads>(
      kt_lds, k + kv_base, kv_row_stride, kv_lo, kv0, Skv_loc - 1, threadIdx.x);

  f32x4 dk_acc[kNT], dv_acc[kNT];
#pragma unroll
  for (int nt = 0; nt < kNT; ++nt) {
    dk_acc[nt] = {0.f, 0.f, 0.f, 0.f};
    dv_acc[nt] = {0.f, 0.f, 0.f, 0.f};
  }

  int q_start = 0;
  if (causal) {
    // first q tile whose last aligned position reaches kv0
    q_start = (max(kv0 - causal_off, 0) / kBwdQ) * kBwdQ;
  }
  if (q_start >= Sq_loc) return;

  // T14: each q-tile's Q/dO rows are prefetched into registers while the
  // previous tile's MFMAs run; the transposed images are derived from the
  // row-major LDS copies (cheap ds_reads) instead of re-reading global.
  constexpr int kQdoRegs =
      (kBwdQ * D + kBwdThreads * 8 - 1) / (kBwdThreads * 8);  // >= 1 (D <= 128)
  bf16x8 q_reg[kQdoRegs], do_reg[kQdoRegs];

  auto load_qdo_regs = [&](int qt_next) {
#pragma unroll
    for (int it = 0; it < kQdoRegs; ++it) {
      const int idx = (threadIdx.x + it * kBwdThreads) * 8;
      if (idx >= kBwdQ * D) break;
      const int row = idx / D;
      const int col = idx % D;
      const int g_row = q_lo + min(qt_next + row, Sq_loc - 1);
      q_reg[it] = *reinterpret_cast<const bf16x8*>(
          q + q_base + (int64_t)g_row * q_row_stride + col);
      do_reg[it] = *reinterpret_cast<const bf16x8*>(
          dout + q_base + (int64_t)g_row * q_row_stride + col);
    }
  };
  auto store_qdo_lds = [&]() {
#pragma unroll
    for (int it = 0; it < kQdoRegs; ++it) {
      const int idx = (threadIdx.x + it * kBwdThreads) * 8;
      if (idx >= kBwdQ * D) break;
      const int row = idx / D;
      const int col = idx % D;
      *reinterpret_cast<bf16x8*>(
          swz_rm_at<D>(reinterpret_cast<char*>(q_lds), row, col)) = q_reg[it];
      *reinterpret_cast<bf16x8*>(
          swz_rm_at<D>(reinterpret_cast<char*>(do_lds), row, col)) = do_reg[it];
    }
  };

  load_qdo_regs(q_start);
  store_qdo_lds();
  __syncthreads();

  for (int qt = q_start; qt < Sq_loc; qt += kBwdQ) {
    if (qt + kBwdQ < Sq_loc) load_qdo_regs(qt + kBwdQ);  // issue early
    // dO^T and Q^T images for the dV/dK B fragments (cheap LDS-to-LDS).
    // NO barrier here: tdo/tq are first read after the x-stage barrier
    // below, which also publishes these writes (2 barriers per q-tile
    // instead of 4 — the PMC wave-parked share was the top bwd cost).
    transpose_lds_tile<D, kBwdThreads>(tdo_lds, do_lds, threadIdx.x);
    transpose_lds_tile<D, kBwdThreads>(tq_lds, q_lds, threadIdx.x);

    // ---- S^T = K @ Q^T (per wave: 16 kv x 64 q) ----------------------------
    f32x4 st_acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) st_acc[nt] = {0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int q_row = nt * 16 + (lane & 15);
#pragma unroll
      for (int ks = 0; ks < kKS; ++ks) {
        const int d0 = ks * 32 + (lane >> 4) * 8;
        const bf16x8 qb = *reinterpret_cast<const bf16x8*>(
            swz_rm_at<D>(reinterpret_cast<char*>(q_lds), q_row, d0));
        st_acc[nt] = mfma16(k_frag[ks], qb, st_acc[nt]);
      }
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- P^T = exp(S^T * scale - lse[q]); masked entries 0 -----------------
    // Tile-level mask skip (see fwd): interior tiles take the select-free
    // path, only diagonal/edge tiles run the per-element mask chain.
    const bool any_mask =
        (kv0 + kBwdKv > Skv_loc) || (qt + kBwdQ > Sq_loc) ||
        (causal && kv0 + kBwdKv - 1 > qt + causal_off) ||
        (window_left >= 0 &&
         kv0 < qt + kBwdQ - 1 + causal_off - window_left);
    float pt_val[4][4];  // [nt][r]
    if (any_mask) {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int q_glob = qt + nt * 16 + (lane & 15);
        const float l = (q_glob < Sq_loc) ? lse_row[min(q_glob, Sq_loc - 1)] : 1e30f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kv_glob = kv0 + wave * 16 + (lane >> 4) * 4 + r;
          float s = st_acc[nt][r] * scale;
          const bool masked = causal_window_masked(
              (kv_glob >= Skv_loc) || (q_glob >= Sq_loc), q_glob + causal_off,
              kv_glob, causal, window_left);
          pt_val[nt][r] =
              masked ? 0.f : __builtin_amdgcn_exp2f((s - l) * kLog2e);
        }
      }
    } else {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        // clamp even on the fast path: the compiler may speculate this load
        // across the branch, and edge tiles would read past the lse buffer
        const float l = lse_row[min(qt + nt * 16 + (lane & 15), Sq_loc - 1)];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          pt_val[nt][r] =
              __builtin_amdgcn_exp2f((st_acc[nt][r] * scale - l) * kLog2e);
        }
      }
    }

    // ---- dP^T = V @ dO^T ---------------------------------------------------
    f32x4 dpt_acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) dpt_acc[nt] = {0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int q_row = nt * 16 + (lane & 15);
#pragma unroll
      for (int ks = 0; ks < kKS; ++ks) {
        const int d0 = ks * 32 + (lane >> 4) * 8;
        const bf16x8 db = *reinterpret_cast<const bf16x8*>(
            swz_rm_at<D>(reinterpret_cast<char*>(do_lds), q_row, d0));
        dpt_acc[nt] = mfma16(v_frag[ks], db, dpt_acc[nt]);
      }
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- dS^T = P^T * (dP^T - delta[q]) * scale ---------------------------
    float dst_val[4][4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int q_glob = qt + nt * 16 + (lane & 15);
      const float dlt = (q_glob < Sq_loc) ? delta_row[min(q_glob, Sq_loc - 1)] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        dst_val[nt][r] = pt_val[nt][r] * (dpt_acc[nt][r] - dlt) * scale;
      }
    }

    // ---- stage P and dS into the blocked images, ONE barrier --------------
    // value (q, kv) at qb = q>>2 row, block kv>>4, inner (q&3)*32 + (kv&15)*2;
    // the 4 r-values (4 consecutive kv at fixed q) pack into one b64 store.
    {
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int q_l = nt * 16 + (lane & 15);
        const int kv_l = wave * 16 + (lane >> 4) * 4;
        const size_t byte = (size_t)(q_l >> 2) * kXqStride +
                            (kv_l >> 4) * 128 + (q_l & 3) * 32 +
                            (kv_l & 15) * 2;
        bf16x4_bits p4, d4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p4.s[r] = bf16_bits((bf16_t)pt_val[nt][r]);
          d4.s[r] = bf16_bits((bf16_t)dst_val[nt][r]);
        }
        *reinterpret_cast<uint64_t*>(x1_lds + byte) = p4.u;
        *reinterpret_cast<uint64_t*>(x2_lds + byte) = d4.u;
      }
      __syncthreads();
    }

    // ---- dV += P^T @ dO; dK += dS^T @ Q: back-to-back, no barrier ----------
    {
      // A fragment (m = kv row wave*16 + lane&15, k = 8 q at q_off) = two
      // ds_read_b64_tr_b16 of the [4 q][16 kv] blocks (qb, wave)
      auto xfrag = [&](const char* img, int q_off) -> bf16x8 {
        const size_t b0 = (size_t)(q_off >> 2) * kXqStride + wave * 128 +
                          (lane & 15) * 8;
        bf16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (__attribute__((address_space(3))) bf16x4*)(img + b0));
        bf16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (__attribute__((address_space(3))) bf16x4*)(img + b0 + kXqStride));
        bf16x8 f;
#pragma unroll
        for (int t2 = 0; t2 < 4; ++t2) { f[t2] = lo4[t2]; f[4 + t2] = hi4[t2]; }
        return f;
      };
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks2 = 0; ks2 < 2; ++ks2) {
        const int q_off = ks2 * 32 + (lane >> 4) * 8;
        const bf16x8 pa = xfrag(x1_lds, q_off);
        const bf16x8 da = xfrag(x2_lds, q_off);
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt) {
          const int d = nt * 16 + (lane & 15);
          const bf16x8 dob = *reinterpret_cast<const bf16x8*>(
              swz_t_at<kBwdQ>(reinterpret_cast<char*>(tdo_lds), d, q_off));
          const bf16x8 qb = *reinterpret_cast<const bf16x8*>(
              swz_t_at<kBwdQ>(reinterpret_cast<char*>(tq_lds), d, q_off));
          dv_acc[nt] = mfma16(pa, dob, dv_acc[nt]);
          dk_acc[nt] = mfma16(da, qb, dk_acc[nt]);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }

    // ---- dQ partial = dS @ K; atomicAdd (A = dS q-major via x3) -----------
    {
      // ALL 8 waves: wave & 3 picks the 16-row q m-tile, wave >> 2 the
      // d-half -- the old waves-0-3-only split parked half the block
      // through an entire MFMA phase.
      constexpr int kNTH = kNT / 2;  // nt per d-half
      const int q_mt = wave & 3;
      const int nt0 = (wave >> 2) * kNTH;
      f32x4 dq_acc[kNTH];
#pragma unroll
      for (int nt = 0; nt < kNTH; ++nt) dq_acc[nt] = {0.f, 0.f, 0.f, 0.f};
      const int q_row = q_mt * 16 + (lane & 15);
      const size_t qbase = (size_t)(q_row >> 2) * kXqStride + (q_row & 3) * 32;
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int ks2 = 0; ks2 < kBwdKv / 32; ++ks2) {
        const int kv_off = ks2 * 32 + (lane >> 4) * 8;
        const bf16x8 da = *reinterpret_cast<const bf16x8*>(
            x2_lds + qbase + (kv_off >> 4) * 128 + (kv_off & 15) * 2);
#pragma unroll
        for (int nt = 0; nt < kNTH; ++nt) {
          const int d = (nt0 + nt) * 16 + (lane & 15);
          const bf16x8 kb = *reinterpret_cast<const bf16x8*>(
              swz_t_at<kBwdKv>(reinterpret_cast<char*>(kt_lds), d, kv_off));
          dq_acc[nt] = mfma16(da, kb, dq_acc[nt]);
        }
      }
      __builtin_amdgcn_s_setprio(0);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int q_glob = qt + q_mt * 16 + (lane >> 4) * 4 + r;
        if (q_glob < Sq_loc) {
#pragma unroll
          for (int nt = 0; nt < kNTH; ++nt) {
            atomicAdd(dq + q_base +
                          (int64_t)(q_lo + q_glob) * q_row_stride +
                          (nt0 + nt) * 16 + (lane & 15),
                      dq_acc[nt][r]);
          }
        }
      }
    }
    // The Q/dO store overlaps the dV/dK/dQ MFMA phases above: nothing in
    // them reads q_lds/do_lds (their consumers — S^T, dP^T and the
    // transposes — all ran before the x-stage barrier), so the write only
    // needs the end-of-iteration barrier to publish for the next tile.
    if (qt + kBwdQ < Sq_loc) {
      store_qdo_lds();
    }
    __syncthreads();
  }

  // ---- flush dK, dV (atomicAdd: GQA groups and padded tiles overlap) -------
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kv_glob = kv0 + wave * 16 + (lane >> 4) * 4 + r;
    if (kv_glob < Skv_loc) {
#pragma unroll
      for (int nt = 0; nt < kNT; ++nt) {
        const int d = nt * 16 + (lane & 15);
        atomicAdd(dk + kv_base + (int64_t)(kv_lo + kv_glob) * kv_row_stride + d,
                  dk_acc[nt][r]);
        atomicAdd(dv + kv_base + (int64_t)(kv_lo + kv_glob) * kv_row_stride + d,
                  dv_acc[nt][r]);
      }
    }
  }
}

// MFMA fragment-map self-check: C = A@B for one 16x32 @ 32x16 tile.
__global__ void mfma_selfcheck_kernel(
    const bf16_t* __restrict__ a,  // (16, 32) row-major
    const bf16_t* __restrict__ b,  // (32, 16) row-major
    float* __restrict__ c) {       // (16, 16) row-major
  const int lane = threadIdx.x & 63;
  bf16x8 af, bf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    af[j] = a[(lane & 15) * 32 + (lane >> 4) * 8 + j];
    bf[j] = b[((lane >> 4) * 8 + j) * 16 + (lane & 15)];
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = mfma16(af, bf, acc);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    c[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[r];
  }
}

// Chained-fragment self-check, the forward's layout argument at its smallest
// size: X = A1 @ B1 (32x32 @ 32x16) as two 16-row C tiles whose A fragments
// take A1's rows in pv_pos order; X's C registers, packed as the forward packs
// P^T, are then the B operand of Y = A2 @ X with A2 (16x32) in natural order.
__global__ void mfma_chain_selfcheck_kernel(
    const bf16_t* __restrict__ a1,  // (32, 32) row-major
    const bf16_t* __restrict__ b1,  // (32, 16) row-major
    const bf16_t* __restrict__ a2,  // (16, 32) row-major
    float* __restrict__ y) {        // (16, 16) row-major
  const int lane = threadIdx.x & 63;
  bf16x8 bf, a2f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    bf[j] = b1[((lane >> 4) * 8 + j) * 16 + (lane & 15)];
    a2f[j] = a2[(lane & 15) * 32 + (lane >> 4) * 8 + j];
  }
  f32x4 x[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    bf16x8 af;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      af[j] = a1[pv_pos(t * 16 + (lane & 15)) * 32 + (lane >> 4) * 8 + j];
    }
    x[t] = mfma16(af, bf, f32x4{0.f, 0.f, 0.f, 0.f});
  }
  bf16x8 xb;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    xb[j] = (bf16_t)x[0][j];
    xb[4 + j] = (bf16_t)x[1][j];
  }
  const f32x4 acc = mfma16(a2f, xb, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    y[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = acc[r];
  }
}

// Fused fp32 -> bf16 cast of the three backward accumulators in ONE launch
// (the three at::native casts measured ~2.6 TB/s and ~0.7 ms per backward at
// bench shape). Sizes are multiples of 8 (B*S*H*D), so 8-float groups never
// straddle a buffer boundary.
__global__ void cast3_f32_bf16_kernel(
    const float* __restrict__ a, const float* __restrict__ b,
    const float* __restrict__ c,
    ushort* __restrict__ oa, ushort* __restrict__ ob, ushort* __restrict__ oc,
    int64_t na, int64_t nb, int64_t nc) {
  const int64_t total = na + nb + nc;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x * 8;
  for (int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
       i < total; i += stride) {
    const float* src;
    ushort* dst;
    int64_t off = i;
    if (off < na) {
      src = a; dst = oa;
    } else if (off < na + nb) {
      src = b; dst = ob; off -= na;
    } else {
      src = c; dst = oc; off -= na + nb;
    }
    f32x4 lo = *reinterpret_cast<const f32x4*>(src + off);
    f32x4 hi = *reinterpret_cast<const f32x4*>(src + off + 4);
    bf16x4_bits p0, p1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      p0.s[j] = bf16_bits((bf16_t)lo[j]);
      p1.s[j] = bf16_bits((bf16_t)hi[j]);
    }
    *reinterpret_cast<uint64_t*>(dst + off) = p0.u;
    *reinterpret_cast<uint64_t*>(dst + off + 4) = p1.u;
  }
}

}  // namespace d9d

// ---------------------------------------------------------------------------
// Host wrappers
// ---------------------------------------------------------------------------

namespace {

int padded_head_dim(int d) {
  for (int cand : {32, 64, 96, 128}) {
    if (d <= cand) return cand;
  }
  TORCH_CHECK(false, "head_dim too large: ", d);
  return -1;
}

torch::Tensor maybe_pad_d(torch::Tensor t, int D_pad) {
  const int D = t.size(-1);
  if (D == D_pad) return t.contiguous();
  auto padded = torch::zeros(
      {t.size(0), t.size(1), t.size(2), (int64_t)D_pad}, t.options());
  padded.narrow(-1, 0, D).copy_(t);
  return padded;
}

// Varlen launch metadata: device copies of the int32 cu_seqlens and of the
// per-sequence tile-count prefix that the kernels binary-search. All null / 0
// for a dense batch.
struct VarlenMeta {
  torch::Tensor cu_q, cu_k, pref;  // own the device memory behind the pointers
  const int *cu_q_ptr = nullptr, *cu_k_ptr = nullptr, *pref_ptr = nullptr;
  int nseq = 0, n_tiles = 0;
};

// The grid tiles each sequence's q (tile_kv = false) or kv in `tile` rows.
VarlenMeta prepare_varlen(const c10::optional<torch::Tensor>& cu_seqlens_q,
                          const c10::optional<torch::Tensor>& cu_seqlens_k,
                          int tile, bool tile_kv, c10::Device device) {
  VarlenMeta m;
  if (!cu_seqlens_q.has_value()) return m;
  auto cu_q_cpu = cu_seqlens_q->to(torch::kInt32).cpu().contiguous();
  auto cu_k_cpu = cu_seqlens_k->to(torch::kInt32).cpu().contiguous();
  m.nseq = cu_q_cpu.numel() - 1;
  auto pref = torch::empty({m.nseq + 1}, torch::dtype(torch::kInt32));
  const int* cu = (tile_kv ? cu_k_cpu : cu_q_cpu).data_ptr<int>();
  int* p = pref.data_ptr<int>();
  for (int i = 0; i < m.nseq; ++i) {
    p[i] = m.n_tiles;
    m.n_tiles += (cu[i + 1] - cu[i] + tile - 1) / tile;
  }
  p[m.nseq] = m.n_tiles;
  m.cu_q = cu_q_cpu.to(device, true);
  m.cu_k = cu_k_cpu.to(device, true);
  m.pref = pref.to(device, true);
  m.cu_q_ptr = m.cu_q.data_ptr<int>();
  m.cu_k_ptr = m.cu_k.data_ptr<int>();
  m.pref_ptr = m.pref.data_ptr<int>();
  return m;
}

// Calls f(std::integral_constant<int, D_pad>) for the instantiated head dims.
template <typename F>
void dispatch_head_dim(int D_pad, F&& f) {
  switch (D_pad) {
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 64: f(std::integral_constant<int, 64>{}); break;
    case 96: f(std::integral_constant<int, 96>{}); break;
    case 128: f(std::integral_constant<int, 128>{}); break;
  }
}

}  // namespace

std::vector<torch::Tensor> flash_attn_fwd(
    torch::Tensor q, torch::Tensor k, torch::Tensor v,
    c10::optional<torch::Tensor> sinks,
    c10::optional<torch::Tensor> cu_seqlens_q,
    c10::optional<torch::Tensor> cu_seqlens_k,
    bool causal, double softmax_scale, int64_t window_left, int64_t q_offset) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == torch::kBFloat16);
  const bool varlen = cu_seqlens_q.has_value();
  if (varlen) {
    TORCH_CHECK(q.dim() == 3, "varlen expects (total, H, D)");
    q = q.unsqueeze(0);
    k = k.unsqueeze(0);
    v = v.unsqueeze(0);
  }
  TORCH_CHECK(q.dim() == 4 && k.dim() == 4 && v.dim() == 4);
  const int B = q.size(0), Sq = q.size(1), Hq = q.size(2), D = q.size(3);
  const int Skv = k.size(1), Hkv = k.size(2);
  TORCH_CHECK(Hq % Hkv == 0, "GQA head mismatch");

  const int D_pad = padded_head_dim(D);
  auto qp = maybe_pad_d(q, D_pad);
  auto kp = maybe_pad_d(k, D_pad);
  auto vp = maybe_pad_d(v, D_pad);

  const VarlenMeta vl = prepare_varlen(cu_seqlens_q, cu_seqlens_k, d9d::kFwdQ,
                                       /*tile_kv=*/false, q.device());

  auto out = torch::empty_like(qp);
  auto lse = torch::empty({varlen ? 1 : B, Hq, Sq},
                          q.options().dtype(torch::kFloat32));
  const float* sinks_ptr = nullptr;
  torch::Tensor sinks_f;
  if (sinks.has_value()) {
    sinks_f = sinks->to(torch::kFloat32).contiguous();
    TORCH_CHECK(sinks_f.numel() == Hq, "sinks must be (Hq,)");
    sinks_ptr = sinks_f.data_ptr<float>();
  }

  const dim3 grid(varlen ? vl.n_tiles : (Sq + d9d::kFwdQ - 1) / d9d::kFwdQ,
                  varlen ? Hq : B * Hq);
  auto stream = at::hip::getCurrentHIPStream();

  dispatch_head_dim(D_pad, [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    hipLaunchKernelGGL((d9d::flash_fwd_kernel<DP>), grid, dim3(256),
                       d9d::fwd_smem_bytes<DP>(), stream,
                       reinterpret_cast<const __bf16*>(qp.data_ptr()),
                       reinterpret_cast<const __bf16*>(kp.data_ptr()),
                       reinterpret_cast<const __bf16*>(vp.data_ptr()),
                       reinterpret_cast<__bf16*>(out.data_ptr()),
                       lse.data_ptr<float>(), sinks_ptr, vl.cu_q_ptr,
                       vl.cu_k_ptr, vl.pref_ptr, vl.nseq, B, Sq, Skv, Hq, Hkv,
                       (float)softmax_scale, causal ? 1 : 0, (int)window_left,
                       (int)q_offset);
  });

  if (D_pad != D) out = out.narrow(-1, 0, D).contiguous();
  if (varlen) {
    out = out.squeeze(0);
    lse = lse.squeeze(0);  // (Hq, total)
  }
  return {out, lse};
}

std::vector<torch::Tensor> flash_attn_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse,
    c10::optional<torch::Tensor> cu_seqlens_q,
    c10::optional<torch::Tensor> cu_seqlens_k,
    bool causal, double softmax_scale, int64_t window_left, int64_t q_offset,
    c10::optional<torch::Tensor> dlse) {
  const bool varlen = cu_seqlens_q.has_value();
  if (varlen) {
    dout = dout.unsqueeze(0);
    q = q.unsqueeze(0);
    k = k.unsqueeze(0);
    v = v.unsqueeze(0);
    out = out.unsqueeze(0);
    lse = lse.unsqueeze(0);
  }
  const int B = q.size(0), Sq = q.size(1), Hq = q.size(2), D = q.size(3);
  const int Skv = k.size(1), Hkv = k.size(2);
  const int D_pad = padded_head_dim(D);

  const VarlenMeta vl = prepare_varlen(cu_seqlens_q, cu_seqlens_k, d9d::kBwdKv,
                                       /*tile_kv=*/true, q.device());

  auto qp = maybe_pad_d(q, D_pad);
  auto kp = maybe_pad_d(k, D_pad);
  auto vp = maybe_pad_d(v, D_pad);
  auto dop = maybe_pad_d(dout, D_pad);
  auto op = maybe_pad_d(out, D_pad);

  auto f32opt = q.options().dtype(torch::kFloat32);
  auto delta = torch::empty({B, Hq, Sq}, f32opt);
  // atomicAdd accumulators: cleared via the copy/DMA engine (hipMemsetAsync)
  // instead of torch::zeros — the fill kernels measured ~1.7 TB/s in-step
  // and 400 MB/call of clears showed up at ~1.3% of the whole bench step.
  auto dq32 = torch::empty({B, Sq, Hq, D_pad}, f32opt);
  auto dk32 = torch::empty({B, Skv, Hkv, D_pad}, f32opt);
  auto dv32 = torch::empty({B, Skv, Hkv, D_pad}, f32opt);

  auto stream = at::hip::getCurrentHIPStream();
  hipMemsetAsync(dq32.data_ptr(), 0, dq32.numel() * sizeof(float), stream);
  hipMemsetAsync(dk32.data_ptr(), 0, dk32.numel() * sizeof(float), stream);
  hipMemsetAsync(dv32.data_ptr(), 0, dv32.numel() * sizeof(float), stream);
  {
    const int64_t rows = (int64_t)B * Sq * Hq;
    hipLaunchKernelGGL(d9d::attn_delta_kernel, dim3(rows), dim3(64), 0, stream,
                       reinterpret_cast<const __bf16*>(dop.data_ptr()),
                       reinterpret_cast<const __bf16*>(op.data_ptr()),
                       delta.data_ptr<float>(), B, Sq, Hq, D_pad);
  }
  if (dlse.has_value()) {
    // lse is itself an output: d(lse_i)/d(S_ij) = P_ij, so its upstream grad
    // enters as dS = P*(dP - delta) + P*dlse = P*(dP - (delta - dlse)).
    auto g = dlse->to(torch::kFloat32);
    if (varlen) g = g.unsqueeze(0);
    TORCH_CHECK(g.is_cuda() && g.sizes() == delta.sizes(),
                "flash_attn_bwd: dlse must have the layout of lse");
    delta.sub_(g);
  }

  const dim3 grid(varlen ? vl.n_tiles : (Skv + d9d::kBwdKv - 1) / d9d::kBwdKv,
                  varlen ? Hq : B * Hq);
  dispatch_head_dim(D_pad, [&](auto dp) {
    constexpr int DP = decltype(dp)::value;
    hipLaunchKernelGGL((d9d::flash_bwd_kernel<DP>), grid,
                       dim3(d9d::kBwdThreads), d9d::bwd_smem_bytes<DP>(), stream,
                       reinterpret_cast<const __bf16*>(qp.data_ptr()),
                       reinterpret_cast<const __bf16*>(kp.data_ptr()),
                       reinterpret_cast<const __bf16*>(vp.data_ptr()),
                       reinterpret_cast<const __bf16*>(dop.data_ptr()),
                       lse.data_ptr<float>(), delta.data_ptr<float>(),
                       dq32.data_ptr<float>(), dk32.data_ptr<float>(),
                       dv32.data_ptr<float>(), vl.cu_q_ptr, vl.cu_k_ptr,
                       vl.pref_ptr, vl.nseq, B, Sq, Skv, Hq, Hkv,
                       (float)softmax_scale, causal ? 1 : 0, (int)window_left,
                       (int)q_offset);
  });

  torch::Tensor dq, dk, dv;
  if (D == D_pad) {
    // one fused cast launch for all three accumulators
    auto bf = q.options().dtype(torch::kBFloat16);
    dq = torch::empty(dq32.sizes(), bf);
    dk = torch::empty(dk32.sizes(), bf);
    dv = torch::empty(dv32.sizes(), bf);
    const int64_t na = dq32.numel(), nb = dk32.numel(), nc = dv32.numel();
    const int64_t groups = (na + nb + nc) / 8;
    const int blocks = (int)std::min<int64_t>((groups + 255) / 256, 16384);
    hipLaunchKernelGGL(d9d::cast3_f32_bf16_kernel, dim3(blocks), dim3(256), 0,
                       stream, dq32.data_ptr<float>(), dk32.data_ptr<float>(),
                       dv32.data_ptr<float>(),
                       reinterpret_cast<ushort*>(dq.data_ptr()),
                       reinterpret_cast<ushort*>(dk.data_ptr()),
                       reinterpret_cast<ushort*>(dv.data_ptr()),
                       na, nb, nc);
  } else {
    dq = dq32.narrow(-1, 0, D).to(torch::kBFloat16).contiguous();
    dk = dk32.narrow(-1, 0, D).to(torch::kBFloat16).contiguous();
    dv = dv32.narrow(-1, 0, D).to(torch::kBFloat16).contiguous();
  }
  if (varlen) {
    dq = dq.squeeze(0);
    dk = dk.squeeze(0);
    dv = dv.squeeze(0);
  }
  return {dq, dk, dv};
}

torch::Tensor mfma_selfcheck(torch::Tensor a, torch::Tensor b) {
  TORCH_CHECK(a.sizes() == torch::IntArrayRef({16, 32}));
  TORCH_CHECK(b.sizes() == torch::IntArrayRef({32, 16}));
  auto c = torch::empty({16, 16}, a.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(d9d::mfma_selfcheck_kernel, dim3(1), dim3(64), 0, stream,
                     reinterpret_cast<const __bf16*>(a.contiguous().data_ptr()),
                     reinterpret_cast<const __bf16*>(b.contiguous().data_ptr()),
                     c.data_ptr<float>());
  return c;
}

torch::Tensor mfma_chain_selfcheck(torch::Tensor a1, torch::Tensor b1,
                                   torch::Tensor a2) {
  TORCH_CHECK(a1.sizes() == torch::IntArrayRef({32, 32}));
  TORCH_CHECK(b1.sizes() == torch::IntArrayRef({32, 16}));
  TORCH_CHECK(a2.sizes() == torch::IntArrayRef({16, 32}));
  for (const auto& t : {a1, b1, a2}) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16);
  }
  auto a1c = a1.contiguous(), b1c = b1.contiguous(), a2c = a2.contiguous();
  auto y = torch::empty({16, 16}, a1.options().dtype(torch::kFloat32));
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(d9d::mfma_chain_selfcheck_kernel, dim3(1), dim3(64), 0,
                     stream, reinterpret_cast<const __bf16*>(a1c.data_ptr()),
                     reinterpret_cast<const __bf16*>(b1c.data_ptr()),
                     reinterpret_cast<const __bf16*>(a2c.data_ptr()),
                     y.data_ptr<float>());
  return y;
}
