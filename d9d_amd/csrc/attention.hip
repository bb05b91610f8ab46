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
// Layouts: q (B,Sq,Hq,Dqk), k (B,Skv,Hkv,Dqk), v (B,Skv,Hkv,Dv),
// out (B,Sq,Hq,Dv), lse (B,Hq,Sq). The kernels are templated on the pair
// <DQK, DV>: Q, K, S = Q K^T, dQ and dK run over DQK; V, O, dO, dP = dO V^T,
// dV and delta over DV. Instantiated: DQK = DV in {32, 64, 96, 128} and the
// one wide pair <192, 128> (MLA: qk 192 / v 128), whose forward takes 64 q
// rows per workgroup (one m-tile per wave) to stay inside 256 VGPRs and whose
// backward stages 32 q rows per tile instead of 64 to fit the LDS. The host
// pads other sizes up to the next pair; qk > 192 or v > 128 is an error.
#include "common.h"
#include "mfma.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <type_traits>

namespace d9d {

constexpr int kFwdQ = 128;   // forward: q rows per workgroup (4 waves x 32)
constexpr int kFwdQWide = 64;  // ... and for the wide pair <192, 128> (4 x 16)
constexpr int kFwdKv = 64;   // forward: kv rows per staged K/V tile
constexpr int kBwdQ = 64;    // backward: q rows per staged Q/dO tile (DQK <= 128)
constexpr int kBwdQWide = 32;  // ... and for the wide pair <192, 128>
constexpr int kBwdKv = 128;  // backward: kv rows per workgroup (8 waves x 16)
constexpr int kBwdThreads = 512;
constexpr float kLog2e = 1.44269504088896340736f;

// XOR swizzles keep ds_read_b128 bank-conflict-free (guide G4). The XOR moves
// 16-byte units and must stay inside the LDS row: a mask of m bits needs rows
// that are a multiple of 16 << m bytes. Row-major [rows][D] tiles (D*2-byte
// rows) use swz_rm_mask<D>() -- D = 96 has 192-byte rows, a multiple of 64
// only, so it takes the 2-bit mask, D = 192 (384-byte rows) the 3-bit one;
// transposed [D][ROWS] tiles use mask 7, or 3 where ROWS = 32 (64-byte rows).
template <int D>
constexpr int swz_rm_mask() {
  constexpr int mask = D == 128 ? 15 : ((D == 64 || D == 192) ? 7 : 3);
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
  constexpr int mask = ROWS * 2 >= 128 ? 7 : 3;
  static_assert((ROWS * 2) % (16 * (mask + 1)) == 0, "swizzle leaves its LDS row");
  return tile + d * (ROWS * 2) + ((r * 2) ^ ((d & mask) << 4));
}

// Transpose a swizzled row-major [ROWS][D] LDS image into a swizzled
// [D][ROWS] LDS image using 4B LDS reads + 8B LDS writes.
template <int D, int ROWS, int BLOCK = 256>
D9D_DEVICE void transpose_lds_tile(bf16_t* dst, const bf16_t* src_rm, int tid) {
  // Work mapping: consecutive threads take consecutive ROW-quads of the
  // same d-pair, so the two b64 writes of a ROWS/4-thread group land on one
  // [d][ROWS] row contiguously (128 B span at 64 rows, conflict-free). The
  // b32 source reads pay a 4-way conflict instead of the old mapping's 8-way
  // b64 write conflict (rows 256 B apart XOR-spread only 4 ways per group).
  constexpr int kQuads = ROWS / 4;
  for (int idx = tid; idx < kQuads * (D / 2); idx += BLOCK) {
    const int d0 = (idx / kQuads) * 2;
    const int rb = (idx % kQuads) * 4;
    bf16x4_bits c0, c1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t pair = *reinterpret_cast<const uint32_t*>(
          swz_rm_at<D>(reinterpret_cast<const char*>(src_rm), rb + i, d0));
      c0.s[i] = (ushort)(pair & 0xffffu);
      c1.s[i] = (ushort)(pair >> 16);
    }
    *reinterpret_cast<uint64_t*>(
        swz_t_at<ROWS>(reinterpret_cast<char*>(dst), d0, rb)) = c0.u;
    *reinterpret_cast<uint64_t*>(
        swz_t_at<ROWS>(reinterpret_cast<char*>(dst), d0 + 1, rb)) = c1.u;
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

// FQ: q rows per workgroup. Two workgroups per CU (a 256-VGPR budget); up to
// DQK = 128 the kernel just fits with kFwdQ rows (two m-tiles per wave). The
// wide pair holds 16 more q_frag and 8 more k_reg registers, so it takes
// kFwdQWide rows (one m-tile per wave) instead of spilling.
template <int DQK, int DV, int FQ>
__global__ __launch_bounds__(256, 2) void flash_fwd_kernel(
    const bf16_t* __restrict__ q,   // (B,Sq,Hq,DQK)
    const bf16_t* __restrict__ k,   // (B,Skv,Hkv,DQK)
    const bf16_t* __restrict__ v,   // (B,Skv,Hkv,DV)
    bf16_t* __restrict__ out,       // (B,Sq,Hq,DV); DQK > 128: (2,B,Sq,Hq,DV)
    float* __restrict__ lse,        // (B,Hq,Sq)
    const float* __restrict__ sinks,  // (Hq,) raw sink logits, or nullptr
    const int* __restrict__ cu_q,     // (nseq+1,) packed-seq bounds, or nullptr
    const int* __restrict__ cu_k,
    const int* __restrict__ qtile_pref,  // (nseq+1,) prefix of ceil(len_q/FQ)
    int nseq,
    int B, int Sq, int Skv, int Hq, int Hkv,
    float scale, int causal, int window_left, int q_offset) {
  static_assert(DV <= DQK, "the O staging reuses the K tile");
  static_assert(FQ == 128 || FQ == 64, "q rows per workgroup");
  constexpr int kM = FQ / 64;     // 16-row q m-tiles per wave
  constexpr int kWaveQ = FQ / 4;  // q rows per wave
  // The wide pair writes O's bf16 rounding residual as a second plane behind
  // `out`, (2,B,Sq,Hq,DV): with it delta = rowsum(dO * O) is as exact as with
  // an fp32 O. From the rounded O alone delta's error reaches dS un-averaged
  // when the softmax is near one-hot (dq, dk off by 1e-1 at scale 0.5).
  constexpr bool kOutLo = DQK > 128;
  constexpr int kNT = DV / 16;   // n-tiles over the v head dim
  constexpr int kKS = DQK / 32;  // k-steps over the qk head dim

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // [kFwdKv][DQK] swizzled, row p = kv row pv_pos(p); fwd_smem_bytes() is
  // this carve-up
  bf16_t* k_lds = reinterpret_cast<bf16_t*>(smem);
  bf16_t* vt_lds = k_lds + kFwdKv * DQK;             // [DV][kFwdKv] transposed

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int lrow = lane & 15;  // the q row (of a 16-row sub-tile) this lane owns
  const int lgrp = lane >> 4;
  const bool upper = lane >= 32;

  // one (b, h)'s q-tiles share its KV stream (XCD grouping)
  const TileLoc loc = locate_tile<FQ, false>(
      cu_q, cu_k, qtile_pref, nseq, Sq, Skv, Hq, q_offset);
  if (!loc.valid) return;
  const int b = loc.b, h = loc.h, q_tile = loc.tile, causal_off = loc.causal_off;
  const int q_lo = loc.q_lo, Sq_loc = loc.Sq_loc, kv_lo = loc.kv_lo, Skv_loc = loc.Skv_loc;
  const int hkv = h / (Hq / Hkv);

  const int64_t q_base = ((int64_t)b * Sq * Hq + h) * DQK;
  const int64_t kv_base = ((int64_t)b * Skv * Hkv + hkv) * DQK;
  const int64_t q_row_stride = (int64_t)Hq * DQK;
  const int64_t kv_row_stride = (int64_t)Hkv * DQK;
  // the same for the DV-wide tensors (v, out); one value where DQK == DV
  const int64_t o_base = DQK == DV ? q_base : ((int64_t)b * Sq * Hq + h) * DV;
  const int64_t v_base = DQK == DV ? kv_base : ((int64_t)b * Skv * Hkv + hkv) * DV;
  const int64_t o_row_stride = DQK == DV ? q_row_stride : (int64_t)Hq * DV;
  const int64_t v_row_stride = DQK == DV ? kv_row_stride : (int64_t)Hkv * DV;

  // ---- load this wave's 32 q rows (2 sub-tiles) into fragments -------------
  // The kernel computes the TRANSPOSED products S^T = K Q^T and
  // O^T = V^T P^T: Q is the B operand, and in the C layout of S^T and O^T
  // every value a lane holds belongs to ONE q row (lane & 15). The row
  // statistics are then per lane, and the S^T registers are already a legal
  // B operand for PV (see pv_pos): P never leaves the registers.
  bf16x8 q_frag[kM][kKS];
#pragma unroll
  for (int m = 0; m < kM; ++m) {
    const int q_row_local = q_tile * FQ + wave * kWaveQ + m * 16 + lrow;
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
  float m_run[kM], l_run[kM][4];
#pragma unroll
  for (int m = 0; m < kM; ++m) {
    m_run[m] = m_init;
#pragma unroll
    for (int r = 0; r < 4; ++r) l_run[m][r] = r == 0 ? l_init : 0.f;
  }
  f32x4 o_acc[kM][kNT];  // O^T: lane holds O[q = lrow][d = nt*16 + lgrp*4 + r]
#pragma unroll
  for (int m = 0; m < kM; ++m)
#pragma unroll
    for (int nt = 0; nt < kNT; ++nt) o_acc[m][nt] = {0.f, 0.f, 0.f, 0.f};

  const int q_tile_last_row = min(q_tile * FQ + FQ - 1, Sq_loc - 1);
  int kv_end = Skv_loc;
  if (causal) kv_end = min(Skv_loc, q_tile_last_row + causal_off + 1);
  const int num_kv_tiles = (kv_end + kFwdKv - 1) / kFwdKv;
  if (num_kv_tiles <= 0) return;

  // T14 split staging: next tile's K rows and V (4x2 transpose blocks) are
  // loaded into registers while the current tile's MFMAs run; LDS writes and
  // their vmcnt waits land after the compute barrier.
  constexpr int kKIters = (kFwdKv * DQK) / (256 * 8);
  constexpr int kVIters = (kFwdKv / 4) * (DV / 2) / 256;
  static_assert(kKIters * 256 * 8 == kFwdKv * DQK &&
                kVIters * 256 == (kFwdKv / 4) * (DV / 2), "staging covers the tiles");
  bf16x8 k_reg[kKIters];
  bf16x4_bits v_c0[kVIters], v_c1[kVIters];

  auto load_regs = [&](int kt) {
    const int kv0 = kt * kFwdKv;
#pragma unroll
    for (int it = 0; it < kKIters; ++it) {
      const int idx = (threadIdx.x + it * 256) * 8;
      const int row = idx / DQK;
      const int col = idx % DQK;
      const int g_row = kv_lo + min(kv0 + pv_pos(row), Skv_loc - 1);
      k_reg[it] = *reinterpret_cast<const bf16x8*>(
          k + kv_base + (int64_t)g_row * kv_row_stride + col);
    }
#pragma unroll
    for (int it = 0; it < kVIters; ++it) {
      // (v_base is kv_base where DQK == DV, but as one more captured variable
      // it changes how the D = 32 prologue is vectorized and scheduled)
      if constexpr (DQK == DV) {
        load_transposed_block<DV>(v_c0[it], v_c1[it], v + kv_base, kv_row_stride,
                                  kv_lo, kv0, Skv_loc - 1, threadIdx.x + it * 256);
      } else {
        load_transposed_block<DV>(v_c0[it], v_c1[it], v + v_base, v_row_stride,
                                  kv_lo, kv0, Skv_loc - 1, threadIdx.x + it * 256);
      }
    }
  };

  auto store_lds = [&]() {
#pragma unroll
    for (int it = 0; it < kKIters; ++it) {
      const int idx = (threadIdx.x + it * 256) * 8;
      *reinterpret_cast<bf16x8*>(
          swz_rm_at<DQK>(reinterpret_cast<char*>(k_lds), idx / DQK, idx % DQK)) =
          k_reg[it];
    }
#pragma unroll
    for (int it = 0; it < kVIters; ++it) {
      store_transposed_block<DV, kFwdKv>(vt_lds, v_c0[it], v_c1[it],
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
    f32x4 st[kM][4];
#pragma unroll
    for (int m = 0; m < kM; ++m)
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
            swz_rm_at<DQK>(reinterpret_cast<char*>(k_lds), kv_row, d0));
#pragma unroll
        for (int m = 0; m < kM; ++m) st[m][nt] = mfma16(ka, q_frag[m][ks], st[m][nt]);
      }
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- per-lane online softmax; P^T packed as PV's B operand -------------
    bf16x8 pb[kM][2];  // [m][ks2]
#pragma unroll
    for (int m = 0; m < kM; ++m) {
      const int my_q_row = q_tile * FQ + wave * kWaveQ + m * 16;
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
        for (int m = 0; m < kM; ++m) o_acc[m][nt] = mfma16(va, pb[m][ks2], o_acc[m][nt]);
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
  for (int m = 0; m < kM; ++m) {
    // butterfly over the 16 column classes in the order c ^ 1, 2, 4, 8
    l_run[m][0] = (l_run[m][0] + l_run[m][1]) + (l_run[m][2] + l_run[m][3]);
    l_run[m][0] += __shfl_xor(l_run[m][0], 32, 64);
    l_run[m][0] += __shfl_xor(l_run[m][0], 16, 64);
  }
  {
    // reuse: swizzled [64][DV], staged once per 64-row half of the q tile
    char* o_lds = reinterpret_cast<char*>(k_lds);
#pragma unroll
    for (int half = 0; half < FQ / 64; ++half) {
      __syncthreads();
      // FQ = 128: waves 0,1 hold q rows 0..63 of the tile; waves 2,3 rows
      // 64..127. FQ = 64: every wave holds 16 rows of the one half.
      if ((FQ == 128 ? (wave >> 1) : 0) == half) {
#pragma unroll
        for (int m = 0; m < kM; ++m) {
          const float inv_l = (l_run[m][0] > 0.f) ? 1.f / l_run[m][0] : 0.f;
          const int row = (FQ == 128 ? (wave & 1) * 32 : wave * 16) + m * 16 + lrow;
#pragma unroll
          for (int nt = 0; nt < kNT; ++nt) {
            bf16x4_bits o4;  // 4 consecutive d of one row
#pragma unroll
            for (int r = 0; r < 4; ++r)
              o4.s[r] = bf16_bits((bf16_t)(o_acc[m][nt][r] * inv_l));
            *reinterpret_cast<uint64_t*>(
                swz_rm_at<DV>(o_lds, row, nt * 16 + lgrp * 4)) = o4.u;
          }
        }
      }
      __syncthreads();
      constexpr int elems = 64 * DV;
      for (int idx = threadIdx.x * 8; idx < elems; idx += 256 * 8) {
        const int row = idx / DV;
        const int col = idx % DV;
        const int rg = q_tile * FQ + half * 64 + row;
        if (rg < Sq_loc) {
          *reinterpret_cast<bf16x8*>(
              out + o_base + (int64_t)(q_lo + rg) * o_row_stride + col) =
              *reinterpret_cast<const bf16x8*>(swz_rm_at<DV>(o_lds, row, col));
        }
      }
      if constexpr (kOutLo) {
        // Second plane of `out`: the bf16 rounding residual O - bf16(O), the
        // same way through LDS. The backward adds it back in delta.
        __syncthreads();
        if ((FQ == 128 ? (wave >> 1) : 0) == half) {
#pragma unroll
          for (int m = 0; m < kM; ++m) {
            const float inv_l = (l_run[m][0] > 0.f) ? 1.f / l_run[m][0] : 0.f;
            const int row = (FQ == 128 ? (wave & 1) * 32 : wave * 16) + m * 16 + lrow;
#pragma unroll
            for (int nt = 0; nt < kNT; ++nt) {
              bf16x4_bits o4;
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const float o = o_acc[m][nt][r] * inv_l;
                o4.s[r] = bf16_bits((bf16_t)(o - (float)(bf16_t)o));
              }
              *reinterpret_cast<uint64_t*>(
                  swz_rm_at<DV>(o_lds, row, nt * 16 + lgrp * 4)) = o4.u;
            }
          }
        }
        __syncthreads();
        bf16_t* out_lo = out + (int64_t)B * Sq * Hq * DV;
        for (int idx = threadIdx.x * 8; idx < elems; idx += 256 * 8) {
          const int row = idx / DV;
          const int col = idx % DV;
          const int rg = q_tile * FQ + half * 64 + row;
          if (rg < Sq_loc) {
            *reinterpret_cast<bf16x8*>(
                out_lo + o_base + (int64_t)(q_lo + rg) * o_row_stride + col) =
                *reinterpret_cast<const bf16x8*>(swz_rm_at<DV>(o_lds, row, col));
          }
        }
      }
    }
    if (lgrp == 0) {
#pragma unroll
      for (int m = 0; m < kM; ++m) {
        const int rg = q_tile * FQ + wave * kWaveQ + m * 16 + lrow;
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
template <int DQK, int DV>
constexpr size_t fwd_smem_bytes() {
  return sizeof(bf16_t) * (kFwdKv * DQK + DV * kFwdKv);
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

// The same with O given as its bf16 value plus its rounding residual (the
// wide forward's second plane): delta = sum_d dO * (O + O_lo).
__global__ void attn_delta_lo_kernel(
    const bf16_t* __restrict__ dout,  // (B,Sq,Hq,D)
    const bf16_t* __restrict__ out,
    const bf16_t* __restrict__ out_lo,
    float* __restrict__ delta,        // (B,Hq,Sq)
    int B, int Sq, int Hq, int D) {
  const int64_t row = blockIdx.x;  // over B*Sq*Hq
  if (row >= (int64_t)B * Sq * Hq) return;
  const int h = row % Hq;
  const int s = (row / Hq) % Sq;
  const int b = row / ((int64_t)Hq * Sq);
  float acc = 0.f;
  for (int i = threadIdx.x; i < D; i += 64) {
    acc += (float)dout[row * D + i] *
           ((float)out[row * D + i] + (float)out_lo[row * D + i]);
  }
  acc = wave_reduce_sum(acc);
  if (threadIdx.x == 0) {
    delta[((int64_t)b * Hq + h) * Sq + s] = acc;
  }
}

// P / dS images: kBwdKv / 16 blocks of 128 B per 4-q row, stride padded +32 B.
constexpr int kBwdXStride = (kBwdKv / 16) * 128 + 32;

// Q, dO, dO^T, Q^T tiles (QR q rows each) + K^T + the P and dS images. At
// <192, 128> 64 q rows would need 164864 B, 1 KiB over a workgroup's 160 KiB;
// 32 rows need 107008 B.
template <int DQK, int DV, int QR>
constexpr size_t bwd_smem_bytes() {
  return sizeof(bf16_t) * (2 * QR * DQK + 2 * QR * DV + DQK * kBwdKv) +
         2 * (QR / 4) * kBwdXStride;
}

// QR: q rows per staged Q/dO tile (kBwdQ, or kBwdQWide for the wide pair).
template <int DQK, int DV, int QR>
__global__ __launch_bounds__(512, 1) void flash_bwd_kernel(
    const bf16_t* __restrict__ q,
    const bf16_t* __restrict__ k,
    const bf16_t* __restrict__ v,
    const bf16_t* __restrict__ dout,
    const float* __restrict__ lse,    // (B,Hq,Sq)
    const float* __restrict__ delta,  // (B,Hq,Sq)
    float* __restrict__ dq,           // (B,Sq,Hq,DQK) fp32 accum
    float* __restrict__ dk,           // (B,Skv,Hkv,DQK) fp32 accum
    float* __restrict__ dv,           // (B,Skv,Hkv,DV) fp32 accum
    const int* __restrict__ cu_q,     // packed-seq bounds, or nullptr
    const int* __restrict__ cu_k,
    const int* __restrict__ kvtile_pref,  // prefix of ceil(len_k/kBwdKv)
    int nseq,
    int B, int Sq, int Skv, int Hq, int Hkv,
    float scale, int causal, int window_left, int q_offset) {
  static_assert(DV <= DQK, "the loops over DQK carry the DV work along");
  static_assert(QR == 64 || QR == 32, "q tile rows");
  constexpr int kNT = DQK / 16;   // n-tiles over the qk head dim (dK, dQ)
  constexpr int kKS = DQK / 32;   // k-steps over the qk head dim (S)
  constexpr int kNTV = DV / 16;   // n-tiles over the v head dim (dV)
  constexpr int kKSV = DV / 32;   // k-steps over the v head dim (dP)
  constexpr int kQT = QR / 16;    // 16-row q m-tiles per staged tile
  // dQ: the 8 waves split into kQT m-tiles x (8 / kQT) slices of the head dim
  constexpr int kDqParts = 8 / kQT;
  static_assert(kNT % kDqParts == 0, "dQ splits the head dim evenly");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  // Separate buffers for every staged operand: the three MFMA phases
  // (dV, dK, dQ) then run back-to-back with NO barrier between them, and the
  // whole q-tile iteration needs 4 __syncthreads instead of 8 (PMC showed
  // ~50% of bwd wave cycles parked on barriers with the shared-buffer
  // schedule). 149 KB LDS at D=128 -- one workgroup per CU, which this
  // kernel is at anyway.
  // bwd_smem_bytes() is this carve-up.
  bf16_t* q_lds = reinterpret_cast<bf16_t*>(smem);   // [QR][DQK] swizzled rows
  bf16_t* do_lds = q_lds + QR * DQK;                 // [QR][DV]
  bf16_t* tdo_lds = do_lds + QR * DV;                // [DV][QR]: dO^T
  bf16_t* tq_lds = tdo_lds + DV * QR;                // [DQK][QR]: Q^T
  bf16_t* kt_lds = tq_lds + DQK * QR;                // [DQK][kBwdKv]
  // P and dS live in ONE q-major blocked image each: [4 q][16 kv] 128-B
  // tr16 blocks at (q>>2, kv>>4), qb stride padded +32 B so the packed
  // b64 stores of 4 kv values per (q, nt) are bank-spread. dV/dK read
  // their kv-major A fragments via ds_read_b64_tr_b16 pairs; dQ reads its
  // q-major fragments as plain 16-B rows of the SAME dS image — the old
  // third (q-major) copy and 48 scalar stores per wave are gone.
  constexpr int kXqStride = kBwdXStride;             // bytes per q-block row
  char* x1_lds = reinterpret_cast<char*>(kt_lds + DQK * kBwdKv);  // P image
  char* x2_lds = x1_lds + (QR / 4) * kXqStride;                   // dS image

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;   // 8 waves x 16 kv rows = 128 kv/block

  // one (b, h)'s kv-tiles share its Q/dO/lse streams (XCD grouping)
  const TileLoc loc = locate_tile<kBwdKv, true>(
      cu_q, cu_k, kvtile_pref, nseq, Sq, Skv, Hq, q_offset);
  if (!loc.valid || loc.Sq_loc <= 0) return;
  const int b = loc.b, h = loc.h, kv_tile = loc.tile, causal_off = loc.causal_off;
  const int q_lo = loc.q_lo, Sq_loc = loc.Sq_loc, kv_lo = loc.kv_lo, Skv_loc = loc.Skv_loc;
  const int hkv = h / (Hq / Hkv);

  const int64_t q_base = ((int64_t)b * Sq * Hq + h) * DQK;
  const int64_t kv_base = ((int64_t)b * Skv * Hkv + hkv) * DQK;
  const int64_t q_row_stride = (int64_t)Hq * DQK;
  const int64_t kv_row_stride = (int64_t)Hkv * DQK;
  // the same for the DV-wide tensors (dout; v, dv); one value where DQK == DV
  const int64_t o_base = DQK == DV ? q_base : ((int64_t)b * Sq * Hq + h) * DV;
  const int64_t v_base = DQK == DV ? kv_base : ((int64_t)b * Skv * Hkv + hkv) * DV;
  const int64_t o_row_stride = DQK == DV ? q_row_stride : (int64_t)Hq * DV;
  const int64_t v_row_stride = DQK == DV ? kv_row_stride : (int64_t)Hkv * DV;
  const float* lse_row = lse + ((int64_t)b * Hq + h) * Sq + q_lo;
  const float* delta_row = delta + ((int64_t)b * Hq + h) * Sq + q_lo;

  const int kv0 = kv_tile * kBwdKv;

  // This wave's 16 kv rows: K and V A-fragments in registers.
  const int kv_row_local = lane & 15;
  const int kv_row_global =
      kv_lo + min(kv0 + wave * 16 + kv_row_local, Skv_loc - 1);
  bf16x8 k_frag[kKS], v_frag[kKSV];
  {
    const bf16_t* kp = k + kv_base + (int64_t)kv_row_global * kv_row_stride;
    const bf16_t* vp = v + v_base + (int64_t)kv_row_global * v_row_stride;
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) {
      const int d0 = ks * 32 + (lane >> 4) * 8;
      k_frag[ks] = *reinterpret_cast<const bf16x8*>(kp + d0);
      if (ks < kKSV) v_frag[ks] = *reinterpret_cast<const bf16x8*>(vp + d0);
    }
  }

  // Stage K^T once (for dQ's B fragments).
  stage_transposed_tile<DQK, kBwdKv, kBwdThreads>(
      kt_lds, k + kv_base, kv_row_stride, kv_lo, kv0, Skv_loc - 1, threadIdx.x);

  f32x4 dk_acc[kNT], dv_acc[kNTV];
#pragma unroll
  for (int nt = 0; nt < kNT; ++nt) {
    dk_acc[nt] = {0.f, 0.f, 0.f, 0.f};
    if (nt < kNTV) dv_acc[nt] = {0.f, 0.f, 0.f, 0.f};
  }

  int q_start = 0;
  if (causal) {
    // first q tile whose last aligned position reaches kv0
    q_start = (max(kv0 - causal_off, 0) / QR) * QR;
  }
  if (q_start >= Sq_loc) return;

  // T14: each q-tile's Q/dO rows are prefetched into registers while the
  // previous tile's MFMAs run; the transposed images are derived from the
  // row-major LDS copies (cheap ds_reads) instead of re-reading global.
  // Work item idx is an 8-element group of the [QR][DQK] Q tile and, while
  // idx < QR * DV, of the narrower [QR][DV] dO tile as well.
  constexpr int kQRegs =
      (QR * DQK + kBwdThreads * 8 - 1) / (kBwdThreads * 8);  // >= 1
  constexpr int kDoRegs = (QR * DV + kBwdThreads * 8 - 1) / (kBwdThreads * 8);
  bf16x8 q_reg[kQRegs], do_reg[kDoRegs];

  auto load_qdo_regs = [&](int qt_next) {
#pragma unroll
    for (int it = 0; it < kQRegs; ++it) {
      const int idx = (threadIdx.x + it * kBwdThreads) * 8;
      if (idx >= QR * DQK) break;
      const int row = idx / DQK;
      const int col = idx % DQK;
      const int g_row = q_lo + min(qt_next + row, Sq_loc - 1);
      q_reg[it] = *reinterpret_cast<const bf16x8*>(
          q + q_base + (int64_t)g_row * q_row_stride + col);
      if constexpr (DQK == DV) {
        do_reg[it] = *reinterpret_cast<const bf16x8*>(
            dout + q_base + (int64_t)g_row * q_row_stride + col);
      } else if (it < kDoRegs && idx < QR * DV) {
        const int o_row = q_lo + min(qt_next + idx / DV, Sq_loc - 1);
        do_reg[it] = *reinterpret_cast<const bf16x8*>(
            dout + o_base + (int64_t)o_row * o_row_stride + idx % DV);
      }
    }
  };
  auto store_qdo_lds = [&]() {
#pragma unroll
    for (int it = 0; it < kQRegs; ++it) {
      const int idx = (threadIdx.x + it * kBwdThreads) * 8;
      if (idx >= QR * DQK) break;
      const int row = idx / DQK;
      const int col = idx % DQK;
      *reinterpret_cast<bf16x8*>(
          swz_rm_at<DQK>(reinterpret_cast<char*>(q_lds), row, col)) = q_reg[it];
      if constexpr (DQK == DV) {
        *reinterpret_cast<bf16x8*>(
            swz_rm_at<DV>(reinterpret_cast<char*>(do_lds), row, col)) = do_reg[it];
      } else if (it < kDoRegs && idx < QR * DV) {
        *reinterpret_cast<bf16x8*>(swz_rm_at<DV>(
            reinterpret_cast<char*>(do_lds), idx / DV, idx % DV)) = do_reg[it];
      }
    }
  };

  load_qdo_regs(q_start);
  store_qdo_lds();
  __syncthreads();

  for (int qt = q_start; qt < Sq_loc; qt += QR) {
    if (qt + QR < Sq_loc) load_qdo_regs(qt + QR);  // issue early
    // dO^T and Q^T images for the dV/dK B fragments (cheap LDS-to-LDS).
    // NO barrier here: tdo/tq are first read after the x-stage barrier
    // below, which also publishes these writes (2 barriers per q-tile
    // instead of 4 — the PMC wave-parked share was the top bwd cost).
    transpose_lds_tile<DV, QR, kBwdThreads>(tdo_lds, do_lds, threadIdx.x);
    transpose_lds_tile<DQK, QR, kBwdThreads>(tq_lds, q_lds, threadIdx.x);

    // ---- S^T = K @ Q^T (per wave: 16 kv x QR q) ----------------------------
    f32x4 st_acc[kQT];
#pragma unroll
    for (int nt = 0; nt < kQT; ++nt) st_acc[nt] = {0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int nt = 0; nt < kQT; ++nt) {
      const int q_row = nt * 16 + (lane & 15);
#pragma unroll
      for (int ks = 0; ks < kKS; ++ks) {
        const int d0 = ks * 32 + (lane >> 4) * 8;
        const bf16x8 qb = *reinterpret_cast<const bf16x8*>(
            swz_rm_at<DQK>(reinterpret_cast<char*>(q_lds), q_row, d0));
        st_acc[nt] = mfma16(k_frag[ks], qb, st_acc[nt]);
      }
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- P^T = exp(S^T * scale - lse[q]); masked entries 0 -----------------
    // Tile-level mask skip (see fwd): interior tiles take the select-free
    // path, only diagonal/edge tiles run the per-element mask chain.
    const bool any_mask =
        (kv0 + kBwdKv > Skv_loc) || (qt + QR > Sq_loc) ||
        (causal && kv0 + kBwdKv - 1 > qt + causal_off) ||
        (window_left >= 0 &&
         kv0 < qt + QR - 1 + causal_off - window_left);
    float pt_val[kQT][4];  // [nt][r]
    if (any_mask) {
#pragma unroll
      for (int nt = 0; nt < kQT; ++nt) {
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
      for (int nt = 0; nt < kQT; ++nt) {
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
    f32x4 dpt_acc[kQT];
#pragma unroll
    for (int nt = 0; nt < kQT; ++nt) dpt_acc[nt] = {0.f, 0.f, 0.f, 0.f};
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int nt = 0; nt < kQT; ++nt) {
      const int q_row = nt * 16 + (lane & 15);
#pragma unroll
      for (int ks = 0; ks < kKSV; ++ks) {
        const int d0 = ks * 32 + (lane >> 4) * 8;
        const bf16x8 db = *reinterpret_cast<const bf16x8*>(
            swz_rm_at<DV>(reinterpret_cast<char*>(do_lds), q_row, d0));
        dpt_acc[nt] = mfma16(v_frag[ks], db, dpt_acc[nt]);
      }
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- dS^T = P^T * (dP^T - delta[q]) * scale ---------------------------
    float dst_val[kQT][4];
#pragma unroll
    for (int nt = 0; nt < kQT; ++nt) {
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
      for (int nt = 0; nt < kQT; ++nt) {
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
      for (int ks2 = 0; ks2 < QR / 32; ++ks2) {
        const int q_off = ks2 * 32 + (lane >> 4) * 8;
        const bf16x8 pa = xfrag(x1_lds, q_off);
        const bf16x8 da = xfrag(x2_lds, q_off);
#pragma unroll
        for (int nt = 0; nt < kNT; ++nt) {
          const int d = nt * 16 + (lane & 15);
          bf16x8 dob;  // dV has DV / 16 n-tiles, dK DQK / 16
          if (nt < kNTV) {
            dob = *reinterpret_cast<const bf16x8*>(
                swz_t_at<QR>(reinterpret_cast<char*>(tdo_lds), d, q_off));
          }
          const bf16x8 qb = *reinterpret_cast<const bf16x8*>(
              swz_t_at<QR>(reinterpret_cast<char*>(tq_lds), d, q_off));
          if (nt < kNTV) dv_acc[nt] = mfma16(pa, dob, dv_acc[nt]);
          dk_acc[nt] = mfma16(da, qb, dk_acc[nt]);
        }
      }
      __builtin_amdgcn_s_setprio(0);
    }

    // ---- dQ partial = dS @ K; atomicAdd (A = dS q-major via x3) -----------
    {
      // ALL 8 waves: wave & 3 picks the 16-row q m-tile, wave >> 2 the
      // d-half -- the old waves-0-3-only split parked half the block
      // through an entire MFMA phase. (32 q rows: wave & 1 and the d-quarter
      // wave >> 1.)
      constexpr int kNTH = kNT / kDqParts;  // nt per d-slice
      const int q_mt = wave & (kQT - 1);
      const int nt0 = (wave >> (kQT == 4 ? 2 : 1)) * kNTH;
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
    if (qt + QR < Sq_loc) {
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
        if (nt < kNTV) {
          atomicAdd(dv + v_base + (int64_t)(kv_lo + kv_glob) * v_row_stride + d,
                    dv_acc[nt][r]);
        }
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

// The instantiated <DQK, DV> pair a (qk, v) head-dim pair is padded to: one
// common D in {32, 64, 96, 128} while both fit, else the wide pair.
struct HeadDims {
  int qk, v;
};

HeadDims padded_head_dims(int d_qk, int d_v) {
  const int d = std::max(d_qk, d_v);
  for (int cand : {32, 64, 96, 128}) {
    if (d <= cand) return {cand, cand};
  }
  TORCH_CHECK(d_qk <= 192 && d_v <= 128,
              "flash attention supports qk head_dim <= 192 with v head_dim <= "
              "128; got qk ", d_qk, ", v ", d_v);
  return {192, 128};
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

// Calls f(integral_constant<DQK>, integral_constant<DV>) for the instantiated
// pairs (what padded_head_dims returns).
template <typename F>
void dispatch_head_dims(HeadDims d, F&& f) {
  using std::integral_constant;
  switch (d.qk) {
    case 32: f(integral_constant<int, 32>{}, integral_constant<int, 32>{}); break;
    case 64: f(integral_constant<int, 64>{}, integral_constant<int, 64>{}); break;
    case 96: f(integral_constant<int, 96>{}, integral_constant<int, 96>{}); break;
    case 128: f(integral_constant<int, 128>{}, integral_constant<int, 128>{}); break;
    case 192: f(integral_constant<int, 192>{}, integral_constant<int, 128>{}); break;
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
  const int Skv = k.size(1), Hkv = k.size(2), Dv = v.size(3);
  TORCH_CHECK(Hq % Hkv == 0, "GQA head mismatch");
  TORCH_CHECK(k.size(3) == D && v.size(1) == Skv && v.size(2) == Hkv,
              "flash_attn_fwd: k/v shape mismatch");

  const HeadDims pad = padded_head_dims(D, Dv);
  auto qp = maybe_pad_d(q, pad.qk);
  auto kp = maybe_pad_d(k, pad.qk);
  auto vp = maybe_pad_d(v, pad.v);

  const int fq = pad.qk > 128 ? d9d::kFwdQWide : d9d::kFwdQ;  // q rows per workgroup
  const VarlenMeta vl = prepare_varlen(cu_seqlens_q, cu_seqlens_k, fq,
                                       /*tile_kv=*/false, q.device());

  // the wide pair writes a second plane: O's bf16 rounding residual
  const bool wide = pad.qk > 128;
  auto out2 = wide ? torch::empty({2, B, Sq, Hq, (int64_t)pad.v}, qp.options())
                   : torch::empty({B, Sq, Hq, (int64_t)pad.v}, qp.options());
  auto out = wide ? out2.select(0, 0) : out2;
  auto lse = torch::empty({varlen ? 1 : B, Hq, Sq},
                          q.options().dtype(torch::kFloat32));
  const float* sinks_ptr = nullptr;
  torch::Tensor sinks_f;
  if (sinks.has_value()) {
    sinks_f = sinks->to(torch::kFloat32).contiguous();
    TORCH_CHECK(sinks_f.numel() == Hq, "sinks must be (Hq,)");
    sinks_ptr = sinks_f.data_ptr<float>();
  }

  const dim3 grid(varlen ? vl.n_tiles : (Sq + fq - 1) / fq,
                  varlen ? Hq : B * Hq);
  auto stream = at::hip::getCurrentHIPStream();

  dispatch_head_dims(pad, [&](auto dqk, auto dv) {
    constexpr int DQK = decltype(dqk)::value, DV = decltype(dv)::value;
    constexpr int FQ = DQK > 128 ? d9d::kFwdQWide : d9d::kFwdQ;
    hipLaunchKernelGGL((d9d::flash_fwd_kernel<DQK, DV, FQ>), grid, dim3(256),
                       (d9d::fwd_smem_bytes<DQK, DV>()), stream,
                       reinterpret_cast<const __bf16*>(qp.data_ptr()),
                       reinterpret_cast<const __bf16*>(kp.data_ptr()),
                       reinterpret_cast<const __bf16*>(vp.data_ptr()),
                       reinterpret_cast<__bf16*>(out2.data_ptr()),
                       lse.data_ptr<float>(), sinks_ptr, vl.cu_q_ptr,
                       vl.cu_k_ptr, vl.pref_ptr, vl.nseq, B, Sq, Skv, Hq, Hkv,
                       (float)softmax_scale, causal ? 1 : 0, (int)window_left,
                       (int)q_offset);
  });

  if (pad.v != Dv) out = out.narrow(-1, 0, Dv).contiguous();
  if (varlen) {
    out = out.squeeze(0);
    lse = lse.squeeze(0);  // (Hq, total)
  }
  if (!wide) return {out, lse};
  // third result, wide pair only: the residual, for flash_attn_bwd's out_lo
  auto out_lo = out2.select(0, 1);
  if (pad.v != Dv) out_lo = out_lo.narrow(-1, 0, Dv).contiguous();
  if (varlen) out_lo = out_lo.squeeze(0);
  return {out, lse, out_lo};
}

std::vector<torch::Tensor> flash_attn_bwd(
    torch::Tensor dout, torch::Tensor q, torch::Tensor k, torch::Tensor v,
    torch::Tensor out, torch::Tensor lse,
    c10::optional<torch::Tensor> cu_seqlens_q,
    c10::optional<torch::Tensor> cu_seqlens_k,
    bool causal, double softmax_scale, int64_t window_left, int64_t q_offset,
    c10::optional<torch::Tensor> dlse, c10::optional<torch::Tensor> out_lo) {
  const bool varlen = cu_seqlens_q.has_value();
  if (varlen) {
    if (out_lo.has_value()) out_lo = out_lo->unsqueeze(0);
    dout = dout.unsqueeze(0);
    q = q.unsqueeze(0);
    k = k.unsqueeze(0);
    v = v.unsqueeze(0);
    out = out.unsqueeze(0);
    lse = lse.unsqueeze(0);
  }
  const int B = q.size(0), Sq = q.size(1), Hq = q.size(2), D = q.size(3);
  const int Skv = k.size(1), Hkv = k.size(2), Dv = v.size(3);
  TORCH_CHECK(k.size(3) == D && out.size(3) == Dv && dout.size(3) == Dv,
              "flash_attn_bwd: k is as wide as q; out and dout as wide as v");
  const HeadDims pad = padded_head_dims(D, Dv);

  const VarlenMeta vl = prepare_varlen(cu_seqlens_q, cu_seqlens_k, d9d::kBwdKv,
                                       /*tile_kv=*/true, q.device());

  auto qp = maybe_pad_d(q, pad.qk);
  auto kp = maybe_pad_d(k, pad.qk);
  auto vp = maybe_pad_d(v, pad.v);
  auto dop = maybe_pad_d(dout, pad.v);
  auto op = maybe_pad_d(out, pad.v);

  auto f32opt = q.options().dtype(torch::kFloat32);
  auto delta = torch::empty({B, Hq, Sq}, f32opt);
  // atomicAdd accumulators: cleared via the copy/DMA engine (hipMemsetAsync)
  // instead of torch::zeros — the fill kernels measured ~1.7 TB/s in-step
  // and 400 MB/call of clears showed up at ~1.3% of the whole bench step.
  auto dq32 = torch::empty({B, Sq, Hq, pad.qk}, f32opt);
  auto dk32 = torch::empty({B, Skv, Hkv, pad.qk}, f32opt);
  auto dv32 = torch::empty({B, Skv, Hkv, pad.v}, f32opt);

  auto stream = at::hip::getCurrentHIPStream();
  hipMemsetAsync(dq32.data_ptr(), 0, dq32.numel() * sizeof(float), stream);
  hipMemsetAsync(dk32.data_ptr(), 0, dk32.numel() * sizeof(float), stream);
  hipMemsetAsync(dv32.data_ptr(), 0, dv32.numel() * sizeof(float), stream);
  if (out_lo.has_value()) {
    // O = out + out_lo (the wide forward's residual): delta as from an fp32 O
    TORCH_CHECK(out_lo->sizes() == out.sizes() && out_lo->is_cuda() &&
                    out_lo->scalar_type() == torch::kBFloat16,
                "flash_attn_bwd: out_lo must match out");
    auto olp = maybe_pad_d(*out_lo, pad.v);
    const int64_t rows = (int64_t)B * Sq * Hq;
    hipLaunchKernelGGL(d9d::attn_delta_lo_kernel, dim3(rows), dim3(64), 0, stream,
                       reinterpret_cast<const __bf16*>(dop.data_ptr()),
                       reinterpret_cast<const __bf16*>(op.data_ptr()),
                       reinterpret_cast<const __bf16*>(olp.data_ptr()),
                       delta.data_ptr<float>(), B, Sq, Hq, pad.v);
  } else {
    const int64_t rows = (int64_t)B * Sq * Hq;
    hipLaunchKernelGGL(d9d::attn_delta_kernel, dim3(rows), dim3(64), 0, stream,
                       reinterpret_cast<const __bf16*>(dop.data_ptr()),
                       reinterpret_cast<const __bf16*>(op.data_ptr()),
                       delta.data_ptr<float>(), B, Sq, Hq, pad.v);
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
  dispatch_head_dims(pad, [&](auto dqk, auto dv_c) {
    constexpr int DQK = decltype(dqk)::value, DV = decltype(dv_c)::value;
    constexpr int QR = DQK > 128 ? d9d::kBwdQWide : d9d::kBwdQ;
    constexpr size_t smem = d9d::bwd_smem_bytes<DQK, DV, QR>();
    static_assert(smem <= 160 * 1024, "over a workgroup's LDS");
    hipLaunchKernelGGL((d9d::flash_bwd_kernel<DQK, DV, QR>), grid,
                       dim3(d9d::kBwdThreads), smem, stream,
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
  if (D == pad.qk && Dv == pad.v) {
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
    dv = dv32.narrow(-1, 0, Dv).to(torch::kBFloat16).contiguous();
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
