// CDNA4 grouped GEMM for MoE expert compute.
//
// Replaces the reference's nv-grouped-gemm wheel (d9d/kernel/gmm/function.py).
// out[rows_e] = a[rows_e] @ b[e] for each expert e; row counts are ragged.
// Host builds tiny per-expert offset tables (row_offsets, m-tile prefix) from
// the CPU batch_sizes; ONE kernel launch covers every expert — each block
// binary-searches its m-tile, so there is no per-expert launch overhead
// (the eager fallback was E x 3 rocBLAS launches per MoE layer).
//
// Which kernel serves which call (B_ROWMAJOR_KN names the weight layout:
// false = (E, N, K) as nn.Linear stores it, true = (E, K, N)):
//
//   gmm_nt(a, w)  expert forward, w (E, N, K)
//     K % 32 == 0 && K >= 64             -> gmm_8phase_kernel<BN8, false>
//     otherwise, or D9D_GMM_8PHASE=0     -> gmm_staged_kernel<false>
//   gmm(a, b)     expert dgrad, b (E, K, N)
//     K % 32 == 0 && K >= 64 && N % 16 == 0
//                                        -> gmm_8phase_kernel<BN8, true>
//     otherwise, or D9D_GMM_NN_8PHASE=0  -> gmm_staged_kernel<true>
//   gmm_db(a, g)  expert wgrad, db (E, K, N)
//     K and N multiples of 8             -> gmm_db_8phase_kernel<BK8, BN8>
//     otherwise, or D9D_GMM_DB_8PHASE=0  -> gmm_db_kernel
//
// BN8 / BK8 are 256 or 192, chosen per call to waste the least padding.
// Every kernel runs 512 threads = 8 waves as 2 (row halves) x 4 (column
// quarters) on v_mfma_f32_16x16x32_bf16 with fp32 accumulators. The 8-phase
// kernels stage with global_load_lds behind counted vmcnt waits; the
// fallbacks stage through registers (T14) and take any K and N.
#include "common.h"
#include "mfma.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>

namespace d9d {

constexpr int kBM = 256;
constexpr int kBN = 192;
constexpr int kBK = 64;

// ---- helpers shared by the kernels below ------------------------------------

// One forward/dgrad work item: expert e, rows [row0, row_end) of its m-tile
// (row_end is the expert's end, so the tile may be partial), columns from n0.
struct WorkItem {
  int e, row0, row_end, n0;
};

D9D_DEVICE WorkItem locate_work(const int* __restrict__ row_off,
                                const int* __restrict__ mtile_pref,
                                int E, int n_tiles, int bn) {
  // Each XCD gets a contiguous span of expert-major work items, so one
  // expert's weight slice and A rows are re-read from that XCD's L2.
  const int wid = xcd_remap(blockIdx.x, gridDim.x);
  // work id -> (expert, m_tile) via binary search in the m-tile prefix
  const int mt_global = wid / n_tiles;
  int lo = 0, hi = E - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (mtile_pref[mid] <= mt_global) lo = mid; else hi = mid - 1;
  }
  const int e = lo;
  const int m_tile = mt_global - mtile_pref[e];
  return {e, row_off[e] + m_tile * kBM, row_off[e + 1], (wid % n_tiles) * bn};
}

// Store a wave's NI x NJ grid of 16x16 accumulator subtiles as bf16 into a
// row-major matrix with leading dimension ld: subtile (i, j) starts at
// (row0 + 16 i, col0 + 16 j); elements at or past row_end / col_end are
// dropped.
template <int NI, int NJ>
D9D_DEVICE void store_acc_tile(bf16_t* __restrict__ out, int ld,
                               const f32x4 (&acc)[NI][NJ], int row0,
                               int row_end, int col0, int col_end, int lane) {
#pragma unroll
  for (int i = 0; i < NI; ++i) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = row0 + i * 16 + (lane >> 4) * 4 + r;
        const int col = col0 + j * 16 + (lane & 15);
        if (row < row_end && col < col_end) {
          out[(int64_t)row * ld + col] = (bf16_t)acc[i][j][r];
        }
      }
    }
  }
}

// MFMA fragment (8 k-contiguous bf16 at column kk of `row`) from a
// [rows][kBK] LDS tile whose 16-byte units are XOR-swizzled by key & 7
// (key = row gives the plain conflict-free ds_read_b128 layout).
D9D_DEVICE bf16x8 lds_frag(const char* tile, int row, int kk, int key) {
  const int byte = (kk * 2) ^ ((key & 7) << 4);
  return *reinterpret_cast<const bf16x8*>(tile + row * (kBK * 2) + byte);
}

// MFMA fragment from a ROW-major operand staged as a [red/4][W/16][4][16]
// blocked image (red = reduction dim, W = tile width): reduction slice
// red0..red0+8 at the 16 columns of column block ct. ds_read_b64_tr_b16
// reads one 128-B [4 red][16 col] block transposed per 16-lane group; two
// reads make a fragment.
D9D_DEVICE bf16x8 tr16_frag(const char* img, int W, int red0, int ct, int lane) {
  const int rb0 = red0 >> 2;
  const char* blk0 =
      img + ((size_t)rb0 * (W / 16) + ct) * 128 + (lane & 15) * 8;
  const char* blk1 =
      img + ((size_t)(rb0 + 1) * (W / 16) + ct) * 128 + (lane & 15) * 8;
  bf16x4 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)(blk0));
  bf16x4 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
      (__attribute__((address_space(3))) bf16x4*)(blk1));
  bf16x8 f;
#pragma unroll
  for (int t = 0; t < 4; ++t) { f[t] = lo4[t]; f[4 + t] = hi4[t]; }
  return f;
}

// Async 16-byte global -> LDS copy (global_load_lds_dwordx4): no staging
// register, no ds_write; completion is counted by vmcnt. It cannot mask,
// so every source address must be in bounds.
D9D_DEVICE void glds16(const char* src, char* dst) {
  __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint32_t*>(src),
                                   reinterpret_cast<uint32_t*>(dst), 16, 0, 0);
}

// ---- register-staged forward/dgrad fallback (any K, any N) ------------------
//
// 256x192 tiles with 8 waves (2 m-halves x 4 n-quarters of 48): this kernel is
// HBM-bound on A re-reads (once per n-tile), and the big tile quarters that
// traffic vs the old 128x64 geometry. Register (T14) staging doubles as the
// second buffer: loads for k-tile t+1 issue early under tile t's MFMAs.
//
// A LDS tile: [kBM][kBK] row-major, rows kBK*2=128 bytes -> swizzle mask 7.
// B LDS tile: bt[n][k] (kBN x kBK): the MFMA B-fragment needs 8 contiguous k
// at fixed n. How B gets there depends on its storage layout (StagedB*).

// Branchless 8-element staging load from a row-major matrix: clamp the
// address into range, select after the load (a per-element branch around a
// load makes hipcc serialize every load behind a vmcnt(0) drain). Only a
// unit that crosses row_end / col_end takes the per-element fill (rare);
// that fill is what makes K % 8 != 0 and ragged N work.
// Keep the if/else shape: written as `if (ok) return val;` hipcc put a
// vmcnt(0) behind every vector load and both fallbacks ran at half speed.
D9D_DEVICE bf16x8 load8_edge(const bf16_t* __restrict__ base, int ld, int row,
                             int row_end, int col, int col_end) {
  const bool ok = row < row_end && col + 7 < col_end;
  const int64_t sr = min(row, row_end - 1);
  const int64_t sc = min(col, max(col_end - 8, 0));
  const bf16x8 val = *reinterpret_cast<const bf16x8*>(base + sr * ld + sc);
  bf16x8 out;
  if (ok) {
    out = val;
  } else {
    bf16x8 ev = {};
    if (row < row_end) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (col + j < col_end) ev[j] = base[(int64_t)row * ld + col + j];
      }
    }
    out = ev;
  }
  return out;
}

// B stored (E, N, K): k-contiguous like A, so it stages as plain vector
// copies into a row-major swizzled tile -- no scatter.
struct StagedBNK {
  bf16x8 reg[3];

  D9D_DEVICE void load(const bf16_t* __restrict__ w_e, int k0, int n0, int K,
                       int N) {
#pragma unroll
    for (int it = 0; it < 3; ++it) {
      const int idx = (threadIdx.x + it * 512) * 8;
      reg[it] = load8_edge(w_e, K, n0 + idx / kBK, N, k0 + idx % kBK, K);
    }
  }
  D9D_DEVICE void store(char* bt_lds) const {
#pragma unroll
    for (int it = 0; it < 3; ++it) {
      const int idx = (threadIdx.x + it * 512) * 8;
      const int n = idx / kBK;
      const int col = idx % kBK;
      const int byte = (col * 2) ^ ((swizzle_key(n) & 7) << 4);
      *reinterpret_cast<bf16x8*>(bt_lds + n * (kBK * 2) + byte) = reg[it];
    }
  }
  static D9D_DEVICE int swizzle_key(int n) { return n; }
};

// B stored (E, K, N): n-contiguous, so staging reads 8 consecutive n at
// fixed k and TRANSPOSES through registers. (kBK/2) x (kBN/8) = 768 k-pair
// groups; each group loads two bf16x8 (adjacent k, same 8 n) so the LDS
// writes pair into u32s.
struct StagedBKN {
  union bvec {
    bf16x8 v;
    ushort s[8];
  };
  bvec reg[2][2];

  D9D_DEVICE void load(const bf16_t* __restrict__ b_e, int k0, int n0, int K,
                       int N) {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int grp = threadIdx.x + it * 512;
      if (grp >= (kBK / 2) * (kBN / 8)) break;
      const int kk = (grp / (kBN / 8)) * 2;
      const int n = (grp % (kBN / 8)) * 8;
#pragma unroll
      for (int h = 0; h < 2; ++h)
        reg[it][h].v = load8_edge(b_e, N, k0 + kk + h, K, n0 + n, N);
    }
  }
  D9D_DEVICE void store(char* bt_lds) const {
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int grp = threadIdx.x + it * 512;
      if (grp >= (kBK / 2) * (kBN / 8)) break;
      const int kk = (grp / (kBN / 8)) * 2;
      const int n = (grp % (kBN / 8)) * 8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int nn = n + j;
        const uint32_t u = (uint32_t)reg[it][0].s[j] |
                           ((uint32_t)reg[it][1].s[j] << 16);
        const int byte = (kk * 2) ^ ((swizzle_key(nn) & 7) << 4);
        *reinterpret_cast<uint32_t*>(bt_lds + nn * (kBK * 2) + byte) = u;
      }
    }
  }
  // swizzle on (nn ^ nn>>3): the paired writes walk nn in +8 steps
  // inside one instruction (nn&7 alone is constant there -> 24-way
  // bank conflict, PMC-measured 21% of wave cycles); the reads walk
  // nn in +1 steps, and the combined mask spreads both 8 ways.
  static D9D_DEVICE int swizzle_key(int n) { return (n >> 3) ^ n; }
};

template <bool B_ROWMAJOR_KN>
__global__ __launch_bounds__(512, 1) void gmm_staged_kernel(
    const bf16_t* __restrict__ a,    // (T, K)
    const bf16_t* __restrict__ b,    // (E, K, N) if B_ROWMAJOR_KN else (E, N, K)
    bf16_t* __restrict__ out,        // (T, N)
    const int* __restrict__ row_off,      // (E+1,)
    const int* __restrict__ mtile_pref,   // (E+1,) prefix of ceil(rows_e/kBM)
    int E, int K, int N, int n_tiles) {
  using BStage = std::conditional_t<B_ROWMAJOR_KN, StagedBKN, StagedBNK>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* a_lds = smem;                     // [kBM][kBK]
  char* bt_lds = a_lds + kBM * kBK * 2;   // [kBN][kBK]

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 2;   // 0..1: wave row (128 rows each)
  const int wn = wave & 3;    // 0..3: wave col (48 cols each)

  const WorkItem wi = locate_work(row_off, mtile_pref, E, n_tiles, kBN);
  const bf16_t* b_e = b + (int64_t)wi.e * N * K;

  f32x4 acc[8][3];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  const int n_ktiles = (K + kBK - 1) / kBK;

  // T14 split staging: per k-tile, 4x bf16x8 of A and the registers of
  // BStage are loaded EARLY (issue overlaps the previous tile's MFMAs) and
  // written to LDS late.
  bf16x8 a_reg[4];
  BStage b_stage;

  auto load_regs = [&](int kt) {
    const int k0 = kt * kBK;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = (threadIdx.x + it * 512) * 8;
      a_reg[it] = load8_edge(a, K, wi.row0 + idx / kBK, wi.row_end,
                             k0 + idx % kBK, K);
    }
    b_stage.load(b_e, k0, wi.n0, K, N);
  };

  auto store_lds = [&]() {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = (threadIdx.x + it * 512) * 8;
      const int row = idx / kBK;
      const int col = idx % kBK;
      const int byte = (col * 2) ^ ((row & 7) << 4);
      *reinterpret_cast<bf16x8*>(a_lds + row * (kBK * 2) + byte) = a_reg[it];
    }
    b_stage.store(bt_lds);
  };

  load_regs(0);
  store_lds();
  __syncthreads();

  for (int kt = 0; kt < n_ktiles; ++kt) {
    if (kt + 1 < n_ktiles) load_regs(kt + 1);  // issue early, use late

    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {  // kBK=64 -> 2 MFMA k-steps
      const int kk = ks * 32 + (lane >> 4) * 8;
      bf16x8 a_frag[8], b_frag[3];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int row = wm * 128 + i * 16 + (lane & 15);
        a_frag[i] = lds_frag(a_lds, row, kk, row);
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int col = wn * 48 + j * 16 + (lane & 15);
        b_frag[j] = lds_frag(bt_lds, col, kk, BStage::swizzle_key(col));
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[i][j] = mfma16(a_frag[i], b_frag[j], acc[i][j]);
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    if (kt + 1 < n_ktiles) {
      store_lds();
      __syncthreads();
    }
  }

  store_acc_tile(out, N, acc, wi.row0 + wm * 128, wi.row_end,
                 wi.n0 + wn * 48, N, lane);
}

// ---- 8-phase forward/dgrad ---------------------------------------------------
//
// B operand of gmm_8phase_kernel, per storage layout. Each supplies the two
// things that depend on it: stage() issues one thread's glds of 8 KB chunk
// `chunk` of the k-tile starting at k0 into the slot's B region, and frag()
// reads the MFMA B-fragment for k offset kk at the 16 tile columns from col0.

// B stored (E, N, K): rows are k-contiguous like A's, so the B region is a
// [BN8][kBK] row-major tile with A's swizzle, produced by PRE-SWIZZLING the
// per-lane global source address (glds writes linearly: wave-uniform base +
// lane*16). A chunk is 64 rows.
template <int BN8>
struct Tile8BNK {
  static D9D_DEVICE void stage(const bf16_t* __restrict__ w_e, char* b_slot,
                               int k0, int n0, int K, int N, int chunk,
                               int wave, int lane) {
    const int l = wave * 1024 + lane * 16;
    const int nrow = chunk * 64 + (l >> 7);
    const int colb = (l & 127) ^ ((nrow & 7) << 4);
    const int64_t sn = min(n0 + nrow, N - 1);
    glds16(reinterpret_cast<const char*>(w_e) + (sn * (int64_t)K + k0) * 2 + colb,
           b_slot + chunk * (8 * 1024) + l);
  }
  static D9D_DEVICE bf16x8 frag(const char* b_slot, int kk, int col0, int lane) {
    const int col = col0 + (lane & 15);
    return lds_frag(b_slot, col, kk, col);
  }
};

// B stored (E, K, N), n-contiguous rows (dgrad: out = g @ w[e]): the MFMA
// fragment needs 8 reduction (k) elements at fixed n — a COLUMN of the
// row-major weight. glds cannot transpose, so B stages ROW-major into a
// [kBK/4][BN8/16][4][16] blocked image (16-byte units are 8 consecutive n at
// one k: still lane-linear, still coalesced) and fragments are read
// transposed (tr16_frag). Image element el: kb = el / (BN8*4), then
// nb = (el % (BN8*4)) / 64, krow = (el % 64) / 16, ncol = el % 16.
template <int BN8>
struct Tile8BKN {
  static D9D_DEVICE void stage(const bf16_t* __restrict__ w_e, char* b_slot,
                               int k0, int n0, int K, int N, int chunk,
                               int wave, int lane) {
    const int l = chunk * 8192 + wave * 1024 + lane * 16;  // byte offset
    const int el = l >> 1;                                  // bf16 element
    const int kb = el / (BN8 * 4);
    const int rem = el % (BN8 * 4);
    const int nb = rem >> 6;
    const int krow = (rem & 63) >> 4;
    const int ncol = rem & 15;   // 0 or 8 at 16-B granularity
    const int brow = k0 + kb * 4 + krow;
    const int64_t bcol = min((int64_t)(n0 + nb * 16 + ncol), (int64_t)N - 8);
    glds16(reinterpret_cast<const char*>(w_e) + ((int64_t)brow * N + bcol) * 2,
           b_slot + l);
  }
  static D9D_DEVICE bf16x8 frag(const char* b_slot, int kk, int col0, int lane) {
    return tr16_frag(b_slot, BN8, kk, col0 >> 4, lane);
  }
};

// 8-phase counted-vmcnt grouped GEMM (the guide's verified 256-wide template
// adapted to grouped ragged rows), templated on the n-tile width BN8
// (256 or 192 so the production shapes N=576/768/1536/2048 tile exactly)
// and on B's storage layout (Tile8BNK / Tile8BKN above).
// 256(M) x BN8(N) tile, BK=64, 8 waves as 2(M) x 4(N), per-wave
// 128 x BN8/4 output. LDS holds exactly TWO k-tiles
// (2 x (A 32KB + B BN8*128B)); staging is global_load_lds_dwordx4:
// A in 128-row halves (2 glds/thread), B in 8 KB chunks (1 glds/thread),
// issued inside the compute phases so 2-3 staging units stay in flight
// behind ONE counted s_waitcnt vmcnt(NJ) per k-tile (NJ = BN8/64).
// Each k-tile runs as 4 phases: phase p ds_reads the A fragments of
// C-quadrant p (i in {2p, 2p+1}; B fragments for the whole k-tile are read
// once at phase 0 and live in registers), stages its share of upcoming
// tiles, raw-barriers, and issues 4*NJ MFMAs. Raw s_barrier (NOT
// __syncthreads) keeps hipcc from draining the in-flight glds at each
// barrier.
// Death/arrival schedule (slot parity = kt & 1):
//   A(kt+1) goes to the OTHER slot whose tenant A(kt-1) is fully dead
//     -> staged at p0, p1 of kt (one half each)
//   B(kt) region (this slot) dies after phase 0 (all B frags read there)
//     -> B chunks of kt+2 staged at p1..p3
// Per-thread issue order makes the boundary wait vmcnt(NJ): the NJ
// outstanding loads are B chunks of kt+1; everything older has landed.
template <int BN8, bool B_ROWMAJOR_KN>
__global__ __launch_bounds__(512, 1) void gmm_8phase_kernel(
    const bf16_t* __restrict__ a,    // (T, K)
    const bf16_t* __restrict__ w,    // (E, K, N) if B_ROWMAJOR_KN else (E, N, K)
    bf16_t* __restrict__ out,        // (T, N)
    const int* __restrict__ row_off,
    const int* __restrict__ mtile_pref,
    int E, int K, int N, int n_tiles) {
  using BTile = std::conditional_t<B_ROWMAJOR_KN, Tile8BKN<BN8>, Tile8BNK<BN8>>;
  constexpr int NJ = BN8 / 64;             // B frags per wave = B chunks
  constexpr int SLOT = (256 + BN8) * 128;  // bytes per k-tile slot
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // slot s (s = kt & 1): A at smem + s*SLOT (32 KB), B right after
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 2;
  const int wn = wave & 3;

  const WorkItem wi = locate_work(row_off, mtile_pref, E, n_tiles, BN8);
  const bf16_t* w_e = w + (int64_t)wi.e * N * K;

  f32x4 acc[8][NJ];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // K % 64 == 32 tail: the last k-tile stages the OVERLAPPING window
  // [K-64, K) (all loads in bounds, no masking -- glds cannot mask) and the
  // MFMA phases run only its upper half (ks = 1), so columns [K-64, K-32)
  // are not double-counted. Host guarantees K % 32 == 0.
  const int n_ktiles = (K + kBK - 1) / kBK;
  const bool k_tail = (K % kBK) != 0;
  const int last_kt = n_ktiles - 1;

  auto ktile_k0 = [&](int kt) {
    return (k_tail && kt == last_kt) ? K - kBK : kt * kBK;
  };

  // A half (128 rows = 16 KB): 2 glds per thread.
  auto stage_a = [&](int kt, int half) {
    const int k0 = ktile_k0(kt);
    char* base = smem + (size_t)(kt & 1) * SLOT + half * (16 * 1024);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int chunk = wave + i * 8;           // 16 chunks of 1 KB
      const int l = chunk * 1024 + lane * 16;   // linear LDS byte in half
      const int arow = half * 128 + (l >> 7);   // tile row (128-B rows)
      const int colb = (l & 127) ^ ((arow & 7) << 4);  // source pre-swizzle
      const int64_t sr = min(wi.row0 + arow, wi.row_end - 1);
      glds16(reinterpret_cast<const char*>(a) + (sr * (int64_t)K + k0) * 2 + colb,
             base + l);
    }
  };
  auto stage_b = [&](int kt, int chunk) {
    BTile::stage(w_e, smem + (size_t)(kt & 1) * SLOT + (32 * 1024),
                 ktile_k0(kt), wi.n0, K, N, chunk, wave, lane);
  };

  // Fragment reads for C row subtile i / column subtile j at this lane's
  // k offset kk = ks * 32 + (lane >> 4) * 8 within the k-tile.
  auto a_frag_at = [&](const char* a_base, int i, int kk) {
    const int row = wm * 128 + i * 16 + (lane & 15);
    return lds_frag(a_base, row, kk, row);
  };
  auto b_frag_at = [&](const char* b_base, int j, int kk) {
    return BTile::frag(b_base, kk, wn * (BN8 / 4) + j * 16, lane);
  };

  // Prologue: issue order matches the steady-state boundary count.
#pragma unroll
  for (int c = 0; c < NJ; ++c) stage_b(0, c);
  stage_a(0, 0); stage_a(0, 1);
  if (n_ktiles > 1) {
#pragma unroll
    for (int c = 0; c < NJ; ++c) stage_b(1, c);
  }

  const int n_full = k_tail ? n_ktiles - 1 : n_ktiles;
  for (int kt = 0; kt < n_full; ++kt) {
    const char* a_base = smem + (size_t)(kt & 1) * SLOT;
    const char* b_base = a_base + 32 * 1024;

    // k-tile boundary: this tile's staging landed. In steady state the NJ
    // newer loads are B(kt+1); when B(kt+1) was NOT staged (last tile) the
    // newest outstanding loads are THIS tile's A halves — drain fully
    // (vmcnt(NJ) there let the final tile read in-flight A: rare flake
    // caught by the 12x race screen).
    if (kt + 1 < n_ktiles) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NJ) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();

    bf16x8 b_frag[NJ][2];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      // -- ds_read this phase's fragments ---------------------------------
      bf16x8 a_frag[2][2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int kk = ks * 32 + (lane >> 4) * 8;
#pragma unroll
        for (int il = 0; il < 2; ++il)
          a_frag[il][ks] = a_frag_at(a_base, 2 * p + il, kk);
        if (p == 0) {
#pragma unroll
          for (int j = 0; j < NJ; ++j) b_frag[j][ks] = b_frag_at(b_base, j, kk);
        }
      }
      // -- stage upcoming tiles into dead rows ----------------------------
      if (p == 0) {
        if (kt + 1 < n_ktiles) stage_a(kt + 1, 0);
      } else if (p == 1) {
        if (kt + 1 < n_ktiles) stage_a(kt + 1, 1);
        if (kt + 2 < n_ktiles) {
          stage_b(kt + 2, 0);
          if (NJ == 4) stage_b(kt + 2, 1);
        }
      } else if (p == 2) {
        if (kt + 2 < n_ktiles) {
          if (NJ == 4) { stage_b(kt + 2, 2); stage_b(kt + 2, 3); }
          else stage_b(kt + 2, 1);
        }
      } else {
        if (NJ == 3 && kt + 2 < n_ktiles) stage_b(kt + 2, 2);
      }
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int il = 0; il < 2; ++il)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            acc[2 * p + il][j] =
                mfma16(a_frag[il][ks], b_frag[j][ks], acc[2 * p + il][j]);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_s_barrier();
    }
  }

  // Peeled tail k-tile (K % 64 == 32): only its upper half (ks = 1)
  // contributes -- the staged window [K-64, K) overlaps the previous tile.
  // Nothing is staged any more, so the phases need no barriers.
  if (k_tail) {
    const char* a_base = smem + (size_t)(last_kt & 1) * SLOT;
    const char* b_base = a_base + 32 * 1024;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    bf16x8 b_frag_t[NJ];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      bf16x8 a_frag_t[2];
      const int kk = 32 + (lane >> 4) * 8;
#pragma unroll
      for (int il = 0; il < 2; ++il) a_frag_t[il] = a_frag_at(a_base, 2 * p + il, kk);
      if (p == 0) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) b_frag_t[j] = b_frag_at(b_base, j, kk);
      }
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int il = 0; il < 2; ++il)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
          acc[2 * p + il][j] =
              mfma16(a_frag_t[il], b_frag_t[j], acc[2 * p + il][j]);
      __builtin_amdgcn_s_setprio(0);
    }
  }

  store_acc_tile(out, N, acc, wi.row0 + wm * 128, wi.row_end,
                 wi.n0 + wn * (BN8 / 4), N, lane);
}

// ---- wgrad --------------------------------------------------------------------
//
// 8-phase glds + tr16 wgrad: db[e] = a[rows_e]^T @ g[rows_e], out (E, K, N).
// Same block mapping as gmm_db_kernel (expert-order round-robin over
// (e, k-tile, n-tile), ragged row loop in 64-row chunks) but the staging is
// the deep pipeline: BOTH operand chunks stage ROW-major via
// global_load_lds into [rows/4][cols/16][4][16] blocked images and BOTH
// MFMA fragments (reduction = rows) come from ds_read_b64_tr_b16 pairs.
// Rows past the expert's end read from a 16-byte zero buffer (glds cannot
// mask; a per-lane address select costs one v_cndmask, no branch), so pad
// rows contribute exact zeros to the row-sum.
//
// Templated on BOTH output tile dims (256 or 192): the wgrad's output is
// (K x N) and both can quantize badly — the bench's down-projection is
// K = 576 (2.25 tiles of 256 -> 33% wasted MFMA), its gate_up N = 1152
// (4.5 tiles). 192 divides both exactly. Phase count = BK8/64 (k subtiles
// walked two per phase), chunk counts scale with the image sizes, and the
// staging issue order (all a(rt+1) before any g(rt+2)) keeps the counted
// vmcnt waits exact.
template <int BK8, int BN8>
__global__ __launch_bounds__(512, 1) void gmm_db_8phase_kernel(
    const bf16_t* __restrict__ a,   // (T, K)
    const bf16_t* __restrict__ g,   // (T, N)
    bf16_t* __restrict__ db,        // (E, K, N)
    const int* __restrict__ row_off,
    const int* __restrict__ expert_order,
    const bf16_t* __restrict__ zero16,  // >= 8 zero bf16
    int E, int K, int N, int kt_tiles, int nt_tiles) {
  constexpr int KI = BK8 / 32;          // 16-wide k subtiles per wave
  constexpr int NJ = BN8 / 64;          // 16-wide n subtiles per wave
  constexpr int P = KI / 2;             // phases (2 k subtiles each)
  constexpr int ACH = BK8 / 64;         // 8 KB staging chunks per a tile
  constexpr int GCH = BN8 / 64;         // 8 KB staging chunks per g tile
  constexpr int ABYTES = 64 * BK8 * 2;  // blocked-image sizes
  constexpr int GBYTES = 64 * BN8 * 2;
  constexpr int SLOT = ABYTES + GBYTES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 2;  // k-half (BK8/2 rows of db)
  const int wn = wave & 3;   // n-quarter (BN8/4 cols)

  const int wid = blockIdx.x;
  const int tiles_per_e = kt_tiles * nt_tiles;
  const int e = expert_order[wid / tiles_per_e];
  const int k0 = ((wid % tiles_per_e) / nt_tiles) * BK8;
  const int n0 = (wid % nt_tiles) * BN8;
  const int r_start = row_off[e];
  const int r_end = row_off[e + 1];
  bf16_t* db_e = db + (int64_t)e * K * N;

  f32x4 acc[KI][NJ];
#pragma unroll
  for (int i = 0; i < KI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  if (r_start >= r_end) {
    // empty expert: this block zero-fills its tile (acc is still all zero)
    // so the host can hand us an EMPTY output (a torch::zeros prefill wrote
    // 2*K*N*E bytes per call — ~0.9 GB per wgrad at the bench shape, ~1.5%
    // of the whole step)
    store_acc_tile(db_e, N, acc, k0 + wm * (BK8 / 2), K,
                   n0 + wn * (BN8 / 4), N, lane);
    return;
  }

  const int n_rtiles = (r_end - r_start + 63) / 64;

  // Stage one 8 KB chunk of an operand tile (width W) for row tile rt:
  // 1 glds per thread. l = byte offset in the blocked image; the inverse
  // mapping recovers (row, col) for the source address.
  auto stage = [&](const bf16_t* src, int64_t stride, int c0, int cmax,
                   int rt, int chunk, int img_off, int W) {
    char* base = smem + (size_t)(rt & 1) * SLOT + img_off;
    const int l = chunk * 8192 + wave * 1024 + lane * 16;  // byte offset
    const int blk = l >> 7;                // 128-B [4][16] block index
    const int inb = l & 127;
    const int rb = blk / (W / 16);
    const int cb = blk % (W / 16);
    const int row = r_start + rt * 64 + rb * 4 + (inb >> 5);
    const int col8 = cb * 16 + (((inb >> 4) & 1) * 8);
    const int64_t col = min((int64_t)(c0 + col8), (int64_t)cmax - 8);
    const char* sp =
        (row < r_end)
            ? reinterpret_cast<const char*>(src) + (row * stride + col) * 2
            : reinterpret_cast<const char*>(zero16);
    glds16(sp, base + l);
  };
  auto stage_a = [&](int rt, int chunk) {
    stage(a, K, k0, K, rt, chunk, 0, BK8);
  };
  auto stage_g = [&](int rt, int chunk) {
    stage(g, N, n0, N, rt, chunk, ABYTES, BN8);
  };

  // Prologue mirrors the steady-state issue order (a before g).
#pragma unroll
  for (int c = 0; c < GCH; ++c) stage_g(0, c);
#pragma unroll
  for (int c = 0; c < ACH; ++c) stage_a(0, c);
  if (n_rtiles > 1) {
#pragma unroll
    for (int c = 0; c < GCH; ++c) stage_g(1, c);
  }

  for (int rt = 0; rt < n_rtiles; ++rt) {
    const char* a_img = smem + (size_t)(rt & 1) * SLOT;
    const char* g_img = a_img + ABYTES;

    if (rt + 1 < n_rtiles) {
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"(GCH) : "memory");
    } else {
      // no g(rt+1) staged: the newest outstanding loads are THIS row
      // tile's a chunks — drain fully
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();

    bf16x8 b_frag[NJ][2];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      bf16x8 a_frag[2][2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int red0 = ks * 32 + (lane >> 4) * 8;
#pragma unroll
        for (int il = 0; il < 2; ++il) {
          const int kct = (wm * (BK8 / 2) + (2 * p + il) * 16) >> 4;
          a_frag[il][ks] = tr16_frag(a_img, BK8, red0, kct, lane);
        }
        if (p == 0) {
#pragma unroll
          for (int j = 0; j < NJ; ++j) {
            const int nct = (wn * (BN8 / 4) + j * 16) >> 4;
            b_frag[j][ks] = tr16_frag(g_img, BN8, red0, nct, lane);
          }
        }
      }
      // Stage a(rt+1) then g(rt+2), spread evenly over the phases; a fully
      // before g keeps the top-of-iteration vmcnt(GCH) count exact.
      {
        constexpr int TOT = ACH + GCH;
        constexpr int PER = (TOT + P - 1) / P;
#pragma unroll
        for (int s = p * PER; s < (p + 1) * PER && s < TOT; ++s) {
          if (s < ACH) {
            if (rt + 1 < n_rtiles) stage_a(rt + 1, s);
          } else {
            if (rt + 2 < n_rtiles) stage_g(rt + 2, s - ACH);
          }
        }
      }
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int il = 0; il < 2; ++il)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            acc[2 * p + il][j] =
                mfma16(a_frag[il][ks], b_frag[j][ks], acc[2 * p + il][j]);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_s_barrier();
    }
  }

  store_acc_tile(db_e, N, acc, k0 + wm * (BK8 / 2), K, n0 + wn * (BN8 / 4), N,
                 lane);
}

// db[e] = a[rows_e]^T @ g[rows_e]: out (E, K, N).
// Grid (ceil(N/256), ceil(K/256), E): 256x256 tiles per workgroup -- 8 waves
// as 2 (k-halves of 128) x 4 (n-quarters of 64) -- looping the expert's rows
// in chunks of 64. Both operands are staged transposed ([dim][row], 128-byte
// LDS rows, XOR swizzle) for k-contiguous fragments. The big tile is what
// matters here: this kernel is HBM-bound on re-reads (a is read once per
// n-tile, g once per k-tile), and 256x256 halves that traffic vs 128x128.
__global__ __launch_bounds__(512, 1) void gmm_db_kernel(
    const bf16_t* __restrict__ a,   // (T, K)
    const bf16_t* __restrict__ g,   // (T, N)
    bf16_t* __restrict__ db,        // (E, K, N)
    const int* __restrict__ row_off,
    const int* __restrict__ expert_order,  // experts sorted by row count desc
    int E, int K, int N, int kt_tiles, int nt_tiles) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* at_lds = reinterpret_cast<bf16_t*>(smem);   // [256 k][64 rows]
  bf16_t* gt_lds = at_lds + 256 * 64;                 // [256 n][64 rows]

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int wm = wave >> 2;  // k-half (128 rows of db)
  const int wn = wave & 3;   // n-quarter (64 cols)

  // NO XCD grouping here (unlike locate_work): per-tile work scales with
  // the expert's row count, and giving one XCD a contiguous expert-major
  // span concentrates the heavy (sorted-first) experts on it -- measured as
  // an 8-XCD straggler that cost ~15% end-to-end. Round-robin dispatch
  // balances the ragged loop lengths instead. Heavy experts dispatch first
  // so the tail wave holds the small tiles.
  const int wid = blockIdx.x;
  const int tiles_per_e = kt_tiles * nt_tiles;
  const int e = expert_order[wid / tiles_per_e];
  const int k0 = ((wid % tiles_per_e) / nt_tiles) * 256;
  const int n0 = (wid % nt_tiles) * 256;
  const int r_start = row_off[e];
  const int r_end = row_off[e + 1];
  if (r_start >= r_end) return;  // empty expert: db stays zero (host zeros it)

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  // T14 staging: each thread owns 4 (4-row x 2-col) blocks per tensor, loaded
  // into registers early (overlapping the previous chunk's MFMAs) with
  // branchless clamped addresses, transposed into LDS with 8-byte writes
  // late. Rows past r_end are zero-filled (they enter the row-sum).
  bf16x4_bits a_c0[4], a_c1[4], g_c0[4], g_c1[4];

  auto load_regs = [&](int rt) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = threadIdx.x + it * 512;
      const int d0 = (idx & 127) * 2;
      const int rb = (idx >> 7) * 4;
      const bool k_ok = k0 + d0 + 1 < K;
      const bool n_ok = n0 + d0 + 1 < N;
      const int64_t sk = min((int64_t)(k0 + d0), (int64_t)max(K - 2, 0));
      const int64_t sn = min((int64_t)(n0 + d0), (int64_t)max(N - 2, 0));
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int g_row = rt + rb + i;
        const bool row_ok = g_row < r_end;
        const int64_t sr = min((int64_t)g_row, (int64_t)max(r_end - 1, 0));
        const uint32_t pa = *reinterpret_cast<const uint32_t*>(a + sr * K + sk);
        const uint32_t pg = *reinterpret_cast<const uint32_t*>(g + sr * N + sn);
        const uint32_t va = (row_ok && k_ok) ? pa : 0u;
        const uint32_t vg = (row_ok && n_ok) ? pg : 0u;
        a_c0[it].s[i] = (ushort)(va & 0xffffu);
        a_c1[it].s[i] = (ushort)(va >> 16);
        g_c0[it].s[i] = (ushort)(vg & 0xffffu);
        g_c1[it].s[i] = (ushort)(vg >> 16);
      }
    }
  };

  auto store_lds = [&]() {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = threadIdx.x + it * 512;
      const int d0 = (idx & 127) * 2;
      const int rb = (idx >> 7) * 4;
      const int byte0 = (rb * 2) ^ ((d0 & 7) << 4);
      const int byte1 = (rb * 2) ^ (((d0 + 1) & 7) << 4);
      *reinterpret_cast<uint64_t*>(
          reinterpret_cast<char*>(at_lds) + d0 * 128 + byte0) = a_c0[it].u;
      *reinterpret_cast<uint64_t*>(
          reinterpret_cast<char*>(at_lds) + (d0 + 1) * 128 + byte1) = a_c1[it].u;
      *reinterpret_cast<uint64_t*>(
          reinterpret_cast<char*>(gt_lds) + d0 * 128 + byte0) = g_c0[it].u;
      *reinterpret_cast<uint64_t*>(
          reinterpret_cast<char*>(gt_lds) + (d0 + 1) * 128 + byte1) = g_c1[it].u;
    }
  };

  load_regs(r_start);
  store_lds();
  __syncthreads();

  for (int rt = r_start; rt < r_end; rt += 64) {
    if (rt + 64 < r_end) load_regs(rt + 64);  // issue early

    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {  // 64 rows -> 2 k-steps
      const int rr = ks * 32 + (lane >> 4) * 8;
      bf16x8 a_frag[8], g_frag[4];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int krow = wm * 128 + i * 16 + (lane & 15);
        const int byte = (rr * 2) ^ ((krow & 7) << 4);
        a_frag[i] = *reinterpret_cast<const bf16x8*>(
            reinterpret_cast<const char*>(at_lds) + krow * (64 * 2) + byte);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ncol = wn * 64 + j * 16 + (lane & 15);
        const int byte = (rr * 2) ^ ((ncol & 7) << 4);
        g_frag[j] = *reinterpret_cast<const bf16x8*>(
            reinterpret_cast<const char*>(gt_lds) + ncol * (64 * 2) + byte);
      }
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(a_frag[i], g_frag[j], acc[i][j]);
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    if (rt + 64 < r_end) {
      store_lds();
      __syncthreads();
    }
  }

  store_acc_tile(db + (int64_t)e * K * N, N, acc, k0 + wm * 128, K,
                 n0 + wn * 64, N, lane);
}

}  // namespace d9d

// ---------------------------------------------------------------------------

// E == 1 (dense KernelLinear) offsets depend only on the row count: cache
// the device tensors so the hot path pays no per-call CPU alloc + H2D
// (the round-1 measured overhead that cancelled the kernel's 600-vs-260
// TF/s win at bench scale). MoE sizes change per routing step: no cache.
static std::map<std::tuple<int64_t, int, int>,
                std::tuple<torch::Tensor, torch::Tensor, int>> g_e1_offsets;
static std::mutex g_e1_offsets_mu;

static std::tuple<torch::Tensor, torch::Tensor, int> build_offsets(
    torch::Tensor batch_sizes, torch::Device device, int tile_m) {
  const int E = batch_sizes.numel();
  if (E == 1) {
    const int64_t rows = batch_sizes.to(torch::kInt64).item<int64_t>();
    const auto key = std::make_tuple(rows, tile_m, (int)device.index());
    std::lock_guard<std::mutex> lock(g_e1_offsets_mu);
    auto it = g_e1_offsets.find(key);
    if (it != g_e1_offsets.end()) return it->second;
    auto ro = torch::tensor({(int)0, (int)rows},
                            torch::dtype(torch::kInt32)).to(device);
    const int tiles = (int)((rows + tile_m - 1) / tile_m);
    auto mp = torch::tensor({0, tiles}, torch::dtype(torch::kInt32)).to(device);
    auto val = std::make_tuple(ro, mp, tiles);
    g_e1_offsets.emplace(key, val);
    return val;
  }
  auto row_off = torch::empty({E + 1}, torch::dtype(torch::kInt32));
  auto mtile_pref = torch::empty({E + 1}, torch::dtype(torch::kInt32));
  auto bs = batch_sizes.to(torch::kInt64);
  const int64_t* p = bs.data_ptr<int64_t>();
  int32_t* ro = row_off.data_ptr<int32_t>();
  int32_t* mp = mtile_pref.data_ptr<int32_t>();
  int rows = 0, tiles = 0;
  for (int e = 0; e < E; ++e) {
    ro[e] = rows;
    mp[e] = tiles;
    rows += (int)p[e];
    tiles += (int)((p[e] + tile_m - 1) / tile_m);
  }
  ro[E] = rows;
  mp[E] = tiles;
  // total tile count returned from the CPU copy: reading it from the device
  // tensor (`mtile_pref[E].item()`) is a D2H sync on EVERY call, which
  // serializes the launch pipeline (measured ~0.5 ms/call end-to-end).
  return {row_off.to(device, /*non_blocking=*/true),
          mtile_pref.to(device, /*non_blocking=*/true), tiles};
}

// The D9D_GMM_*_8PHASE switches are opt-outs: on unless set to "0...".
static bool env_not_zero(const char* name) {
  const char* v = getenv(name);
  return v == nullptr || v[0] != '0';
}

// Tensors of one forward/dgrad call: out (T, N) = a (T, K) x b[e], with b
// (E, K, N) or (E, N, K) as the kernel's layout parameter says.
struct ForwardArgs {
  torch::Tensor a, b, out, row_off, mtile_pref;
  int total_mtiles;
};

// Launch `kernel` with one block per (m-tile, bn-wide n-tile) work item.
template <typename Kernel>
static void launch_forward(Kernel kernel, int bn, size_t smem,
                           const ForwardArgs& f) {
  const int E = f.b.size(0), K = f.a.size(1), N = f.out.size(1);
  const int n_tiles = (N + bn - 1) / bn;
  hipLaunchKernelGGL(kernel, dim3(n_tiles * f.total_mtiles), dim3(512), smem,
                     at::hip::getCurrentHIPStream(),
                     reinterpret_cast<const __bf16*>(f.a.data_ptr()),
                     reinterpret_cast<const __bf16*>(f.b.data_ptr()),
                     reinterpret_cast<__bf16*>(f.out.data_ptr()),
                     f.row_off.data_ptr<int>(), f.mtile_pref.data_ptr<int>(),
                     E, K, N, n_tiles);
}

template <bool B_ROWMAJOR_KN>
static void launch_8phase(const ForwardArgs& f) {
  // pick the n-tile with the least padded waste. Production shapes:
  // 576 -> 192 exact (654 vs 552 TF/s), 768 -> both exact, 1536/2048 -> 256.
  // Ties -> 256 (measured: 729 vs 655 TF/s at N=768, 807 vs 742 at 1536).
  const int N = f.out.size(1);
  const int pad256 = ((N + 255) / 256) * 256 - N;
  const int pad192 = ((N + 191) / 192) * 192 - N;
  constexpr size_t smem256 = (size_t)2 * (256 + 256) * 128;  // two k-tile slots
  constexpr size_t smem192 = (size_t)2 * (256 + 192) * 128;
  static const bool attr_set = []() {
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(&d9d::gmm_8phase_kernel<256, B_ROWMAJOR_KN>),
        hipFuncAttributeMaxDynamicSharedMemorySize, smem256);
    (void)hipFuncSetAttribute(
        reinterpret_cast<const void*>(&d9d::gmm_8phase_kernel<192, B_ROWMAJOR_KN>),
        hipFuncAttributeMaxDynamicSharedMemorySize, smem192);
    return true;
  }();
  (void)attr_set;
  if (pad256 <= pad192) {
    launch_forward(d9d::gmm_8phase_kernel<256, B_ROWMAJOR_KN>, 256, smem256, f);
  } else {
    launch_forward(d9d::gmm_8phase_kernel<192, B_ROWMAJOR_KN>, 192, smem192, f);
  }
}

template <bool B_ROWMAJOR_KN>
static void launch_staged(const ForwardArgs& f) {
  const size_t smem = (d9d::kBM * d9d::kBK + d9d::kBN * d9d::kBK) * sizeof(__bf16);
  launch_forward(d9d::gmm_staged_kernel<B_ROWMAJOR_KN>, d9d::kBN, smem, f);
}

torch::Tensor gmm(torch::Tensor a, torch::Tensor b, torch::Tensor batch_sizes) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == torch::kBFloat16 && a.is_contiguous());
  TORCH_CHECK(b.is_cuda() && b.scalar_type() == torch::kBFloat16 && b.is_contiguous());
  TORCH_CHECK(batch_sizes.device().is_cpu());
  const int T = a.size(0), K = a.size(1);
  const int N = b.size(2);
  TORCH_CHECK(b.size(1) == K, "gmm K mismatch");

  auto out = torch::empty({(int64_t)T, (int64_t)N}, a.options());
  if (T == 0) return out;
  auto [row_off, mtile_pref, total_mtiles] =
      build_offsets(batch_sizes, a.device(), d9d::kBM);
  if (total_mtiles == 0) return out;
  const ForwardArgs f{a, b, out, row_off, mtile_pref, total_mtiles};

  static const bool use_nn8 = env_not_zero("D9D_GMM_NN_8PHASE");
  if (use_nn8 && K % 32 == 0 && K >= 64 && N % 16 == 0) {
    launch_8phase<true>(f);
  } else {
    launch_staged<true>(f);
  }
  return out;
}

torch::Tensor gmm_nt(torch::Tensor a, torch::Tensor w, torch::Tensor batch_sizes) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == torch::kBFloat16 && a.is_contiguous());
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16 && w.is_contiguous());
  TORCH_CHECK(batch_sizes.device().is_cpu());
  const int T = a.size(0), K = a.size(1);
  const int N = w.size(1);
  TORCH_CHECK(w.size(2) == K, "gmm_nt K mismatch");

  auto out = torch::empty({(int64_t)T, (int64_t)N}, a.options());
  if (T == 0) return out;
  auto [row_off, mtile_pref, total_mtiles] =
      build_offsets(batch_sizes, a.device(), d9d::kBM);
  if (total_mtiles == 0) return out;
  const ForwardArgs f{a, w, out, row_off, mtile_pref, total_mtiles};

  static const bool use_8phase = env_not_zero("D9D_GMM_8PHASE");
  if (use_8phase && K % 32 == 0 && K >= 64) {
    launch_8phase<false>(f);
  } else {
    launch_staged<false>(f);
  }
  return out;
}

torch::Tensor gmm_db(torch::Tensor a, torch::Tensor g, torch::Tensor batch_sizes,
                     int64_t num_experts) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == torch::kBFloat16 && a.is_contiguous());
  TORCH_CHECK(g.is_cuda() && g.scalar_type() == torch::kBFloat16 && g.is_contiguous());
  const int K = a.size(1), N = g.size(1);
  const int E = (int)num_experts;

  // empty (not zeros): the 8-phase kernel covers every tile, including
  // zero-filling empty experts' tiles; only the legacy fallback needs the
  // prefill (it early-returns on empty experts)
  auto db = torch::empty({(int64_t)E, (int64_t)K, (int64_t)N}, a.options());
  if (a.size(0) == 0) return db;
  auto [row_off, mtile_pref, total_mtiles_unused] =
      build_offsets(batch_sizes, a.device(), d9d::kBM);
  (void)total_mtiles_unused;
  auto order_cpu = torch::argsort(batch_sizes.to(torch::kInt64), /*dim=*/0,
                                  /*descending=*/true).to(torch::kInt32);
  auto expert_order = order_cpu.to(a.device(), /*non_blocking=*/true);

  // wgrad tile choice: prefer the width that divides the dim exactly
  // (the bench's down-projection K = 576 loses 33% of its MFMA to a
  // 256-tile ceiling; 192 divides it exactly — likewise N = 1152)
  const int BK = (K % 256 != 0 && K % 192 == 0) ? 192 : 256;
  const int BN = (N % 256 != 0 && N % 192 == 0) ? 192 : 256;
  const int nt_tiles = (N + BN - 1) / BN, kt_tiles = (K + BK - 1) / BK;
  const dim3 grid(nt_tiles * kt_tiles * E);
  auto stream = at::hip::getCurrentHIPStream();

  // K/N must be multiples of 8: a 16-byte staging unit must never straddle
  // the tensor edge (the clamp would shift VALID columns' data — caught by
  // the ragged K=100 parity case).
  static const bool use_db8 = env_not_zero("D9D_GMM_DB_8PHASE");
  if (use_db8 && K >= 8 && N >= 8 && K % 8 == 0 && N % 8 == 0) {
    // cached 16-byte zero source for ragged row tails (glds cannot mask)
    static std::map<int, torch::Tensor> zeros_by_dev;
    torch::Tensor z;
    {
      std::lock_guard<std::mutex> lock(g_e1_offsets_mu);
      auto it = zeros_by_dev.find((int)a.device().index());
      if (it == zeros_by_dev.end()) {
        z = torch::zeros({8}, a.options());
        zeros_by_dev.emplace((int)a.device().index(), z);
      } else {
        z = it->second;
      }
    }
    static bool attr_set_db = false;
    if (!attr_set_db) {
#define DB_ATTR(BK8, BN8)                                                     \
      hipFuncSetAttribute(                                                    \
          reinterpret_cast<const void*>(                                      \
              &d9d::gmm_db_8phase_kernel<BK8, BN8>),                          \
          hipFuncAttributeMaxDynamicSharedMemorySize,                         \
          2 * 64 * (BK8 + BN8) * 2)
      DB_ATTR(256, 256); DB_ATTR(256, 192); DB_ATTR(192, 256); DB_ATTR(192, 192);
#undef DB_ATTR
      attr_set_db = true;
    }
#define DB_LAUNCH(BK8, BN8)                                                   \
    hipLaunchKernelGGL((d9d::gmm_db_8phase_kernel<BK8, BN8>), grid,           \
                       dim3(512), 2 * 64 * (BK8 + BN8) * 2, stream,           \
                       reinterpret_cast<const __bf16*>(a.data_ptr()),         \
                       reinterpret_cast<const __bf16*>(g.data_ptr()),         \
                       reinterpret_cast<__bf16*>(db.data_ptr()),              \
                       row_off.data_ptr<int>(), expert_order.data_ptr<int>(), \
                       reinterpret_cast<const __bf16*>(z.data_ptr()),         \
                       E, K, N, kt_tiles, nt_tiles)
    if (BK == 256 && BN == 256) DB_LAUNCH(256, 256);
    else if (BK == 256) DB_LAUNCH(256, 192);
    else if (BN == 256) DB_LAUNCH(192, 256);
    else DB_LAUNCH(192, 192);
#undef DB_LAUNCH
    return db;
  }

  db.zero_();  // legacy kernel early-returns on empty experts
  const int nt256 = (N + 255) / 256, kt256 = (K + 255) / 256;
  const dim3 grid256(nt256 * kt256 * E);
  const size_t smem = (2 * 256 * 64) * sizeof(__bf16);
  hipLaunchKernelGGL(d9d::gmm_db_kernel, grid256, dim3(512), smem, stream,
                     reinterpret_cast<const __bf16*>(a.data_ptr()),
                     reinterpret_cast<const __bf16*>(g.data_ptr()),
                     reinterpret_cast<__bf16*>(db.data_ptr()),
                     row_off.data_ptr<int>(), expert_order.data_ptr<int>(),
                     E, K, N, kt256, nt256);
  return db;
}
