// LDS tile vocabulary of the 8-phase kernels (gmm.hip, cce.hip): a k-tile is
// kBK = 64 bf16 wide, staged with global_load_lds into [rows][kBK] row-major
// tiles whose 16-byte units are XOR-swizzled, and read back as MFMA fragments.
#pragma once

#include "mfma.h"

namespace d9d {

constexpr int kBK = 64;

// MFMA fragment (8 k-contiguous bf16 at column kk of `row`) from a
// [rows][kBK] LDS tile whose 16-byte units are XOR-swizzled by key & 7
// (key = row gives the plain conflict-free ds_read_b128 layout).
D9D_DEVICE bf16x8 lds_frag(const char* tile, int row, int kk, int key) {
  const int byte = (kk * 2) ^ ((key & 7) << 4);
  return *reinterpret_cast<const bf16x8*>(tile + row * (kBK * 2) + byte);
}

// Async 16-byte global -> LDS copy (global_load_lds_dwordx4): no staging
// register, no ds_write; completion is counted by vmcnt. It cannot mask,
// so every source address must be in bounds.
D9D_DEVICE void glds16(const char* src, char* dst) {
  __builtin_amdgcn_global_load_lds(reinterpret_cast<const uint32_t*>(src),
                                   reinterpret_cast<uint32_t*>(dst), 16, 0, 0);
}

// B stored (E, N, K): rows are k-contiguous like A's, so the B region is a
// [BN8][kBK] row-major tile with A's swizzle, produced by PRE-SWIZZLING the
// per-lane global source address (glds writes linearly: wave-uniform base +
// lane*16). stage() issues one thread's glds of 8 KB chunk `chunk`
// (64 rows) of the k-tile starting at k0 into the slot's B region; frag()
// reads the MFMA B-fragment for k offset kk at the 16 tile columns from col0.
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

}  // namespace d9d
