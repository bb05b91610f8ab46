// bf16 MFMA vocabulary shared by the matrix-core kernels (attention, gmm,
// gdn, cce): fragment types, the MFMA they all use, bf16 bit packing.
#pragma once

#include "common.h"

namespace d9d {

typedef __bf16 bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// Fragment maps for v_mfma_f32_16x16x32_bf16 (M=N=16, K=32):
//   A[m][k]: lane l holds m = l&15, k = (l>>4)*8 + j   (j = 0..7)
//   B[k][n]: lane l holds n = l&15, k = (l>>4)*8 + j
//   C[m][n]: lane l, reg r: m = (l>>4)*4 + r, n = l&15
// (verified on-device by attention.hip's mfma_selfcheck).
D9D_DEVICE f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

D9D_DEVICE ushort bf16_bits(bf16_t v) {
  union { bf16_t b; ushort u; } cv;
  cv.b = v;
  return cv.u;
}

union bf16x4_bits {  // 4 bf16 lanes packed for one 8-byte LDS/global store
  uint64_t u;
  ushort s[4];
};

}  // namespace d9d
