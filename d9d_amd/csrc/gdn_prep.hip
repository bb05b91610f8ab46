// GatedDeltaNet prologue for CDNA4 (gfx950): everything the block does between
// its short convs / gate projections and the chunk kernels of gdn.hip, one
// pass each way.
//
//   forward   q, k (B,S,Hkv,Dk) bf16  -> qn, kn (B,H,S,Dk) bf16: per-row L2
//                                        normalisation, x / max(|x|, 1e-12),
//                                        the row of qk head h / rep written to
//                                        all rep = H / Hkv value heads
//             v (B,S,H,Dv) bf16       -> vt (B,H,S,Dv) bf16, a copy
//             b_raw, a_raw (B,S,H)    -> beta = sigmoid(b_raw), g (B,H,S) fp32
//                                        g = logsigmoid(a_raw), or the Mamba
//                                        gate -exp(A_log[h]) softplus(a_raw +
//                                        dt_bias[h])
//   backward  the mirror image: fp32 gradients in the output layouts come
//             back as bf16 gradients in the input layouts; the rep incoming
//             rows of a qk head are summed BEFORE the normalisation's
//             projection, in fp32; dA_log / ddt_bias are folded in a fixed
//             order (per-block partials, then a second tiny kernel), so two
//             launches return the same bits.
//
// Work split. One workgroup of 4 waves owns (b, a 64-token tile, a role):
// role 0 / 1 walk the qk heads of q / k, role 2 the value heads of v, role 3
// the two gates. The roles are separate workgroups, not phases of one: the
// rows are short (a head's row is 128 or 256 contiguous bytes in both
// layouts), each thread has only a few 16-byte loads in flight, and four
// times the workgroups is what keeps the memory system busy.
//
// Data movement. q, k, v never touch LDS: D/8 lanes own a row with 16-byte
// accesses (8 lanes at D = 64, 16 at 128), so a wave holds 8 or 4 rows and the
// sum of squares is one xor-shuffle cascade inside the lane group (the
// head-norm kernels of rms_norm.hip do the same). Every thread works on
// kRowsInFlight independent rows at a time. beta and g are a true transpose at
// 2-4 byte granularity: a slab of up to 32 heads x 64 tokens goes through an
// LDS image with rows padded to 65 floats, so the (B,S,H) side is accessed
// along h and the (B,H,S) side along s, both coalesced and bank-conflict free.
#include "common.h"

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace d9d {

constexpr int kPrepBlock = 256;
constexpr int kPrepTile = 64;        // tokens per workgroup
constexpr int kPrepSlab = 32;        // heads per LDS gate image
constexpr int kPrepPad = kPrepTile + 1;
constexpr int kRowsInFlight = 2;     // independent rows per thread
constexpr float kPrepEps = 1e-12f;   // F.normalize's clamp

struct PrepShape {
  int64_t S;
  int H, Hkv, rep, tiles;
};

D9D_DEVICE void load8(const ushort* p, float (&x)[8]) {
  Bf16x8 b;
  b.u = *reinterpret_cast<const ushort8v*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = bf16_bits_to_f32(b.s[j]);
}

D9D_DEVICE void load8(const float* p, float (&x)[8]) {
  const float4v a = *reinterpret_cast<const float4v*>(p);
  const float4v b = *reinterpret_cast<const float4v*>(p + 4);
#pragma unroll
  for (int j = 0; j < 4; ++j) { x[j] = a[j]; x[4 + j] = b[j]; }
}

D9D_DEVICE void store8(ushort* p, const float (&x)[8]) {
  Bf16x8 b;
#pragma unroll
  for (int j = 0; j < 8; ++j) b.s[j] = f32_to_bf16_rne(x[j]);
  *reinterpret_cast<ushort8v*>(p) = b.u;
}

// sum over the LANES lanes that share a row (LANES = 8 or 16, aligned)
template <int LANES>
D9D_DEVICE float row_sum(float v) {
#pragma unroll
  for (int off = 1; off < LANES; off <<= 1) v += __shfl_xor(v, off, kWaveSize);
  return v;
}

// e = exp(-|x|) serves sigmoid, log-sigmoid and softplus without overflow
D9D_DEVICE float sigmoid_f(float x) {
  const float e = expf(-fabsf(x));
  return (x >= 0.f ? 1.f : e) / (1.f + e);
}
D9D_DEVICE float softplus_f(float x) {
  return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
}

// ---- forward ----------------------------------------------------------------

// rows of one tile: (token, head) -> D contiguous elements at
// src[((b*S + s)*heads + head)*D]; NORM selects q/k (normalise, write `rep`
// heads) or v (copy, rep = 1).
template <int D, bool NORM>
D9D_DEVICE void prep_rows_fwd(const ushort* __restrict__ src,
                              ushort* __restrict__ dst, int64_t b, int64_t s0,
                              int64_t S, int heads, int rep) {
  constexpr int LANES = D / 8;
  constexpr int ROWS = kPrepBlock / LANES;       // rows per pass
  const int l = threadIdx.x % LANES;
  const int r0 = threadIdx.x / LANES;
  const int H = heads * rep;
  // kPrepTile * heads is a multiple of ROWS * kRowsInFlight (64): every
  // thread makes the same number of trips, the shuffles see whole groups
  for (int base = 0; base < kPrepTile * heads; base += ROWS * kRowsInFlight) {
    float x[kRowsInFlight][8];
    int64_t s[kRowsInFlight];
    int hd[kRowsInFlight];
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
      const int row = base + u * ROWS + r0;
      hd[u] = row / kPrepTile;
      s[u] = s0 + row % kPrepTile;
      // the tail tile reads its last valid token again and stores nothing
      const int64_t tok = s[u] < S ? s[u] : S - 1;
      load8(src + ((b * S + tok) * heads + hd[u]) * D + l * 8, x[u]);
    }
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
      if constexpr (NORM) {
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += x[u][j] * x[u][j];
        ss = row_sum<LANES>(ss);
        const float r = 1.f / fmaxf(sqrtf(ss), kPrepEps);
#pragma unroll
        for (int j = 0; j < 8; ++j) x[u][j] *= r;
      }
      if (s[u] < S) {
        Bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o.s[j] = f32_to_bf16_rne(x[u][j]);
        for (int c = 0; c < rep; ++c) {
          const int64_t h = (int64_t)hd[u] * rep + c;
          *reinterpret_cast<ushort8v*>(
              dst + ((b * H + h) * S + s[u]) * D + l * 8) = o.u;
        }
      }
    }
  }
}

template <int DK, int DV, bool MAMBA>
__global__ __launch_bounds__(kPrepBlock) void gdn_prep_fwd_kernel(
    const ushort* __restrict__ q, const ushort* __restrict__ k,
    const ushort* __restrict__ v, const ushort* __restrict__ b_raw,
    const ushort* __restrict__ a_raw, const float* __restrict__ A_log,
    const float* __restrict__ dt_bias, ushort* __restrict__ qn,
    ushort* __restrict__ kn, ushort* __restrict__ vt, float* __restrict__ beta,
    float* __restrict__ g, PrepShape p) {
  __shared__ float img[2][kPrepSlab * kPrepPad];
  const int64_t b = blockIdx.x / p.tiles;
  const int64_t s0 = (int64_t)(blockIdx.x % p.tiles) * kPrepTile;
  const int role = blockIdx.y;
  if (role == 0) {
    prep_rows_fwd<DK, true>(q, qn, b, s0, p.S, p.Hkv, p.rep);
  } else if (role == 1) {
    prep_rows_fwd<DK, true>(k, kn, b, s0, p.S, p.Hkv, p.rep);
  } else if (role == 2) {
    prep_rows_fwd<DV, false>(v, vt, b, s0, p.S, p.H, 1);
  } else {
    for (int h0 = 0; h0 < p.H; h0 += kPrepSlab) {
      const int hs = min(kPrepSlab, p.H - h0);
      // (B,S,H) side: consecutive lanes walk the heads of one token
      for (int i = threadIdx.x; i < kPrepTile * hs; i += kPrepBlock) {
        const int t = i / hs, hh = i % hs;
        if (s0 + t < p.S) {
          const int64_t at = (b * p.S + s0 + t) * p.H + h0 + hh;
          const float bv = bf16_bits_to_f32(b_raw[at]);
          const float av = bf16_bits_to_f32(a_raw[at]);
          img[0][hh * kPrepPad + t] = sigmoid_f(bv);
          if constexpr (MAMBA) {
            img[1][hh * kPrepPad + t] =
                -expf(A_log[h0 + hh]) * softplus_f(av + dt_bias[h0 + hh]);
          } else {
            img[1][hh * kPrepPad + t] = -softplus_f(-av);  // log-sigmoid
          }
        }
      }
      __syncthreads();
      // (B,H,S) side: consecutive lanes walk the tokens of one head
      for (int i = threadIdx.x; i < kPrepTile * hs; i += kPrepBlock) {
        const int hh = i / kPrepTile, t = i % kPrepTile;
        if (s0 + t < p.S) {
          const int64_t at = (b * p.H + h0 + hh) * p.S + s0 + t;
          beta[at] = img[0][hh * kPrepPad + t];
          g[at] = img[1][hh * kPrepPad + t];
        }
      }
      __syncthreads();
    }
  }
}

// ---- backward ---------------------------------------------------------------

// dq / dk: x (B,S,Hkv,D) bf16 and the rep fp32 rows dy (B,H,S,D) of its value
// heads -> dx (B,S,Hkv,D) bf16. r and x_hat are recomputed from x.
template <int D>
D9D_DEVICE void prep_rows_bwd_norm(const ushort* __restrict__ x_in,
                                   const float* __restrict__ dy,
                                   ushort* __restrict__ dx, int64_t b,
                                   int64_t s0, const PrepShape& p) {
  constexpr int LANES = D / 8;
  constexpr int ROWS = kPrepBlock / LANES;
  const int l = threadIdx.x % LANES;
  const int r0 = threadIdx.x / LANES;
  for (int base = 0; base < kPrepTile * p.Hkv; base += ROWS) {
    const int row = base + r0;
    const int hk = row / kPrepTile;
    const int64_t s = s0 + row % kPrepTile;
    const int64_t tok = s < p.S ? s : p.S - 1;
    const int64_t at = ((b * p.S + tok) * p.Hkv + hk) * D + l * 8;
    float x[8], sum[8];
    load8(x_in + at, x);
    load8(dy + ((b * p.H + (int64_t)hk * p.rep) * p.S + tok) * D + l * 8, sum);
    for (int c = 1; c < p.rep; ++c) {
      float d[8];
      load8(dy + ((b * p.H + (int64_t)hk * p.rep + c) * p.S + tok) * D + l * 8, d);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum[j] += d[j];
    }
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += x[j] * x[j];
    const float norm = sqrtf(row_sum<LANES>(ss));
    const float r = 1.f / fmaxf(norm, kPrepEps);
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      x[j] *= r;  // x_hat
      dot += x[j] * sum[j];
    }
    dot = row_sum<LANES>(dot);
    // below the clamp the divisor is the constant eps: no projection
    if (norm < kPrepEps) dot = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) sum[j] = r * (sum[j] - x[j] * dot);
    if (s < p.S) store8(dx + at, sum);
  }
}

// dv: dvt (B,H,S,D) fp32 -> dv (B,S,H,D) bf16
template <int D>
D9D_DEVICE void prep_rows_bwd_copy(const float* __restrict__ dy,
                                   ushort* __restrict__ dx, int64_t b,
                                   int64_t s0, const PrepShape& p) {
  constexpr int LANES = D / 8;
  constexpr int ROWS = kPrepBlock / LANES;
  const int l = threadIdx.x % LANES;
  const int r0 = threadIdx.x / LANES;
  for (int base = 0; base < kPrepTile * p.H; base += ROWS) {
    const int row = base + r0;
    const int h = row / kPrepTile;
    const int64_t s = s0 + row % kPrepTile;
    if (s < p.S) {
      float d[8];
      load8(dy + ((b * p.H + h) * p.S + s) * D + l * 8, d);
      store8(dx + ((b * p.S + s) * p.H + h) * D + l * 8, d);
    }
  }
}

// part: (2, blocks, H) fp32 per-workgroup sums of da_raw (-> ddt_bias) and of
// dg * g (-> dA_log); written by the gate role only, every entry of it.
template <int DK, int DV, bool MAMBA>
__global__ __launch_bounds__(kPrepBlock) void gdn_prep_bwd_kernel(
    const ushort* __restrict__ q, const ushort* __restrict__ k,
    const ushort* __restrict__ b_raw, const ushort* __restrict__ a_raw,
    const float* __restrict__ A_log, const float* __restrict__ dt_bias,
    const float* __restrict__ dqn, const float* __restrict__ dkn,
    const float* __restrict__ dvt, const float* __restrict__ dbeta,
    const float* __restrict__ dg, ushort* __restrict__ dq,
    ushort* __restrict__ dk, ushort* __restrict__ dv,
    ushort* __restrict__ db_raw, ushort* __restrict__ da_raw,
    float* __restrict__ part, PrepShape p) {
  __shared__ float img[2][kPrepSlab * kPrepPad];
  const int64_t b = blockIdx.x / p.tiles;
  const int64_t s0 = (int64_t)(blockIdx.x % p.tiles) * kPrepTile;
  const int role = blockIdx.y;
  if (role == 0) {
    prep_rows_bwd_norm<DK>(q, dqn, dq, b, s0, p);
  } else if (role == 1) {
    prep_rows_bwd_norm<DK>(k, dkn, dk, b, s0, p);
  } else if (role == 2) {
    prep_rows_bwd_copy<DV>(dvt, dv, b, s0, p);
  } else {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int h0 = 0; h0 < p.H; h0 += kPrepSlab) {
      const int hs = min(kPrepSlab, p.H - h0);
      // (B,H,S) side in; rows past S enter as zeros so the folds below may
      // sum whole image rows
      for (int i = threadIdx.x; i < kPrepTile * hs; i += kPrepBlock) {
        const int hh = i / kPrepTile, t = i % kPrepTile;
        const bool live = s0 + t < p.S;
        const int64_t at = (b * p.H + h0 + hh) * p.S + s0 + t;
        img[0][hh * kPrepPad + t] = live ? dbeta[at] : 0.f;
        img[1][hh * kPrepPad + t] = live ? dg[at] : 0.f;
      }
      __syncthreads();
      // (B,S,H) side out. Each thread rewrites only the image cells it read:
      // img[0] <- da_raw in fp32, img[1] <- dg * g, for the per-head folds.
      for (int i = threadIdx.x; i < kPrepTile * hs; i += kPrepBlock) {
        const int t = i / hs, hh = i % hs;
        if (s0 + t < p.S) {
          const int64_t at = (b * p.S + s0 + t) * p.H + h0 + hh;
          const float bv = bf16_bits_to_f32(b_raw[at]);
          const float av = bf16_bits_to_f32(a_raw[at]);
          const float dbe = img[0][hh * kPrepPad + t];
          const float dgv = img[1][hh * kPrepPad + t];
          // beta (1 - beta) = sigmoid(b) sigmoid(-b), no cancellation
          db_raw[at] = f32_to_bf16_rne(dbe * sigmoid_f(bv) * sigmoid_f(-bv));
          float da;
          if constexpr (MAMBA) {
            const float z = av + dt_bias[h0 + hh];
            const float neg_a = -expf(A_log[h0 + hh]);
            da = dgv * neg_a * sigmoid_f(z);
            img[0][hh * kPrepPad + t] = da;
            img[1][hh * kPrepPad + t] = dgv * neg_a * softplus_f(z);
          } else {
            da = dgv * sigmoid_f(-av);
          }
          da_raw[at] = f32_to_bf16_rne(da);
        }
      }
      __syncthreads();
      if constexpr (MAMBA) {
        // a wave folds one head's 64 tokens in shuffle order, a fixed one
        for (int hh = wave; hh < hs; hh += kPrepBlock / kWaveSize) {
          const float fold_da = wave_reduce_sum(img[0][hh * kPrepPad + lane]);
          const float fold_gg = wave_reduce_sum(img[1][hh * kPrepPad + lane]);
          if (lane == 0) {
            const int64_t nblk = gridDim.x;
            part[(int64_t)blockIdx.x * p.H + h0 + hh] = fold_da;
            part[(nblk + blockIdx.x) * p.H + h0 + hh] = fold_gg;
          }
        }
        __syncthreads();
      }
    }
  }
}

// out[w][h] = sum over blocks of part[w][blk][h], w = blockIdx.y: one
// workgroup per (head, quantity), a fixed strided walk and a fixed tree.
__global__ __launch_bounds__(kPrepBlock) void gdn_prep_fold_kernel(
    const float* __restrict__ part, float* __restrict__ out, int64_t nblk,
    int H) {
  __shared__ float red[kPrepBlock / kWaveSize];
  const int h = blockIdx.x;
  const float* src = part + (int64_t)blockIdx.y * nblk * H + h;
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < nblk; i += kPrepBlock) acc += src[i * H];
  acc = wave_reduce_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    out[(int64_t)blockIdx.y * H + h] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

}  // namespace d9d

// ---- host -------------------------------------------------------------------

namespace {

using OptTensor = c10::optional<torch::Tensor>;

struct PrepArgs {
  int64_t B, S, H, Hkv, Dk, Dv;
  bool mamba;
};

void prep_check_tensor(const char* who, const char* name,
                       const torch::Tensor& t, torch::ScalarType dtype,
                       int64_t rank) {
  TORCH_CHECK(t.is_cuda(), who, ": ", name, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == dtype, who, ": ", name, " must be ", dtype,
              ", got ", t.scalar_type());
  TORCH_CHECK(t.dim() == rank, who, ": ", name, " must have rank ", rank,
              ", got ", t.dim());
  TORCH_CHECK(t.is_contiguous(), who, ": ", name, " must be contiguous");
}

// q, k (B,S,Hkv,Dk); b_raw, a_raw (B,S,H); the gate parameters
PrepArgs prep_checks(const char* who, const torch::Tensor& q,
                     const torch::Tensor& k, const torch::Tensor& b_raw,
                     const torch::Tensor& a_raw, const OptTensor& A_log,
                     const OptTensor& dt_bias) {
  prep_check_tensor(who, "q", q, torch::kBFloat16, 4);
  prep_check_tensor(who, "k", k, torch::kBFloat16, 4);
  prep_check_tensor(who, "b_raw", b_raw, torch::kBFloat16, 3);
  prep_check_tensor(who, "a_raw", a_raw, torch::kBFloat16, 3);
  PrepArgs a;
  a.B = q.size(0); a.S = q.size(1); a.Hkv = q.size(2); a.Dk = q.size(3);
  a.H = b_raw.size(2);
  TORCH_CHECK(k.sizes() == q.sizes(), who, ": q and k must share one (B, S, Hkv, Dk) shape");
  TORCH_CHECK(a.Dk == 64 || a.Dk == 128, who, ": head dim must be 64 or 128, got ", a.Dk);
  TORCH_CHECK(b_raw.size(0) == a.B && b_raw.size(1) == a.S &&
                  a_raw.sizes() == b_raw.sizes(),
              who, ": b_raw and a_raw must be (B, S, H)");
  TORCH_CHECK(a.Hkv >= 1 && a.H >= 1 && a.H % a.Hkv == 0, who, ": H = ", a.H,
              " must be a positive multiple of Hkv = ", a.Hkv);
  TORCH_CHECK(A_log.has_value() == dt_bias.has_value(), who,
              ": A_log and dt_bias come together (Mamba gate) or not at all "
              "(log-sigmoid gate)");
  a.mamba = A_log.has_value();
  if (a.mamba) {
    prep_check_tensor(who, "A_log", *A_log, torch::kFloat32, 1);
    prep_check_tensor(who, "dt_bias", *dt_bias, torch::kFloat32, 1);
    TORCH_CHECK(A_log->numel() == a.H && dt_bias->numel() == a.H, who,
                ": A_log and dt_bias must have length H = ", a.H);
  }
  TORCH_CHECK(a.B * ((a.S + 63) / 64) < ((int64_t)1 << 31), who,
              ": too many token tiles for one grid");
  return a;
}

d9d::PrepShape prep_shape(const PrepArgs& a) {
  d9d::PrepShape p;
  p.S = a.S;
  p.H = (int)a.H; p.Hkv = (int)a.Hkv; p.rep = (int)(a.H / a.Hkv);
  p.tiles = (int)((a.S + d9d::kPrepTile - 1) / d9d::kPrepTile);
  return p;
}

const ushort* bf16_in(const torch::Tensor& t) {
  return reinterpret_cast<const ushort*>(t.data_ptr());
}
ushort* bf16_out(torch::Tensor& t) {
  return reinterpret_cast<ushort*>(t.data_ptr());
}

// pick the <DK, DV, MAMBA> instantiation of KERNEL and run LAUNCH on it
#define GDN_PREP_DISPATCH(KERNEL, a, LAUNCH)                                 \
  do {                                                                       \
    auto pick = [&](auto dk_c, auto dv_c) {                                      \
      if ((a).mamba) {                                                       \
        auto kern = d9d::KERNEL<decltype(dk_c)::value, decltype(dv_c)::value, true>; \
        LAUNCH;                                                              \
      } else {                                                               \
        auto kern = d9d::KERNEL<decltype(dk_c)::value, decltype(dv_c)::value, false>; \
        LAUNCH;                                                              \
      }                                                                      \
    };                                                                       \
    using I64 = std::integral_constant<int, 64>;                             \
    using I128 = std::integral_constant<int, 128>;                           \
    if ((a).Dk == 64 && (a).Dv == 64) pick(I64{}, I64{});                    \
    else if ((a).Dk == 64) pick(I64{}, I128{});                              \
    else if ((a).Dv == 64) pick(I128{}, I64{});                              \
    else pick(I128{}, I128{});                                               \
  } while (0)

}  // namespace

std::vector<torch::Tensor> gdn_prep_fwd(torch::Tensor q, torch::Tensor k,
                                        torch::Tensor v, torch::Tensor b_raw,
                                        torch::Tensor a_raw, OptTensor A_log,
                                        OptTensor dt_bias) {
  const char* who = "gdn_prep_fwd";
  PrepArgs a = prep_checks(who, q, k, b_raw, a_raw, A_log, dt_bias);
  prep_check_tensor(who, "v", v, torch::kBFloat16, 4);
  a.Dv = v.size(3);
  TORCH_CHECK(v.size(0) == a.B && v.size(1) == a.S && v.size(2) == a.H, who,
              ": v must be (B, S, H, Dv) with H = ", a.H);
  TORCH_CHECK(a.Dv == 64 || a.Dv == 128, who, ": head dim must be 64 or 128, got ", a.Dv);

  auto f32 = q.options().dtype(torch::kFloat32);
  auto qn = torch::empty({a.B, a.H, a.S, a.Dk}, q.options());
  auto kn = torch::empty({a.B, a.H, a.S, a.Dk}, q.options());
  auto vt = torch::empty({a.B, a.H, a.S, a.Dv}, q.options());
  auto beta = torch::empty({a.B, a.H, a.S}, f32);
  auto g = torch::empty({a.B, a.H, a.S}, f32);
  if (a.B * a.S == 0) return {qn, kn, vt, beta, g};

  const d9d::PrepShape p = prep_shape(a);
  const dim3 grid((unsigned)(a.B * p.tiles), 4);
  auto stream = at::hip::getCurrentHIPStream();
  GDN_PREP_DISPATCH(
      gdn_prep_fwd_kernel, a,
      hipLaunchKernelGGL(kern, grid, dim3(d9d::kPrepBlock), 0, stream,
                         bf16_in(q), bf16_in(k), bf16_in(v), bf16_in(b_raw),
                         bf16_in(a_raw),
                         a.mamba ? A_log->data_ptr<float>() : nullptr,
                         a.mamba ? dt_bias->data_ptr<float>() : nullptr,
                         bf16_out(qn), bf16_out(kn), bf16_out(vt),
                         beta.data_ptr<float>(), g.data_ptr<float>(), p));
  return {qn, kn, vt, beta, g};
}

std::vector<torch::Tensor> gdn_prep_bwd(torch::Tensor q, torch::Tensor k,
                                        torch::Tensor b_raw, torch::Tensor a_raw,
                                        OptTensor A_log, OptTensor dt_bias,
                                        torch::Tensor dqn, torch::Tensor dkn,
                                        torch::Tensor dvt, torch::Tensor dbeta,
                                        torch::Tensor dg) {
  const char* who = "gdn_prep_bwd";
  PrepArgs a = prep_checks(who, q, k, b_raw, a_raw, A_log, dt_bias);
  prep_check_tensor(who, "dqn", dqn, torch::kFloat32, 4);
  prep_check_tensor(who, "dkn", dkn, torch::kFloat32, 4);
  prep_check_tensor(who, "dvt", dvt, torch::kFloat32, 4);
  prep_check_tensor(who, "dbeta", dbeta, torch::kFloat32, 3);
  prep_check_tensor(who, "dg", dg, torch::kFloat32, 3);
  a.Dv = dvt.size(3);
  const std::vector<int64_t> want{a.B, a.H, a.S, a.Dk};
  TORCH_CHECK(dqn.sizes() == want && dkn.sizes() == want, who,
              ": dqn and dkn must be (B, H, S, Dk)");
  TORCH_CHECK(dvt.size(0) == a.B && dvt.size(1) == a.H && dvt.size(2) == a.S,
              who, ": dvt must be (B, H, S, Dv)");
  TORCH_CHECK(a.Dv == 64 || a.Dv == 128, who, ": head dim must be 64 or 128, got ", a.Dv);
  TORCH_CHECK(dbeta.size(0) == a.B && dbeta.size(1) == a.H &&
                  dbeta.size(2) == a.S && dg.sizes() == dbeta.sizes(),
              who, ": dbeta and dg must be (B, H, S)");

  auto f32 = q.options().dtype(torch::kFloat32);
  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty({a.B, a.S, a.H, a.Dv}, q.options());
  auto db_raw = torch::empty_like(b_raw);
  auto da_raw = torch::empty_like(a_raw);
  torch::Tensor gate_grads;  // (2, H): ddt_bias, dA_log
  if (a.mamba) gate_grads = torch::zeros({2, a.H}, f32);
  if (a.B * a.S > 0) {
    const d9d::PrepShape p = prep_shape(a);
    const int64_t nblk = a.B * p.tiles;
    const dim3 grid((unsigned)nblk, 4);
    torch::Tensor part;
    if (a.mamba) part = torch::empty({2, nblk, a.H}, f32);
    auto stream = at::hip::getCurrentHIPStream();
    GDN_PREP_DISPATCH(
        gdn_prep_bwd_kernel, a,
        hipLaunchKernelGGL(kern, grid, dim3(d9d::kPrepBlock), 0, stream,
                           bf16_in(q), bf16_in(k), bf16_in(b_raw),
                           bf16_in(a_raw),
                           a.mamba ? A_log->data_ptr<float>() : nullptr,
                           a.mamba ? dt_bias->data_ptr<float>() : nullptr,
                           dqn.data_ptr<float>(), dkn.data_ptr<float>(),
                           dvt.data_ptr<float>(), dbeta.data_ptr<float>(),
                           dg.data_ptr<float>(), bf16_out(dq), bf16_out(dk),
                           bf16_out(dv), bf16_out(db_raw), bf16_out(da_raw),
                           a.mamba ? part.data_ptr<float>() : nullptr, p));
    if (a.mamba) {
      hipLaunchKernelGGL(d9d::gdn_prep_fold_kernel, dim3((unsigned)a.H, 2),
                         dim3(d9d::kPrepBlock), 0, stream,
                         part.data_ptr<float>(), gate_grads.data_ptr<float>(),
                         nblk, (int)a.H);
    }
  }
  torch::Tensor dA_log, ddt_bias;
  if (a.mamba) {
    ddt_bias = gate_grads[0];
    dA_log = gate_grads[1];
  }
  return {dq, dk, dv, db_raw, da_raw, dA_log, ddt_bias};
}
