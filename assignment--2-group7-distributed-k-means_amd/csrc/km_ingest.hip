// Device-source ingest (km_load_device): rows that already sit in HBM as a
// row-major [nrows][d] array of fp16, bf16, fp32 or fp64 (a torch tensor or a
// view of one) are converted into the context's row store, float32 with row
// stride dp and zero padding columns, without a trip through the host.
//
// One thread writes one 16-byte group of X (4 floats, one float4 store);
// consecutive lanes take consecutive groups of a row, then of the next row.
// The conversion is the host route's: fp16 and bf16 widen exactly, fp64 rounds
// to nearest-even (out of range -> +-inf, NaN stays NaN, the sign of zero is
// kept, subnormals are rounded, not flushed), which is what
// np.ascontiguousarray(rows, dtype=np.float32) does before km_load_rows.
//
// A thread never reads outside [r * src_stride, r * src_stride + d) of its
// row: the group that straddles column d loads element by element, so a view
// whose last row ends at the last byte of its allocation is safe.  No atomics,
// no LDS.
#include <hip/hip_fp16.h>

#include "km_internal.h"

namespace km {
namespace {

// the 4 source elements of one group, as loaded (converted after every load
// of the unrolled body has been issued)
template <class T>
struct Raw4 {
  T v[4];
};

// 16-bit types travel as raw bits: T = __half is fp16, T = uint16_t is bf16
template <class T>
struct Bits {
  using type = T;
};
template <>
struct Bits<__half> {
  using type = uint16_t;
};

template <class T>
__device__ __forceinline__ float widen(typename Bits<T>::type b);
template <>
__device__ __forceinline__ float widen<__half>(uint16_t b) {
  return (float)__builtin_bit_cast(_Float16, b);  // v_cvt_f32_f16: exact, subnormals kept
}
template <>
__device__ __forceinline__ float widen<uint16_t>(uint16_t b) {
  return __uint_as_float((uint32_t)b << 16);  // bf16 is the upper half of a float32
}
template <>
__device__ __forceinline__ float widen<float>(float b) {
  return b;
}
template <>
__device__ __forceinline__ float widen<double>(double b) {
  return (float)b;  // v_cvt_f32_f64: round to nearest-even, +-inf beyond the range
}

// VEC: p is aligned to the group's load (the launcher checked base and stride)
// and the full group is one vector load; otherwise 4 element loads, which the
// compiler is free to merge (today it does, into the same instruction: gfx950
// global loads need no alignment) but which require none wider
template <class T, bool VEC>
__device__ __forceinline__ Raw4<typename Bits<T>::type> load_group(const typename Bits<T>::type* __restrict__ p,
                                                                   int left) {
  using B = typename Bits<T>::type;
  Raw4<B> o;
  if (left >= 4) {
    if constexpr (!VEC) {
      o.v[0] = p[0];
      o.v[1] = p[1];
      o.v[2] = p[2];
      o.v[3] = p[3];
    } else if constexpr (sizeof(B) == 2) {
      const short4 q = *reinterpret_cast<const short4*>(p);
      o.v[0] = (B)(uint16_t)q.x;
      o.v[1] = (B)(uint16_t)q.y;
      o.v[2] = (B)(uint16_t)q.z;
      o.v[3] = (B)(uint16_t)q.w;
    } else if constexpr (sizeof(B) == 4) {
      const float4 q = *reinterpret_cast<const float4*>(p);
      o.v[0] = q.x;
      o.v[1] = q.y;
      o.v[2] = q.z;
      o.v[3] = q.w;
    } else {
      const double2 q0 = *reinterpret_cast<const double2*>(p);
      const double2 q1 = *reinterpret_cast<const double2*>(p + 2);
      o.v[0] = q0.x;
      o.v[1] = q0.y;
      o.v[2] = q1.x;
      o.v[3] = q1.y;
    }
  } else {
    // the group across column d (left in 1..3) or a padding group (left <= 0):
    // all-zero bits are +0.0 in every source type
#pragma unroll
    for (int j = 0; j < 4; ++j) o.v[j] = j < left ? p[j] : B{};
  }
  return o;
}

constexpr int kIngestUnroll = 4;

// gpr = dp / 4 groups per row; step = threads of the grid, as step_r rows and
// step_g groups (step = step_r * gpr + step_g), so the loop carries (row,
// group) without a 64-bit division: rows * gpr exceeds 2^32 for large n
template <class T, bool VEC>
__global__ __launch_bounds__(256) void k_ingest(const typename Bits<T>::type* __restrict__ src, int64_t src_stride,
                                                int64_t nrows, int d, int dp, int step_r, int step_g,
                                                float* __restrict__ X) {
  using B = typename Bits<T>::type;
  const int gpr = dp >> 2;
  const uint32_t i0 = blockIdx.x * 256u + threadIdx.x;  // < step <= 8 n_cu 256
  int64_t r = i0 / (uint32_t)gpr;
  int g = (int)(i0 % (uint32_t)gpr);
  auto advance = [&](int64_t& rr, int& gg) {
    gg += step_g;
    rr += step_r;
    if (gg >= gpr) {
      gg -= gpr;
      ++rr;
    }
  };
  auto store = [&](int64_t rr, int gg, const Raw4<B>& raw) {
    float4 o;
    o.x = widen<T>(raw.v[0]);
    o.y = widen<T>(raw.v[1]);
    o.z = widen<T>(raw.v[2]);
    o.w = widen<T>(raw.v[3]);
    *reinterpret_cast<float4*>(X + rr * dp + 4 * gg) = o;
  };
  for (;;) {
    int64_t rr[kIngestUnroll];
    int gg[kIngestUnroll];
    rr[0] = r;
    gg[0] = g;
#pragma unroll
    for (int u = 1; u < kIngestUnroll; ++u) {
      rr[u] = rr[u - 1];
      gg[u] = gg[u - 1];
      advance(rr[u], gg[u]);
    }
    if (rr[kIngestUnroll - 1] >= nrows) break;  // rows only grow: the others are in range too
    Raw4<B> raw[kIngestUnroll];
#pragma unroll
    for (int u = 0; u < kIngestUnroll; ++u)
      raw[u] = load_group<T, VEC>(src + rr[u] * src_stride + 4 * gg[u], d - 4 * gg[u]);
#pragma unroll
    for (int u = 0; u < kIngestUnroll; ++u) store(rr[u], gg[u], raw[u]);
    r = rr[kIngestUnroll - 1];
    g = gg[kIngestUnroll - 1];
    advance(r, g);
  }
  for (; r < nrows; advance(r, g)) store(r, g, load_group<T, VEC>(src + r * src_stride + 4 * g, d - 4 * g));
}

template <class T>
hipError_t launch_t(const void* src, int64_t src_stride, int64_t nrows, int d, int dp, float* X, int n_cu,
                    hipStream_t s) {
  using B = typename Bits<T>::type;
  const int64_t gpr = dp / 4;
  const int64_t total = nrows * gpr;
  int64_t blocks = (total + 255) / 256;
  if (blocks > (int64_t)8 * n_cu) blocks = (int64_t)8 * n_cu;
  const int64_t step = blocks * 256;
  const int step_r = (int)(step / gpr), step_g = (int)(step % gpr);
  const bool vec = ingest_vec(src, src_stride, (int)sizeof(B));
  const B* p = static_cast<const B*>(src);
  if (vec)
    hipLaunchKernelGGL((k_ingest<T, true>), dim3((unsigned)blocks), dim3(256), 0, s, p, src_stride, nrows, d, dp,
                       step_r, step_g, X);
  else
    hipLaunchKernelGGL((k_ingest<T, false>), dim3((unsigned)blocks), dim3(256), 0, s, p, src_stride, nrows, d, dp,
                       step_r, step_g, X);
  return hipGetLastError();
}

}  // namespace

int ingest_elem_size(int dtype) {
  switch (dtype) {
    case KM_DT_F32: return 4;
    case KM_DT_F64: return 8;
    case KM_DT_F16:
    case KM_DT_BF16: return 2;
    default: return 0;
  }
}

bool ingest_vec(const void* src, int64_t src_stride, int elem_size) {
  // one group is 4 elements: an 8-byte load for the 16-bit types, a 16-byte
  // load for float, two 16-byte loads for double
  const uint64_t a = elem_size == 2 ? 8 : 16;
  return (uint64_t)(uintptr_t)src % a == 0 && ((uint64_t)src_stride * (uint64_t)elem_size) % a == 0;
}

hipError_t launch_ingest(const void* src, int dtype, int64_t src_stride, int64_t nrows, const Geometry& g, float* X,
                         int n_cu, hipStream_t s) {
  if (nrows <= 0) return hipSuccess;
  if (g.dp % 4 != 0 || g.dp < g.d || src_stride < g.d || n_cu <= 0) return hipErrorInvalidValue;
  switch (dtype) {
    case KM_DT_F32: return launch_t<float>(src, src_stride, nrows, g.d, g.dp, X, n_cu, s);
    case KM_DT_F64: return launch_t<double>(src, src_stride, nrows, g.d, g.dp, X, n_cu, s);
    case KM_DT_F16: return launch_t<__half>(src, src_stride, nrows, g.d, g.dp, X, n_cu, s);
    case KM_DT_BF16: return launch_t<uint16_t>(src, src_stride, nrows, g.d, g.dp, X, n_cu, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace km
