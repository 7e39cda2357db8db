// k-means|| seeding (Bahmani et al. 2012; seeding.py is the host side and
// states the algorithm): the streaming passes over the resident rows.
//
// The heavy step, "nearest of the m new candidates for every row", is the
// labels-only assignment the context already has (km_predict's kernels: the
// reference's np.argmin(np.linalg.norm(C - x, axis=1)) exactly).  What is
// here runs after it:
//   k_seed_fold    t = np.add.reduce((c - x) * (c - x)) for the candidate the
//                  label names, in float64 with NumPy's pairwise order
//                  (km_exact.h: the sum the np_pw helpers form before their
//                  sqrt), min-folded into D2 / near, and the workgroup's
//                  share of phi = sum D2;
//   k_seed_sample  the keyed Bernoulli pick u * phi < ell * D2[i], u from a
//                  counter-based hash of the global row, compacted in row
//                  order (count pass, scan, write pass);
//   k_seed_weights the histogram of near.
// phi is summed in a fixed order (per-thread row order, a fixed tree per
// workgroup, workgroups in index order): two identical calls return the same
// bits.  Integer atomics only.
#include <algorithm>

#include "km_exact.h"
#include "km_internal.h"

namespace km {

namespace {

constexpr int SEED_T = 256;          // threads per workgroup
constexpr int SEED_ROWS = 64;        // rows per workgroup step of the fold: 32 lane groups x 2 rows
constexpr int SEED_LDS_BINS = 8192;  // histogram bins privatised in LDS (32 KiB)

__global__ __launch_bounds__(SEED_T) void k_seed_init(double* __restrict__ D2, int32_t* __restrict__ near,
                                                      int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * SEED_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * SEED_T) {
    D2[i] = __longlong_as_double(0x7FF0000000000000ll);  // +inf
    near[i] = -1;
  }
}

// fixed-order sum of one value per thread: lanes by shuffle-down, then the
// four waves in order; the result in thread 0
__device__ __forceinline__ double seed_block_sum(double v, double* wsum) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) wsum[w] = v;
  __syncthreads();
  return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// 8 consecutive lanes evaluate the sums of two rows (np_pw8: lane u holds
// NumPy's accumulator r[u] of both); lane u == 0 folds.  X is read once; the
// candidate rows (m of them) come from L2 / Infinity Cache.
template <int DEPTH>
__global__ __launch_bounds__(SEED_T) void k_seed_fold(const float* __restrict__ X, int64_t n, int d, int dp,
                                                      const double* __restrict__ C, int k,
                                                      const int32_t* __restrict__ labels, int32_t first_id,
                                                      double* __restrict__ D2, int32_t* __restrict__ near,
                                                      double* __restrict__ part) {
  __shared__ double wsum[SEED_T / 64];
  const int u = threadIdx.x & 7, grp = threadIdx.x >> 3;
  double acc = 0.0;
  for (int64_t base = (int64_t)blockIdx.x * SEED_ROWS; base < n; base += (int64_t)gridDim.x * SEED_ROWS) {
    const int64_t ra = base + grp, rb = base + 32 + grp;
    const bool va = ra < n, vb = rb < n;
    // rows past the end re-read the last row (every lane takes part in the
    // butterfly); their result is dropped
    const int64_t ia = va ? ra : n - 1, ib = vb ? rb : n - 1;
    int ja = labels[ia], jb = labels[ib];
    const bool oka = (unsigned)ja < (unsigned)k, okb = (unsigned)jb < (unsigned)k;
    if (!oka) ja = 0;
    if (!okb) jb = 0;
    const float* __restrict__ xa = X + (size_t)ia * dp;
    const float* __restrict__ xb = X + (size_t)ib * dp;
    const double* __restrict__ ca = C + (size_t)ja * d;
    const double* __restrict__ cb = C + (size_t)jb * d;
    double ta, tb;
    np_pw8<DEPTH>(
        [&](int f, double& a, double& b) {
          a = np_sq(ca[f], xa[f]);
          b = np_sq(cb[f], xb[f]);
        },
        0, d, u, ta, tb);
    if (u == 0) {
      if (va) {
        double cur = D2[ra];
        if (oka && ta < cur) {
          cur = ta;
          D2[ra] = ta;
          near[ra] = first_id + ja;
        }
        acc += cur;
      }
      if (vb) {
        double cur = D2[rb];
        if (okb && tb < cur) {
          cur = tb;
          D2[rb] = tb;
          near[rb] = first_id + jb;
        }
        acc += cur;
      }
    }
  }
  const double s = seed_block_sum(acc, wsum);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// part[nb] = part[0] + ... + part[nb - 1]: strided per thread, then the fixed tree
__global__ __launch_bounds__(SEED_T) void k_seed_phi(double* __restrict__ part, int nb) {
  __shared__ double wsum[SEED_T / 64];
  double acc = 0.0;
  for (int b = threadIdx.x; b < nb; b += SEED_T) acc += part[b];
  const double s = seed_block_sum(acc, wsum);
  if (threadIdx.x == 0) part[nb] = s;
}

// Workgroup b owns rows [b * chunk, (b + 1) * chunk).  WRITE = false: the
// number of its picks into cnt[b]; WRITE = true: their local indices, in row
// order, from out[offs[b]] on (nothing at or past cap).
template <bool WRITE>
__global__ __launch_bounds__(SEED_T) void k_seed_sample(const double* __restrict__ D2, int64_t n, int64_t chunk,
                                                        uint64_t key, int64_t row0, double ell, double phi,
                                                        uint32_t* __restrict__ cnt,
                                                        const int64_t* __restrict__ offs, int64_t* __restrict__ out,
                                                        int64_t cap) {
#pragma clang fp contract(off)
  __shared__ uint32_t wc[SEED_T / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < n ? lo + chunk : n;
  const uint64_t below = (1ull << lane) - 1ull;
  int64_t run = WRITE ? offs[blockIdx.x] : 0;
  uint32_t total = 0;
  for (int64_t b = lo; b < hi; b += SEED_T) {
    const int64_t i = b + t;
    bool hit = false;
    if (i < hi) {
      const uint64_t h = splitmix64(key ^ (uint64_t)(row0 + i));
      const double uu = (double)(h >> 11) * (1.0 / 9007199254740992.0);
      const double lhs = uu * phi, rhs = ell * D2[i];
      hit = lhs < rhs;
    }
    const uint64_t m = __ballot(hit);
    if (lane == 0) wc[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, step = 0;
#pragma unroll
    for (int q = 0; q < SEED_T / 64; ++q) {
      if (q < w) before += wc[q];
      step += wc[q];
    }
    if (WRITE && hit) {
      const int64_t idx = run + before + __popcll(m & below);
      if (idx < cap) out[idx] = i;
    }
    run += step;
    total += step;
    __syncthreads();
  }
  if (!WRITE && t == 0) cnt[blockIdx.x] = total;
}

// exclusive scan of the workgroups' counts (nb <= a few thousand: one thread)
__global__ void k_seed_scan(const uint32_t* __restrict__ cnt, int nb, int64_t* __restrict__ offs) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t run = 0;
  for (int b = 0; b < nb; ++b) {
    offs[b] = run;
    run += cnt[b];
  }
  offs[nb] = run;
}

// lds != 0: a histogram per workgroup in LDS (m_total bins), flushed with one
// integer atomic per non-empty bin; else integer atomics on counts directly
__global__ __launch_bounds__(SEED_T) void k_seed_weights(const int32_t* __restrict__ near, int64_t n, int m_total,
                                                         int lds, unsigned long long* __restrict__ counts) {
  __shared__ uint32_t bins[SEED_LDS_BINS];
  if (lds) {
    for (int j = threadIdx.x; j < m_total; j += SEED_T) bins[j] = 0u;
    __syncthreads();
  }
  for (int64_t i = (int64_t)blockIdx.x * SEED_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * SEED_T) {
    const int v = near[i];
    if ((unsigned)v < (unsigned)m_total) {
      if (lds)
        atomicAdd(&bins[v], 1u);
      else
        atomicAdd(&counts[v], 1ull);
    }
  }
  if (lds) {
    __syncthreads();
    for (int j = threadIdx.x; j < m_total; j += SEED_T)
      if (bins[j]) atomicAdd(&counts[j], (unsigned long long)bins[j]);
  }
}

int stream_blocks(int64_t items, int per_block, int n_cu) {
  const int64_t need = (items + per_block - 1) / per_block;
  const int64_t most = (int64_t)std::max(n_cu, 1) * 8;
  return (int)std::max<int64_t>(1, std::min(need, most));
}

}  // namespace

int seed_fold_blocks(int64_t n, int n_cu) { return stream_blocks(n, SEED_ROWS, n_cu); }
int seed_sample_blocks(int64_t n, int n_cu) { return stream_blocks(n, SEED_T, n_cu); }

hipError_t launch_seed_init(double* D2, int32_t* near, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_seed_init, dim3(stream_blocks(n, SEED_T, 256)), dim3(SEED_T), 0, s, D2, near, n);
  return hipGetLastError();
}

hipError_t launch_seed_fold(const float* X, const Geometry& g, const double* C64, const int32_t* labels,
                            int32_t first_id, double* D2, int32_t* near, double* part, int n_cu, hipStream_t s) {
  const int nb = seed_fold_blocks(g.n, n_cu);
  if (g.n <= 0) {
    hipError_t e = hipMemsetAsync(part, 0, sizeof(double) * (nb + 1), s);
    return e;
  }
  // depth of NumPy's pairwise halving: 2 for d <= 256, 5 up to 4096 features
  if (g.d <= 256)
    KM_TIMED_LAUNCH((k_seed_fold<2>), dim3(nb), dim3(SEED_T), 0, s, X, g.n, g.d, g.dp, C64, g.k, labels, first_id, D2,
                    near, part);
  else
    KM_TIMED_LAUNCH((k_seed_fold<5>), dim3(nb), dim3(SEED_T), 0, s, X, g.n, g.d, g.dp, C64, g.k, labels, first_id, D2,
                    near, part);
  hipLaunchKernelGGL(k_seed_phi, dim3(1), dim3(SEED_T), 0, s, part, nb);
  return hipGetLastError();
}

hipError_t launch_seed_sample(const double* D2, int64_t n, uint64_t seed, int32_t round, int64_t row0, double ell,
                              double phi, uint32_t* cnt, int64_t* offs, int64_t* out, int64_t cap, int n_cu,
                              hipStream_t s) {
  const int nb = seed_sample_blocks(n, n_cu);
  if (n <= 0) return hipMemsetAsync(offs, 0, sizeof(int64_t) * (nb + 1), s);
  const uint64_t key = splitmix64(seed ^ ((uint64_t)(int64_t)round * 0xD1B54A32D192ED03ull));
  // whole steps of SEED_T rows per workgroup
  const int64_t chunk = ((n + nb - 1) / nb + SEED_T - 1) / SEED_T * SEED_T;
  hipLaunchKernelGGL((k_seed_sample<false>), dim3(nb), dim3(SEED_T), 0, s, D2, n, chunk, key, row0, ell, phi, cnt,
                     (const int64_t*)nullptr, (int64_t*)nullptr, (int64_t)0);
  hipLaunchKernelGGL(k_seed_scan, dim3(1), dim3(64), 0, s, (const uint32_t*)cnt, nb, offs);
  hipLaunchKernelGGL((k_seed_sample<true>), dim3(nb), dim3(SEED_T), 0, s, D2, n, chunk, key, row0, ell, phi, cnt,
                     (const int64_t*)offs, out, cap);
  return hipGetLastError();
}

hipError_t launch_seed_weights(const int32_t* near, int64_t n, int32_t m_total, unsigned long long* counts, int n_cu,
                               hipStream_t s) {
  if (n <= 0 || m_total <= 0) return hipSuccess;
  const int lds = m_total <= SEED_LDS_BINS ? 1 : 0;
  hipLaunchKernelGGL(k_seed_weights, dim3(stream_blocks(n, SEED_T * 8, n_cu)), dim3(SEED_T), 0, s, near, n,
                     (int)m_total, lds, counts);
  return hipGetLastError();
}

}  // namespace km
