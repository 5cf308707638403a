#pragma once
// Private to the kernels that produce FieldStats (field_reduce.hip, field_axpby.hip): the per-lane accumulators, the
// partial that lanes, waves and blocks exchange, the block tree and the one-block combine launch. Every lane
// accumulates its cells in doubles in registers, the wave reduces by cross-lane shuffles in a fixed tree, the block
// through LDS in wave order, and each block stores one partial into a slab with plain stores; the combine launch on
// the same stream merges the slab in a fixed tree and stores the result into pinned host memory. No atomics anywhere.
#include <hip/hip_runtime.h>

#include <limits>
#include <type_traits>

#include "stencil/kernels/field_reduce.hpp"

namespace stencil {

constexpr int kReduceThreads = 256, kReduceWaves = kReduceThreads / 64;
constexpr int kReduceRowsInFlight = 4; // rows a wave loads before it accumulates them (in row order)

// per-lane accumulators. One operand: min / max / the non-finite test stay in the element type (conversion to double
// is monotone and exact, so they are the same cells). NF: the counter type (32 bits per lane on the device)
template <typename T, bool TWO, typename NF> struct Acc {
  using M = typename std::conditional<TWO, double, T>::type;
  double s = 0, sa = 0, sq = 0, dt = 0;
  M mn = std::numeric_limits<M>::infinity(), mx = -std::numeric_limits<M>::infinity();
  NF nf = 0;
  // comparisons with NaN are false: a NaN never enters min / max
  __host__ __device__ __forceinline__ void add(T va, T vb) {
    double e;
    if (TWO) {
      const double da = double(va), db = double(vb);
      e = da - db;
      dt += da * db;
      nf += __builtin_isfinite(e) ? 0 : 1;
      mn = e < double(mn) ? M(e) : mn;
      mx = e > double(mx) ? M(e) : mx;
    } else {
      e = double(va);
      nf += __builtin_isfinite(va) ? 0 : 1;
      mn = va < T(mn) ? M(va) : mn;
      mx = va > T(mx) ? M(va) : mx;
    }
    s += e;
    sa += __builtin_fabs(e);
    sq += e * e;
  }
};

// a partial in doubles: what lanes, waves and blocks exchange
struct Part {
  double s = 0, sa = 0, sq = 0, dt = 0;
  double mn = std::numeric_limits<double>::infinity(), mx = -std::numeric_limits<double>::infinity();
  unsigned long long nf = 0;
  __host__ __device__ __forceinline__ void merge(const Part &o) {
    s += o.s;
    sa += o.sa;
    sq += o.sq;
    dt += o.dt;
    nf += o.nf;
    mn = o.mn < mn ? o.mn : mn;
    mx = o.mx > mx ? o.mx : mx;
  }
};
template <typename A> __host__ __device__ __forceinline__ Part to_part(const A &x) {
  Part p;
  p.s = x.s;
  p.sa = x.sa;
  p.sq = x.sq;
  p.dt = x.dt;
  p.mn = double(x.mn);
  p.mx = double(x.mx);
  p.nf = x.nf;
  return p;
}
__host__ __device__ __forceinline__ void store_stats(FieldStats *dst, const Part &p, int64_t count) {
  dst->count = count;
  dst->nonfinite = int64_t(p.nf);
  dst->sum = p.s;
  dst->sum_abs = p.sa;
  dst->sum_sq = p.sq;
  dst->min = p.mn;
  dst->max = p.mx;
  dst->dot = p.dt;
}

// Every thread of the block calls this with its partial. Wave: lane l takes lane l + 32, 16, .. 1 (a fixed tree; lanes
// whose partner is beyond the wave read themselves, and only lane 0's value is used). Block: wave leaders through LDS,
// thread 0 merges them in wave order and stores the block's result.
__device__ __forceinline__ void block_reduce_store(Part p, FieldStats *dst, int64_t count) {
  __shared__ double shd[kReduceWaves][6];
  __shared__ unsigned long long shn[kReduceWaves];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    Part o;
    o.s = __shfl_down(p.s, off, 64);
    o.sa = __shfl_down(p.sa, off, 64);
    o.sq = __shfl_down(p.sq, off, 64);
    o.dt = __shfl_down(p.dt, off, 64);
    o.mn = __shfl_down(p.mn, off, 64);
    o.mx = __shfl_down(p.mx, off, 64);
    o.nf = __shfl_down(p.nf, off, 64);
    p.merge(o);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    shd[wave][0] = p.s;
    shd[wave][1] = p.sa;
    shd[wave][2] = p.sq;
    shd[wave][3] = p.dt;
    shd[wave][4] = p.mn;
    shd[wave][5] = p.mx;
    shn[wave] = p.nf;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Part t = p; // wave 0's
#pragma unroll
    for (int w = 1; w < kReduceWaves; ++w) {
      Part o;
      o.s = shd[w][0];
      o.sa = shd[w][1];
      o.sq = shd[w][2];
      o.dt = shd[w][3];
      o.mn = shd[w][4];
      o.mx = shd[w][5];
      o.nf = shn[w];
      t.merge(o);
    }
    store_stats(dst, t, count);
  }
}

// one block: thread t merges partials t, t + 256, ... in index order, then the block tree; n = 0 stores the identity.
// static: each kernel file that includes this header launches its own copy
static __global__ __launch_bounds__(kReduceThreads) void field_reduce_combine_kernel(const FieldStats *slab, int n,
                                                                                    int64_t count, FieldStats *out) {
  Part p;
  for (int i = threadIdx.x; i < n; i += kReduceThreads) {
    Part o;
    o.s = slab[i].sum;
    o.sa = slab[i].sum_abs;
    o.sq = slab[i].sum_sq;
    o.dt = slab[i].dot;
    o.mn = slab[i].min;
    o.mx = slab[i].max;
    o.nf = (unsigned long long)slab[i].nonfinite;
    p.merge(o);
  }
  block_reduce_store(p, out, count);
}

// the combine launch behind the `blocks` partials of `slab`, on the same stream
inline void enqueue_combine(const FieldStats *slab, int64_t blocks, int64_t count, FieldStats *out, hipStream_t stream) {
  hipLaunchKernelGGL(field_reduce_combine_kernel, dim3(1), dim3(kReduceThreads), 0, stream, slab, int(blocks), count, out);
}

} // namespace stencil
