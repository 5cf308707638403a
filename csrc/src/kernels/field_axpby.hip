// Field linear combinations for gfx950, optionally fused with the reduction of the stored values.
// See stencil/kernels/field_axpby.hpp.
//   dst = a * x          t = a_T * x rounded in T
//   dst = a * x + b * y  t = a_T * x, s = b_T * y, dst = t + s: three roundings in T
// The same expression in the row kernel, the generic kernel and the host loop, so all three are bitwise equal to
// stencil2_amd.ops.axpby_reference. The stats (FieldStats of the stored values) accumulate as in field_reduce.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "field_reduce_common.hpp"
#include "stencil_common.hpp"
#include "stencil/kernels/field_axpby.hpp"
#include "stencil/rt/hip_check.hpp"

// no FMA contraction anywhere below, device or host (hipcc contracts by default)
#pragma clang fp contract(off)

namespace stencil {

template <typename T> struct AxpbyArgs {
  T *dst;     // raw [0,0,0] of the destination buffer
  const T *x; // ... of operand x
  const T *y; // ... of operand y (null: one source)
  T a, b;     // the coefficients in the element type
  int64_t px, pxy;
  int lox, loy, loz, hix, hiy, hiz; // region, raw coordinates
  int x0;                           // raw x of chunk 0 (16-B aligned in memory, <= lox)
  int nchunks;                      // chunks covering [x0, hix)
  int ny;                           // rows per plane of the region
  int64_t nrows;                    // (row, plane) items
  int64_t count;                    // cells of the region
  FieldStats *slab;                 // one partial per block (stats only)
};

template <typename T, bool TWO> __host__ __device__ __forceinline__ T axpby_cell(T a, T x, T b, T y) {
  const T t = a * x;
  if (!TWO) return t;
  const T s = b * y;
  return t + s;
}

template <typename T> __device__ __forceinline__ void vset(typename Vec16<T>::type &v, int i, T s);
template <> __device__ __forceinline__ void vset<float>(float4 &v, int i, float s) {
  if (i == 0) v.x = s;
  else if (i == 1) v.y = s;
  else if (i == 2) v.z = s;
  else v.w = s;
}
template <> __device__ __forceinline__ void vset<double>(double2 &v, int i, double s) {
  if (i == 0) v.x = s;
  else v.y = s;
}

// The aligned vector layout: wave gw of the grid takes rows gw, gw + GW, ... (GW = waves of the grid) of the region's
// (row, plane) items, U rows at a time, its lanes the rows' 16-B chunks lane, lane + 64, ... A lane's batch is one
// chunk of each of the U rows: all 2 U loads first, then the U stores, so dst may alias x and / or y (the lane that
// stores a cell is the one that loaded it). Chunks 0 and nchunks - 1 may reach outside [lox, hix): they are loaded
// whole (inside the row's read limit) and stored cell by cell for the cells inside only.
template <typename T, bool TWO, bool STATS, bool NT>
__global__ __launch_bounds__(kReduceThreads) void field_axpby_rows_kernel(AxpbyArgs<T> a) {
  using VT = typename Vec16<T>::type;
  using NV = typename Vec16<T>::native;
  constexpr int V = Vec16<T>::N;
  constexpr int U = kReduceRowsInFlight;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gw = int64_t(blockIdx.x) * kReduceWaves + wave, GW = int64_t(gridDim.x) * kReduceWaves;
  Acc<T, false, unsigned int> acc;
  for (int64_t r0 = gw; r0 < a.nrows; r0 += GW * U) {
    int64_t off[U];
    bool rv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = r0 + u * GW;
      rv[u] = r < a.nrows; // wave-uniform
      const int64_t rr = rv[u] ? r : r0;
      const int y = a.loy + int(rr % a.ny), z = a.loz + int(rr / a.ny);
      off[u] = int64_t(z) * a.pxy + int64_t(y) * a.px + a.x0;
    }
    for (int c = lane; c < a.nchunks; c += 64) {
      VT vx[U], vy[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        vx[u] = *reinterpret_cast<const VT *>(a.x + off[u] + int64_t(c) * V);
        if (TWO) vy[u] = *reinterpret_cast<const VT *>(a.y + off[u] + int64_t(c) * V);
      }
      const int xb = a.x0 + c * V;
      const bool full = xb >= a.lox && xb + V <= a.hix;
      VT vo[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int e = 0; e < V; ++e)
          vset<T>(vo[u], e, axpby_cell<T, TWO>(a.a, vget<T>(vx[u], e), a.b, TWO ? vget<T>(vy[u], e) : T(0)));
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!rv[u]) continue;
        T *dp = a.dst + off[u] + int64_t(c) * V;
        if (full) {
          if (NT) {
            NV nv;
#pragma unroll
            for (int e = 0; e < V; ++e) nv[e] = vget<T>(vo[u], e);
            __builtin_nontemporal_store(nv, reinterpret_cast<NV *>(dp));
          } else {
            *reinterpret_cast<VT *>(dp) = vo[u];
          }
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e)
            if (xb + e >= a.lox && xb + e < a.hix) dp[e] = vget<T>(vo[u], e);
        }
        if (STATS) {
#pragma unroll
          for (int e = 0; e < V; ++e)
            if (full || (xb + e >= a.lox && xb + e < a.hix)) acc.add(vget<T>(vo[u], e), T(0));
        }
      }
    }
  }
  if (STATS) block_reduce_store(to_part(acc), a.slab + blockIdx.x, 0);
}

// one thread per cell, grid-strided in cell order: every layout the row kernel refuses
template <typename T, bool TWO, bool STATS>
__global__ __launch_bounds__(kReduceThreads) void field_axpby_generic_kernel(AxpbyArgs<T> a) {
  const int64_t nx = a.hix - a.lox, ny = a.ny;
  Acc<T, false, unsigned int> acc;
  for (int64_t i = int64_t(blockIdx.x) * kReduceThreads + threadIdx.x; i < a.count;
       i += int64_t(gridDim.x) * kReduceThreads) {
    const int x = a.lox + int(i % nx), y = a.loy + int((i / nx) % ny), z = a.loz + int(i / (nx * ny));
    const int64_t o = int64_t(z) * a.pxy + int64_t(y) * a.px + x;
    const T vx = a.x[o];
    const T vy = TWO ? a.y[o] : T(0);
    const T v = axpby_cell<T, TWO>(a.a, vx, a.b, vy);
    a.dst[o] = v;
    if (STATS) acc.add(v, T(0));
  }
  if (STATS) block_reduce_store(to_part(acc), a.slab + blockIdx.x, 0);
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
template <typename T, bool TWO> static FieldStats axpby_host(const AxpbyArgs<T> &a) {
  Acc<T, false, unsigned long long> acc;
  for (int z = a.loz; z < a.hiz; ++z)
    for (int y = a.loy; y < a.hiy; ++y)
      for (int x = a.lox; x < a.hix; ++x) {
        const int64_t o = int64_t(z) * a.pxy + int64_t(y) * a.px + x;
        const T vx = a.x[o];
        const T vy = TWO ? a.y[o] : T(0);
        const T v = axpby_cell<T, TWO>(a.a, vx, a.b, vy);
        a.dst[o] = v;
        acc.add(v, T(0));
      }
  FieldStats r;
  store_stats(&r, to_part(acc), a.count);
  return r;
}

static bool axpby_fp(const LocalDomain &dom, int64_t q, int64_t *es) {
  return q >= 0 && q < dom.num_data() && fp_quantity(dom, q, es);
}

bool field_axpby_supported(const LocalDomain &dom, int64_t qdst, int64_t qx, int64_t qy) {
  int64_t ed = 0, ex = 0, ey = 0;
  if (!dom.realized() || !axpby_fp(dom, qdst, &ed) || !axpby_fp(dom, qx, &ex)) return false;
  if (ed != ex || dom.pitch(qdst).x != dom.pitch(qx).x) return false;
  return qy < 0 || (axpby_fp(dom, qy, &ey) && ed == ey && dom.pitch(qdst).x == dom.pitch(qy).x);
}

// the refusals shared by enqueue and launch_info; returns the element size
static int64_t axpby_check(const LocalDomain &dom, FieldRef dst, FieldRef x, FieldRef y, const Rect3 &region,
                           int maxBlocks) {
  STENCIL_REQUIRE(dom.realized(), "field axpby of an unrealized domain");
  int64_t ed = 0, ex = 0, ey = 0;
  STENCIL_REQUIRE(axpby_fp(dom, dst.q, &ed), "field axpby takes fp32 / fp64 quantities (dst: quantity " << dst.q << ")");
  STENCIL_REQUIRE(axpby_fp(dom, x.q, &ex), "field axpby takes fp32 / fp64 quantities (operand x: quantity " << x.q << ")");
  STENCIL_REQUIRE(ed == ex, "field axpby operands differ in type: " << ed << "- and " << ex << "-byte elements");
  STENCIL_REQUIRE(dom.pitch(dst.q).x == dom.pitch(x.q).x, "field axpby operands differ in row pitch");
  if (y.q >= 0) {
    STENCIL_REQUIRE(axpby_fp(dom, y.q, &ey), "field axpby takes fp32 / fp64 quantities (operand y: quantity " << y.q << ")");
    STENCIL_REQUIRE(ed == ey, "field axpby operands differ in type: " << ed << "- and " << ey << "-byte elements");
    STENCIL_REQUIRE(dom.pitch(dst.q).x == dom.pitch(y.q).x, "field axpby operands differ in row pitch");
  }
  STENCIL_REQUIRE(maxBlocks >= 0 && maxBlocks <= (1 << 20), "field axpby maxBlocks " << maxBlocks);
  require_region_in_compute(dom, region, "axpby region");
  return ed;
}

template <typename T> static const void *axpby_kernel(int path, bool two, bool stats, bool nt) {
  if (path == 2) {
    if (two) {
      if (stats) return nt ? (const void *)field_axpby_rows_kernel<T, true, true, true>
                           : (const void *)field_axpby_rows_kernel<T, true, true, false>;
      return nt ? (const void *)field_axpby_rows_kernel<T, true, false, true>
                : (const void *)field_axpby_rows_kernel<T, true, false, false>;
    }
    if (stats) return nt ? (const void *)field_axpby_rows_kernel<T, false, true, true>
                         : (const void *)field_axpby_rows_kernel<T, false, true, false>;
    return nt ? (const void *)field_axpby_rows_kernel<T, false, false, true>
              : (const void *)field_axpby_rows_kernel<T, false, false, false>;
  }
  if (two) return stats ? (const void *)field_axpby_generic_kernel<T, true, true>
                        : (const void *)field_axpby_generic_kernel<T, true, false>;
  return stats ? (const void *)field_axpby_generic_kernel<T, false, true>
               : (const void *)field_axpby_generic_kernel<T, false, false>;
}

static const void *buf(const LocalDomain &dom, FieldRef f) { return f.curr ? dom.curr_data(f.q) : dom.next_data(f.q); }

template <typename T>
static AxpbyArgs<T> axpby_plan(const LocalDomain &dom, FieldRef dst, double ca, FieldRef x, double cb, FieldRef y,
                               const Rect3 &region, bool stats, int maxBlocks, bool nt, AxpbyLaunchInfo *info) {
  AxpbyArgs<T> a{};
  const bool two = y.q >= 0;
  const Dim3 org = dom.accessor_origin();
  const Dim3 p = dom.pitch(dst.q);
  a.dst = static_cast<T *>(const_cast<void *>(buf(dom, dst)));
  a.x = static_cast<const T *>(buf(dom, x));
  a.y = two ? static_cast<const T *>(buf(dom, y)) : nullptr;
  a.a = T(ca);
  a.b = T(cb);
  a.px = p.x;
  a.pxy = p.x * p.y;
  a.lox = int(region.lo.x - org.x);
  a.loy = int(region.lo.y - org.y);
  a.loz = int(region.lo.z - org.z);
  a.hix = int(region.hi.x - org.x);
  a.hiy = int(region.hi.y - org.y);
  a.hiz = int(region.hi.z - org.z);
  a.ny = a.hiy - a.loy;
  a.nrows = int64_t(a.ny) * (a.hiz - a.loz);
  a.count = a.nrows * (a.hix - a.lox);
  *info = AxpbyLaunchInfo();
  info->items = a.nrows;
  if (dom.backend() == Backend::Host) return a;
  info->path = 1;
  constexpr int V = Vec16<T>::N;
  // chunk grid anchored at the 16-B aligned interior start, as in field_reduce.hip: x0 <= lox, x0 >= the -x radius,
  // and the last chunk may reach past hix up to the rows' read limit
  const int rxm = int(dom.radius().x(-1));
  const int off = ((a.lox - rxm) % V + V) % V;
  a.x0 = a.lox - off;
  a.nchunks = (a.hix - a.x0 + V - 1) / V;
  bool ok = !dom.x_halo_align() && a.x0 >= 0;
  for (const FieldRef &f : {dst, x, y}) {
    if (f.q < 0) continue;
    ok = ok && aligned_vector_layout(dom, f.q, a.x0) && a.x0 + int64_t(a.nchunks) * V <= dom.row_limit(f.q);
  }
  if (ok) info->path = 2;
  if (maxBlocks > 0) {
    info->blocks = maxBlocks;
  } else {
    dom.set_device();
    const int64_t resident = resident_blocks(axpby_kernel<T>(info->path, two, stats, nt), kReduceThreads, 4);
    info->blocks = std::max<int64_t>(1, std::min(resident, a.nrows));
  }
  return a;
}

template <typename T, bool TWO, bool STATS>
static void axpby_launch(const AxpbyArgs<T> &a, const AxpbyLaunchInfo &info, bool nt, hipStream_t stream) {
  const dim3 grid(uint32_t(info.blocks)), block(kReduceThreads);
  if (info.path == 2) {
    if (nt)
      hipLaunchKernelGGL((field_axpby_rows_kernel<T, TWO, STATS, true>), grid, block, 0, stream, a);
    else
      hipLaunchKernelGGL((field_axpby_rows_kernel<T, TWO, STATS, false>), grid, block, 0, stream, a);
  } else {
    hipLaunchKernelGGL((field_axpby_generic_kernel<T, TWO, STATS>), grid, block, 0, stream, a);
  }
  HIP_CHECK(hipGetLastError());
}

template <typename T>
static void axpby_enqueue_t(const LocalDomain &dom, FieldRef dst, double ca, FieldRef x, double cb, FieldRef y,
                            const Rect3 &region, hipStream_t stream, ReduceScratch *stats, int maxBlocks, bool nt) {
  AxpbyLaunchInfo info;
  const bool two = y.q >= 0;
  AxpbyArgs<T> a = axpby_plan<T>(dom, dst, ca, x, cb, y, region, stats != nullptr, maxBlocks, nt, &info);
  if (info.path == 0) {
    const FieldStats r = two ? axpby_host<T, true>(a) : axpby_host<T, false>(a);
    if (stats) *stats->result_host() = r;
    return;
  }
  if (stats) a.slab = stats->slab(dom.gpu(), info.blocks);
  dom.set_device();
  if (two) {
    if (stats)
      axpby_launch<T, true, true>(a, info, nt, stream);
    else
      axpby_launch<T, true, false>(a, info, nt, stream);
  } else {
    if (stats)
      axpby_launch<T, false, true>(a, info, nt, stream);
    else
      axpby_launch<T, false, false>(a, info, nt, stream);
  }
  if (stats) {
    enqueue_combine(a.slab, info.blocks, a.count, stats->result_device(), stream);
    HIP_CHECK(hipGetLastError());
  }
}

void field_axpby_enqueue(const LocalDomain &dom, FieldRef dst, double a, FieldRef x, double b, FieldRef y,
                         const Rect3 &region, hipStream_t stream, ReduceScratch *stats, int maxBlocks, bool nontemporal) {
  const int64_t es = axpby_check(dom, dst, x, y, region, maxBlocks);
  if (region.empty()) {
    if (!stats) return;
    // the identity, in stream order behind whatever this scratch's result still waits for
    if (dom.backend() == Backend::Host) {
      *stats->result_host() = FieldStats();
      return;
    }
    FieldStats *slab = stats->slab(dom.gpu(), 1);
    dom.set_device();
    enqueue_combine(slab, 0, 0, stats->result_device(), stream);
    HIP_CHECK(hipGetLastError());
    return;
  }
  if (es == 4)
    axpby_enqueue_t<float>(dom, dst, a, x, b, y, region, stream, stats, maxBlocks, nontemporal);
  else
    axpby_enqueue_t<double>(dom, dst, a, x, b, y, region, stream, stats, maxBlocks, nontemporal);
}

AxpbyLaunchInfo field_axpby_launch_info(const LocalDomain &dom, FieldRef dst, double a, FieldRef x, double b, FieldRef y,
                                        const Rect3 &region, bool stats, int maxBlocks, bool nontemporal) {
  const int64_t es = axpby_check(dom, dst, x, y, region, maxBlocks);
  AxpbyLaunchInfo info;
  if (region.empty()) {
    info.path = -1;
    return info;
  }
  if (es == 4)
    axpby_plan<float>(dom, dst, a, x, b, y, region, stats, maxBlocks, nontemporal, &info);
  else
    axpby_plan<double>(dom, dst, a, x, b, y, region, stats, maxBlocks, nontemporal, &info);
  return info;
}

} // namespace stencil
