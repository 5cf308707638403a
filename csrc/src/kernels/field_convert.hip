// A type-converting, scaled field copy between two domains of one compute region for gfx950, optionally fused with the
// reduction of the stored values. See stencil/kernels/field_convert.hpp.
//   dst = D( scale * double(src) )   one product in double, one conversion to the destination type D
// The same expression in the row kernel, the generic kernel and the host loop, so all three are bitwise equal to
// stencil2_amd.ops.convert_reference. The stats (FieldStats of the stored values) accumulate as in field_axpby.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "field_reduce_common.hpp"
#include "stencil_common.hpp"
#include "stencil/kernels/field_convert.hpp"
#include "stencil/rt/hip_check.hpp"

#pragma clang fp contract(off)

namespace stencil {

constexpr int kConvertCells = 4; // cells of a lane's item: one 16-B fp32 chunk, two 16-B fp64 chunks

template <typename S, typename D> struct ConvertArgs {
  D *dst;       // raw [0,0,0] of the destination buffer
  const S *src; // ... of the source buffer
  double scale;
  int64_t spx, spxy, dpx, dpxy;     // row and plane pitches of each side, in elements
  int slox, sloy, sloz;             // the region's low corner, raw coordinates of the source
  int dlox, dloy, dloz;             // ... of the destination
  int nx, ny, nz;                   // the region's extent
  int head;                         // cells of item 0 in front of the region (0..3)
  int nitems;                       // 4-cell items covering [lox - head, hix)
  int64_t nrows;                    // (row, plane) pairs
  int64_t count;                    // cells of the region
  FieldStats *slab;                 // one partial per block (stats only)
};

template <typename S, typename D> __host__ __device__ __forceinline__ D convert_cell(double scale, S x) {
  const double t = scale * double(x);
  return D(t);
}

// 4 consecutive cells held as 16-B chunks
template <typename T> struct Quad;
template <> struct Quad<float> {
  float4 v;
  __device__ __forceinline__ void load(const float *p) { v = *reinterpret_cast<const float4 *>(p); }
  __device__ __forceinline__ void store(float *p) const { *reinterpret_cast<float4 *>(p) = v; }
  __device__ __forceinline__ float get(int e) const { return vget<float>(v, e); }
  __device__ __forceinline__ void set(int e, float s) {
    if (e == 0) v.x = s;
    else if (e == 1) v.y = s;
    else if (e == 2) v.z = s;
    else v.w = s;
  }
};
template <> struct Quad<double> {
  double2 a, b;
  __device__ __forceinline__ void load(const double *p) {
    a = *reinterpret_cast<const double2 *>(p);
    b = *reinterpret_cast<const double2 *>(p + 2);
  }
  __device__ __forceinline__ void store(double *p) const {
    *reinterpret_cast<double2 *>(p) = a;
    *reinterpret_cast<double2 *>(p + 2) = b;
  }
  __device__ __forceinline__ double get(int e) const { return e == 0 ? a.x : (e == 1 ? a.y : (e == 2 ? b.x : b.y)); }
  __device__ __forceinline__ void set(int e, double s) {
    if (e == 0) a.x = s;
    else if (e == 1) a.y = s;
    else if (e == 2) b.x = s;
    else b.y = s;
  }
};

// Both sides in the aligned vector layout: wave gw of the grid takes rows gw, gw + GW, ... (GW = waves of the grid) of
// the region's (row, plane) items, U rows at a time, its lanes the rows' 4-cell items lane, lane + 64, ...: a wave's
// loads are one contiguous run of the source row and its stores one of the destination row. A lane's batch is one
// item of each of the U rows: all loads first, then the stores. Items 0 and nitems - 1 may reach outside the region:
// they are loaded whole (inside the source row's read limit) and stored cell by cell for the cells inside only.
template <typename S, typename D, bool STATS>
__global__ __launch_bounds__(kReduceThreads) void field_convert_rows_kernel(ConvertArgs<S, D> a) {
  constexpr int V = kConvertCells;
  constexpr int U = kReduceRowsInFlight;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gw = int64_t(blockIdx.x) * kReduceWaves + wave, GW = int64_t(gridDim.x) * kReduceWaves;
  const int end = a.head + a.nx; // the region is cells [head, end) of the item grid
  Acc<D, false, unsigned int> acc;
  for (int64_t r0 = gw; r0 < a.nrows; r0 += GW * U) {
    int64_t so[U], dofs[U];
    bool rv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t r = r0 + u * GW;
      rv[u] = r < a.nrows; // wave-uniform
      const int64_t rr = rv[u] ? r : r0;
      const int y = int(rr % a.ny), z = int(rr / a.ny);
      so[u] = int64_t(a.sloz + z) * a.spxy + int64_t(a.sloy + y) * a.spx + (a.slox - a.head);
      dofs[u] = int64_t(a.dloz + z) * a.dpxy + int64_t(a.dloy + y) * a.dpx + (a.dlox - a.head);
    }
    for (int c = lane; c < a.nitems; c += 64) {
      Quad<S> in[U];
#pragma unroll
      for (int u = 0; u < U; ++u) in[u].load(a.src + so[u] + int64_t(c) * V);
      const int xb = c * V;
      const bool full = xb >= a.head && xb + V <= end;
      Quad<D> out[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int e = 0; e < V; ++e) out[u].set(e, convert_cell<S, D>(a.scale, in[u].get(e)));
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!rv[u]) continue;
        D *dp = a.dst + dofs[u] + int64_t(c) * V;
        if (full) {
          out[u].store(dp);
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e)
            if (xb + e >= a.head && xb + e < end) dp[e] = out[u].get(e);
        }
        if (STATS) {
#pragma unroll
          for (int e = 0; e < V; ++e)
            if (full || (xb + e >= a.head && xb + e < end)) acc.add(out[u].get(e), D(0));
        }
      }
    }
  }
  if (STATS) block_reduce_store(to_part(acc), a.slab + blockIdx.x, 0);
}

// one thread per cell, grid-strided in cell order: every layout the row kernel refuses
template <typename S, typename D, bool STATS>
__global__ __launch_bounds__(kReduceThreads) void field_convert_generic_kernel(ConvertArgs<S, D> a) {
  const int64_t nx = a.nx, ny = a.ny;
  Acc<D, false, unsigned int> acc;
  for (int64_t i = int64_t(blockIdx.x) * kReduceThreads + threadIdx.x; i < a.count;
       i += int64_t(gridDim.x) * kReduceThreads) {
    const int x = int(i % nx), y = int((i / nx) % ny), z = int(i / (nx * ny));
    const S vs = a.src[int64_t(a.sloz + z) * a.spxy + int64_t(a.sloy + y) * a.spx + (a.slox + x)];
    const D v = convert_cell<S, D>(a.scale, vs);
    a.dst[int64_t(a.dloz + z) * a.dpxy + int64_t(a.dloy + y) * a.dpx + (a.dlox + x)] = v;
    if (STATS) acc.add(v, D(0));
  }
  if (STATS) block_reduce_store(to_part(acc), a.slab + blockIdx.x, 0);
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
template <typename S, typename D> static FieldStats convert_host(const ConvertArgs<S, D> &a) {
  Acc<D, false, unsigned long long> acc;
  for (int z = 0; z < a.nz; ++z)
    for (int y = 0; y < a.ny; ++y)
      for (int x = 0; x < a.nx; ++x) {
        const S vs = a.src[int64_t(a.sloz + z) * a.spxy + int64_t(a.sloy + y) * a.spx + (a.slox + x)];
        const D v = convert_cell<S, D>(a.scale, vs);
        a.dst[int64_t(a.dloz + z) * a.dpxy + int64_t(a.dloy + y) * a.dpx + (a.dlox + x)] = v;
        acc.add(v, D(0));
      }
  FieldStats r;
  store_stats(&r, to_part(acc), a.count);
  return r;
}

static bool convert_fp(const LocalDomain &dom, int64_t q, int64_t *es) {
  return q >= 0 && q < dom.num_data() && fp_quantity(dom, q, es);
}

static bool same_compute_region(const LocalDomain &a, const LocalDomain &b) {
  return a.origin() == b.origin() && a.size() == b.size();
}

bool field_convert_supported(const LocalDomain &srcDom, int64_t qsrc, const LocalDomain &dstDom, int64_t qdst) {
  int64_t es = 0, ed = 0;
  if (!srcDom.realized() || !dstDom.realized() || !convert_fp(srcDom, qsrc, &es) || !convert_fp(dstDom, qdst, &ed))
    return false;
  if (srcDom.backend() != dstDom.backend() || srcDom.gpu() != dstDom.gpu() || !same_compute_region(srcDom, dstDom))
    return false;
  return true;
}

struct ConvertSizes {
  int64_t es, ed;
};

// the refusals shared by enqueue and launch_info; returns the element sizes
static ConvertSizes convert_check(const LocalDomain &srcDom, FieldRef src, const LocalDomain &dstDom, FieldRef dst,
                                  const Rect3 &region, int maxBlocks) {
  STENCIL_REQUIRE(srcDom.realized() && dstDom.realized(), "field convert of an unrealized domain");
  ConvertSizes s{0, 0};
  STENCIL_REQUIRE(convert_fp(srcDom, src.q, &s.es), "field convert takes fp32 / fp64 quantities (src: quantity " << src.q << ")");
  STENCIL_REQUIRE(convert_fp(dstDom, dst.q, &s.ed), "field convert takes fp32 / fp64 quantities (dst: quantity " << dst.q << ")");
  STENCIL_REQUIRE(srcDom.backend() == dstDom.backend(), "field convert domains differ in backend");
  STENCIL_REQUIRE(srcDom.gpu() == dstDom.gpu(),
                  "field convert domains differ in device: " << srcDom.gpu() << " and " << dstDom.gpu());
  STENCIL_REQUIRE(same_compute_region(srcDom, dstDom), "field convert domains differ in compute region: "
                                                           << srcDom.get_compute_region() << " and "
                                                           << dstDom.get_compute_region());
  STENCIL_REQUIRE(!(&srcDom == &dstDom && src.q == dst.q && src.curr == dst.curr),
                  "field convert source and destination are the same buffer (quantity " << src.q << ")");
  STENCIL_REQUIRE(maxBlocks >= 0 && maxBlocks <= (1 << 20), "field convert maxBlocks " << maxBlocks);
  require_region_in_compute(dstDom, region, "convert region");
  return s;
}

template <typename S, typename D> static const void *convert_kernel(int path, bool stats) {
  if (path == 2)
    return stats ? (const void *)field_convert_rows_kernel<S, D, true> : (const void *)field_convert_rows_kernel<S, D, false>;
  return stats ? (const void *)field_convert_generic_kernel<S, D, true>
               : (const void *)field_convert_generic_kernel<S, D, false>;
}

static const void *cbuf(const LocalDomain &dom, FieldRef f) { return f.curr ? dom.curr_data(f.q) : dom.next_data(f.q); }

template <typename S, typename D>
static ConvertArgs<S, D> convert_plan(const LocalDomain &srcDom, FieldRef src, const LocalDomain &dstDom, FieldRef dst,
                                      double scale, const Rect3 &region, bool stats, int maxBlocks,
                                      ConvertLaunchInfo *info) {
  ConvertArgs<S, D> a{};
  const Dim3 so = srcDom.accessor_origin(), dorg = dstDom.accessor_origin();
  const Dim3 sp = srcDom.pitch(src.q), dp = dstDom.pitch(dst.q);
  a.dst = static_cast<D *>(const_cast<void *>(cbuf(dstDom, dst)));
  a.src = static_cast<const S *>(cbuf(srcDom, src));
  a.scale = scale;
  a.spx = sp.x;
  a.spxy = sp.x * sp.y;
  a.dpx = dp.x;
  a.dpxy = dp.x * dp.y;
  a.slox = int(region.lo.x - so.x);
  a.sloy = int(region.lo.y - so.y);
  a.sloz = int(region.lo.z - so.z);
  a.dlox = int(region.lo.x - dorg.x);
  a.dloy = int(region.lo.y - dorg.y);
  a.dloz = int(region.lo.z - dorg.z);
  a.nx = int(region.hi.x - region.lo.x);
  a.ny = int(region.hi.y - region.lo.y);
  a.nz = int(region.hi.z - region.lo.z);
  a.nrows = int64_t(a.ny) * a.nz;
  a.count = a.nrows * a.nx;
  *info = ConvertLaunchInfo();
  info->items = a.nrows;
  if (dstDom.backend() == Backend::Host) return a;
  info->path = 1;
  constexpr int V = kConvertCells;
  // the item grid is anchored at the interior start, which the aligned layouts put on a 64- / 128-B unit on both
  // sides: item 0 starts `head` cells in front of the region (never in front of the interior), and the last item may
  // reach past the region up to the source rows' read limit
  a.head = int((region.lo.x - dstDom.origin().x) % V);
  a.nitems = (a.head + a.nx + V - 1) / V;
  const int64_t sx0 = a.slox - a.head, dx0 = a.dlox - a.head;
  const bool ok = !srcDom.x_halo_align() && !dstDom.x_halo_align() && aligned_vector_layout(srcDom, src.q, sx0) &&
                  aligned_vector_layout(dstDom, dst.q, dx0) && sx0 + int64_t(a.nitems) * V <= srcDom.row_limit(src.q);
  if (ok) info->path = 2;
  if (maxBlocks > 0) {
    info->blocks = maxBlocks;
  } else {
    dstDom.set_device();
    const int64_t resident = resident_blocks(convert_kernel<S, D>(info->path, stats), kReduceThreads, 4);
    info->blocks = std::max<int64_t>(1, std::min(resident, a.nrows));
  }
  return a;
}

template <typename S, typename D, bool STATS>
static void convert_launch(const ConvertArgs<S, D> &a, const ConvertLaunchInfo &info, hipStream_t stream) {
  const dim3 grid(uint32_t(info.blocks)), block(kReduceThreads);
  if (info.path == 2)
    hipLaunchKernelGGL((field_convert_rows_kernel<S, D, STATS>), grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL((field_convert_generic_kernel<S, D, STATS>), grid, block, 0, stream, a);
  HIP_CHECK(hipGetLastError());
}

template <typename S, typename D>
static void convert_enqueue_t(const LocalDomain &srcDom, FieldRef src, const LocalDomain &dstDom, FieldRef dst,
                              double scale, const Rect3 &region, hipStream_t stream, ReduceScratch *stats,
                              int maxBlocks) {
  ConvertLaunchInfo info;
  ConvertArgs<S, D> a = convert_plan<S, D>(srcDom, src, dstDom, dst, scale, region, stats != nullptr, maxBlocks, &info);
  if (info.path == 0) {
    const FieldStats r = convert_host<S, D>(a);
    if (stats) *stats->result_host() = r;
    return;
  }
  if (stats) a.slab = stats->slab(dstDom.gpu(), info.blocks);
  dstDom.set_device();
  if (stats)
    convert_launch<S, D, true>(a, info, stream);
  else
    convert_launch<S, D, false>(a, info, stream);
  if (stats) {
    enqueue_combine(a.slab, info.blocks, a.count, stats->result_device(), stream);
    HIP_CHECK(hipGetLastError());
  }
}

void field_convert_enqueue(const LocalDomain &srcDom, FieldRef src, const LocalDomain &dstDom, FieldRef dst, double scale,
                           const Rect3 &region, hipStream_t stream, ReduceScratch *stats, int maxBlocks) {
  const ConvertSizes s = convert_check(srcDom, src, dstDom, dst, region, maxBlocks);
  if (region.empty()) {
    if (!stats) return;
    // the identity, in stream order behind whatever this scratch's result still waits for
    if (dstDom.backend() == Backend::Host) {
      *stats->result_host() = FieldStats();
      return;
    }
    FieldStats *slab = stats->slab(dstDom.gpu(), 1);
    dstDom.set_device();
    enqueue_combine(slab, 0, 0, stats->result_device(), stream);
    HIP_CHECK(hipGetLastError());
    return;
  }
  if (s.es == 4 && s.ed == 4)
    convert_enqueue_t<float, float>(srcDom, src, dstDom, dst, scale, region, stream, stats, maxBlocks);
  else if (s.es == 4)
    convert_enqueue_t<float, double>(srcDom, src, dstDom, dst, scale, region, stream, stats, maxBlocks);
  else if (s.ed == 4)
    convert_enqueue_t<double, float>(srcDom, src, dstDom, dst, scale, region, stream, stats, maxBlocks);
  else
    convert_enqueue_t<double, double>(srcDom, src, dstDom, dst, scale, region, stream, stats, maxBlocks);
}

ConvertLaunchInfo field_convert_launch_info(const LocalDomain &srcDom, FieldRef src, const LocalDomain &dstDom,
                                            FieldRef dst, double scale, const Rect3 &region, bool stats, int maxBlocks) {
  const ConvertSizes s = convert_check(srcDom, src, dstDom, dst, region, maxBlocks);
  ConvertLaunchInfo info;
  if (region.empty()) {
    info.path = -1;
    return info;
  }
  if (s.es == 4 && s.ed == 4)
    convert_plan<float, float>(srcDom, src, dstDom, dst, scale, region, stats, maxBlocks, &info);
  else if (s.es == 4)
    convert_plan<float, double>(srcDom, src, dstDom, dst, scale, region, stats, maxBlocks, &info);
  else if (s.ed == 4)
    convert_plan<double, float>(srcDom, src, dstDom, dst, scale, region, stats, maxBlocks, &info);
  else
    convert_plan<double, double>(srcDom, src, dstDom, dst, scale, region, stats, maxBlocks, &info);
  return info;
}

} // namespace stencil
