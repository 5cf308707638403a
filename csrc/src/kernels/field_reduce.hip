// Field reductions for gfx950. See stencil/kernels/field_reduce.hpp (FieldStats).
//   one operand:  e = double(a)
//   two operands: e = double(a) - double(b), dot = sum of double(a) * double(b)
// Every lane accumulates its cells in doubles in registers, the wave reduces by cross-lane shuffles in a fixed tree,
// the block through LDS in wave order, and each block stores one partial into a slab with plain stores; a second
// one-block launch on the same stream combines the slab in a fixed tree and stores the result into pinned host
// memory. No atomics anywhere: the result depends on the layout, the region and the number of blocks only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "field_reduce_common.hpp"
#include "stencil_common.hpp"
#include "stencil/kernels/field_reduce.hpp"
#include "stencil/rt/hip_check.hpp"

namespace stencil {

template <typename T> struct ReduceArgs {
  const T *a; // raw [0,0,0] of operand a
  const T *b; // ... of operand b (null: one operand)
  int64_t px, pxy;
  int lox, loy, loz, hix, hiy, hiz; // region, raw coordinates
  int x0;                           // raw x of chunk 0 (16-B aligned in memory, <= lox)
  int nchunks;                      // chunks covering [x0, hix)
  int ny;                           // rows per plane of the region
  int64_t nrows;                    // (row, plane) items
  int64_t count;                    // cells of the region
  FieldStats *slab;                 // one partial per block
};


// The aligned vector layout: wave gw of the grid takes rows gw, gw + GW, gw + 2 GW, ... (GW = waves of the grid) of
// the region's (row, plane) items, its lanes the row's 16-B chunks lane, lane + 64, ... Chunks 0 and nchunks - 1 may
// reach outside [lox, hix): those cells are loaded (inside the row's read limit) and dropped before any accumulator.
template <typename T, bool TWO>
__global__ __launch_bounds__(kReduceThreads) void field_reduce_rows_kernel(ReduceArgs<T> a) {
  using VT = typename Vec16<T>::type;
  constexpr int V = Vec16<T>::N;
  constexpr int U = kReduceRowsInFlight;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gw = int64_t(blockIdx.x) * kReduceWaves + wave, GW = int64_t(gridDim.x) * kReduceWaves;
  Acc<T, TWO, unsigned int> acc;
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
      VT va[U], vb[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        va[u] = *reinterpret_cast<const VT *>(a.a + off[u] + int64_t(c) * V);
        if (TWO) vb[u] = *reinterpret_cast<const VT *>(a.b + off[u] + int64_t(c) * V);
      }
      const int xb = a.x0 + c * V;
      const bool full = xb >= a.lox && xb + V <= a.hix;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!rv[u]) continue;
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (full || (xb + e >= a.lox && xb + e < a.hix)) acc.add(vget<T>(va[u], e), TWO ? vget<T>(vb[u], e) : T(0));
      }
    }
  }
  block_reduce_store(to_part(acc), a.slab + blockIdx.x, 0);
}

// one thread per cell, grid-strided in cell order: every layout the row kernel refuses
template <typename T, bool TWO>
__global__ __launch_bounds__(kReduceThreads) void field_reduce_generic_kernel(ReduceArgs<T> a) {
  const int64_t nx = a.hix - a.lox, ny = a.ny;
  Acc<T, TWO, unsigned int> acc;
  for (int64_t i = int64_t(blockIdx.x) * kReduceThreads + threadIdx.x; i < a.count;
       i += int64_t(gridDim.x) * kReduceThreads) {
    const int x = a.lox + int(i % nx), y = a.loy + int((i / nx) % ny), z = a.loz + int(i / (nx * ny));
    const int64_t o = int64_t(z) * a.pxy + int64_t(y) * a.px + x;
    acc.add(a.a[o], TWO ? a.b[o] : T(0));
  }
  block_reduce_store(to_part(acc), a.slab + blockIdx.x, 0);
}


// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
ReduceScratch::~ReduceScratch() { release(); }

void ReduceScratch::release() {
  if (dev_ >= 0) (void)hipSetDevice(dev_);
  if (slab_) (void)hipFree(slab_);
  if (host_) (void)hipHostFree(host_);
  slab_ = nullptr;
  host_ = hostDev_ = nullptr;
  cap_ = 0;
  dev_ = -1;
}

FieldStats *ReduceScratch::slab(int dev, int64_t blocks) {
  if (dev < 0) return nullptr;
  if (dev != dev_) {
    release();
    dev_ = dev;
  }
  HIP_CHECK(hipSetDevice(dev));
  if (!host_) {
    HIP_CHECK(hipHostMalloc((void **)&host_, sizeof(FieldStats), hipHostMallocMapped));
    *host_ = FieldStats();
    HIP_CHECK(hipHostGetDevicePointer((void **)&hostDev_, host_, 0));
  }
  if (blocks > cap_) {
    // a reduction in flight may still read the old slab: hipFree waits for the device
    if (slab_) HIP_CHECK(hipFree(slab_));
    slab_ = nullptr;
    cap_ = std::max<int64_t>(blocks, 1024);
    HIP_CHECK(hipMalloc((void **)&slab_, size_t(cap_) * sizeof(FieldStats)));
  }
  return slab_;
}

template <typename T, bool TWO> static FieldStats reduce_host(const ReduceArgs<T> &a) {
  Acc<T, TWO, unsigned long long> acc;
  for (int z = a.loz; z < a.hiz; ++z)
    for (int y = a.loy; y < a.hiy; ++y)
      for (int x = a.lox; x < a.hix; ++x) {
        const int64_t o = int64_t(z) * a.pxy + int64_t(y) * a.px + x;
        acc.add(a.a[o], TWO ? a.b[o] : T(0));
      }
  FieldStats r;
  store_stats(&r, to_part(acc), a.count);
  return r;
}

static bool reduce_fp(const LocalDomain &dom, int64_t q, int64_t *es) {
  return q >= 0 && q < dom.num_data() && fp_quantity(dom, q, es);
}

bool field_reduce_supported(const LocalDomain &dom, int64_t qa, int64_t qb) {
  int64_t ea = 0, eb = 0;
  if (!dom.realized() || !reduce_fp(dom, qa, &ea)) return false;
  return qb < 0 || (reduce_fp(dom, qb, &eb) && ea == eb);
}

// the refusals shared by enqueue and launch_info; returns the element size
static int64_t reduce_check(const LocalDomain &dom, int64_t qa, int64_t qb, const Rect3 &region, int maxBlocks) {
  STENCIL_REQUIRE(dom.realized(), "field reduction of an unrealized domain");
  int64_t ea = 0, eb = 0;
  STENCIL_REQUIRE(reduce_fp(dom, qa, &ea), "field reductions take fp32 / fp64 quantities (operand a: quantity " << qa << ")");
  if (qb >= 0) {
    STENCIL_REQUIRE(reduce_fp(dom, qb, &eb), "field reductions take fp32 / fp64 quantities (operand b: quantity " << qb << ")");
    STENCIL_REQUIRE(ea == eb, "field reduction operands differ in type: " << ea << "- and " << eb << "-byte elements");
    STENCIL_REQUIRE(dom.pitch(qa).x == dom.pitch(qb).x, "field reduction operands differ in row pitch");
  }
  STENCIL_REQUIRE(maxBlocks >= 0 && maxBlocks <= (1 << 20), "field reduction maxBlocks " << maxBlocks);
  require_region_in_compute(dom, region, "reduction region");
  return ea;
}

template <typename T, bool TWO>
static ReduceArgs<T> reduce_plan(const LocalDomain &dom, int64_t qa, bool currA, int64_t qb, bool currB,
                                 const Rect3 &region, int maxBlocks, ReduceLaunchInfo *info) {
  ReduceArgs<T> a{};
  const Dim3 org = dom.accessor_origin();
  const Dim3 p = dom.pitch(qa);
  a.a = static_cast<const T *>(currA ? dom.curr_data(qa) : dom.next_data(qa));
  a.b = TWO ? static_cast<const T *>(currB ? dom.curr_data(qb) : dom.next_data(qb)) : nullptr;
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
  *info = ReduceLaunchInfo();
  info->items = a.nrows;
  if (dom.backend() == Backend::Host) return a;
  info->path = 1;
  constexpr int V = Vec16<T>::N;
  // chunk grid anchored at the 16-B aligned interior start: x0 <= lox, and x0 >= the -x radius (no cell in front of
  // the row's raw cells is read); the last chunk may reach past hix, up to the row's read limit
  const int rxm = int(dom.radius().x(-1));
  const int off = ((a.lox - rxm) % V + V) % V;
  a.x0 = a.lox - off;
  a.nchunks = (a.hix - a.x0 + V - 1) / V;
  const bool aligned = aligned_vector_layout(dom, qa, a.x0) && (!TWO || aligned_vector_layout(dom, qb, a.x0));
  const bool fits = a.x0 >= 0 && a.x0 + int64_t(a.nchunks) * V <= dom.row_limit(qa);
  // the halo-aligned x layout (set_x_halo_align) is left to the generic kernel, like the unpadded one
  if (aligned && fits && !dom.x_halo_align()) info->path = 2;
  if (maxBlocks > 0) {
    info->blocks = maxBlocks;
  } else {
    dom.set_device();
    const void *kern = info->path == 2 ? (const void *)field_reduce_rows_kernel<T, TWO>
                                       : (const void *)field_reduce_generic_kernel<T, TWO>;
    const int64_t resident = resident_blocks(kern, kReduceThreads, 4);
    info->blocks = std::max<int64_t>(1, std::min(resident, a.nrows));
  }
  return a;
}

template <typename T, bool TWO>
static void reduce_enqueue_t(const LocalDomain &dom, int64_t qa, bool currA, int64_t qb, bool currB, const Rect3 &region,
                             ReduceScratch &scratch, hipStream_t stream, int maxBlocks) {
  ReduceLaunchInfo info;
  ReduceArgs<T> a = reduce_plan<T, TWO>(dom, qa, currA, qb, currB, region, maxBlocks, &info);
  if (info.path == 0) {
    *scratch.result_host() = reduce_host<T, TWO>(a);
    return;
  }
  a.slab = scratch.slab(dom.gpu(), info.blocks);
  dom.set_device();
  if (info.path == 2)
    hipLaunchKernelGGL((field_reduce_rows_kernel<T, TWO>), dim3(uint32_t(info.blocks)), dim3(kReduceThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((field_reduce_generic_kernel<T, TWO>), dim3(uint32_t(info.blocks)), dim3(kReduceThreads), 0, stream, a);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(field_reduce_combine_kernel, dim3(1), dim3(kReduceThreads), 0, stream, a.slab, int(info.blocks),
                     a.count, scratch.result_device());
  HIP_CHECK(hipGetLastError());
}

void field_reduce_enqueue(const LocalDomain &dom, int64_t qa, bool currA, int64_t qb, bool currB, const Rect3 &region,
                          ReduceScratch &scratch, hipStream_t stream, int maxBlocks) {
  const int64_t es = reduce_check(dom, qa, qb, region, maxBlocks);
  if (region.empty()) {
    // the identity, in stream order behind whatever this scratch's result still waits for
    if (dom.backend() == Backend::Host) {
      *scratch.result_host() = FieldStats();
      return;
    }
    FieldStats *slab = scratch.slab(dom.gpu(), 1);
    dom.set_device();
    hipLaunchKernelGGL(field_reduce_combine_kernel, dim3(1), dim3(kReduceThreads), 0, stream, slab, 0, int64_t(0),
                       scratch.result_device());
    HIP_CHECK(hipGetLastError());
    return;
  }
  const bool two = qb >= 0;
  if (es == 4) {
    if (two)
      reduce_enqueue_t<float, true>(dom, qa, currA, qb, currB, region, scratch, stream, maxBlocks);
    else
      reduce_enqueue_t<float, false>(dom, qa, currA, qb, currB, region, scratch, stream, maxBlocks);
  } else {
    if (two)
      reduce_enqueue_t<double, true>(dom, qa, currA, qb, currB, region, scratch, stream, maxBlocks);
    else
      reduce_enqueue_t<double, false>(dom, qa, currA, qb, currB, region, scratch, stream, maxBlocks);
  }
}

FieldStats field_reduce(const LocalDomain &dom, int64_t qa, bool currA, int64_t qb, bool currB, const Rect3 &region,
                        ReduceScratch &scratch, hipStream_t stream, int maxBlocks) {
  field_reduce_enqueue(dom, qa, currA, qb, currB, region, scratch, stream, maxBlocks);
  if (dom.backend() == Backend::Device) {
    dom.set_device();
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  return scratch.result();
}

ReduceLaunchInfo field_reduce_launch_info(const LocalDomain &dom, int64_t qa, bool currA, int64_t qb, bool currB,
                                          const Rect3 &region, int maxBlocks) {
  const int64_t es = reduce_check(dom, qa, qb, region, maxBlocks);
  ReduceLaunchInfo info;
  if (region.empty()) {
    info.path = -1;
    return info;
  }
  const bool two = qb >= 0;
  if (es == 4) {
    if (two)
      reduce_plan<float, true>(dom, qa, currA, qb, currB, region, maxBlocks, &info);
    else
      reduce_plan<float, false>(dom, qa, currA, qb, currB, region, maxBlocks, &info);
  } else {
    if (two)
      reduce_plan<double, true>(dom, qa, currA, qb, currB, region, maxBlocks, &info);
    else
      reduce_plan<double, false>(dom, qa, currA, qb, currB, region, maxBlocks, &info);
  }
  return info;
}

} // namespace stencil
