#pragma once
// A type-converting, scaled field copy between two LocalDomains of the same compute region (field_convert.hip):
//   dst(region) = T_dst( double(scale) * double(src) )
// One product in double, then one conversion to the destination type (round to nearest even, overflow to +-inf,
// subnormals kept), so the result is bitwise equal to stencil2_amd.ops.convert_reference. scale = 1 is an exact cast
// in either direction; NaN and Inf propagate. The element types are fp32 or fp64 on each side, all four combinations:
// with one type on both sides it is a scaled copy under the same rule.
//
// The source is (quantity, curr or next) of srcDom, the destination one of dstDom. Both domains are realized, on the
// same backend and device, with the same compute region (origin and size); radii, pitches, padding and alignment may
// differ: the kernels take both layouts. The two domains may be the same object, but source and destination may not be
// the same (quantity, buffer) of it.
//
// Only cells of `region` (global coordinates, inside the compute region) of dst are written: halos, row padding, the
// guard and every other buffer keep their bytes. The halos of dst are therefore stale afterwards.
//
// With `stats` the same launch accumulates the FieldStats of the values it stored (e = double(v) for v as rounded to
// the destination type, dot = 0) with the accumulators and the combine of field_reduce / field_axpby: no atomics, the
// same call returns the same bits every time.
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "stencil/core/geometry.hpp"
#include "stencil/domain/local_domain.hpp"
#include "stencil/kernels/field_axpby.hpp"
#include "stencil/kernels/field_reduce.hpp"

namespace stencil {

// What field_convert_enqueue would run (nothing is launched; the same refusals raise)
struct ConvertLaunchInfo {
  int path = 0;       // -1 nothing (empty region), 0 host loop, 1 one thread per cell, 2 the row kernel
  int64_t blocks = 0; // blocks of the launch (0: host / empty)
  int64_t items = 0;  // (row, plane) pairs of the region
};

// fp32 / fp64 quantities (or opaque 4- / 8-byte elements, taken as fp32 / fp64) of two realized domains on one backend
// and device with the same compute region, and not the same (domain, quantity): the two buffers of one quantity are
// taken, one buffer onto itself is refused by the enqueue
bool field_convert_supported(const LocalDomain &srcDom, int64_t qsrc, const LocalDomain &dstDom, int64_t qdst);
// Asynchronous on `stream` (Backend::Host: done before the call returns). When both sides are in the aligned vector
// layout the row kernel runs: waves take whole (row, plane) items, a lane owns 4 consecutive cells (one 16-B fp32 chunk,
// two 16-B fp64 chunks), so every access of a wave is one contiguous run on both sides; every load of a lane's batch
// (several rows in flight) is issued before its first store; head and tail chunks of a region off the 4-cell grid are
// loaded whole (inside the source row's read limit) and stored cell by cell for the cells inside only. Any other
// device layout (set_padding(false), set_x_halo_align(true) on either side) runs one thread per cell. maxBlocks and
// stats as in field_axpby_enqueue; the scratch belongs to the destination's device. Refused on the host before any
// launch: other dtypes, domains that differ in backend, device or compute region, a region outside the compute
// region, an unrealized domain, source and destination being the same (domain, quantity, buffer), maxBlocks outside
// [0, 2^20].
void field_convert_enqueue(const LocalDomain &srcDom, FieldRef src, const LocalDomain &dstDom, FieldRef dst, double scale,
                           const Rect3 &region, hipStream_t stream, ReduceScratch *stats = nullptr, int maxBlocks = 0);
ConvertLaunchInfo field_convert_launch_info(const LocalDomain &srcDom, FieldRef src, const LocalDomain &dstDom,
                                            FieldRef dst, double scale, const Rect3 &region, bool stats = false,
                                            int maxBlocks = 0);

} // namespace stencil
