#pragma once
// Linear combinations of fields of one LocalDomain, optionally fused with the reduction of what was stored
// (field_axpby.hip):
//   dst(region) = a * x            (y.q < 0)
//   dst(region) = a * x + b * y
// An operand is (quantity, curr or next), as in field_reduce.hpp. a and b are converted to the element type T once on
// the host; per cell t = a_T * x, s = b_T * y and dst = t + s are each their own rounding in T (no FMA contraction,
// device or host), so the result is bitwise equal to stencil2_amd.ops.axpby_reference. A zero coefficient is
// multiplied like any other (NaN and Inf propagate); a = 1 with no y is an exact copy.
//
// dst may be the same (quantity, buffer) as x, as y or as both, and x may equal y: each cell is loaded by the lane
// that stores it, and every load of a lane's batch is issued before the batch's first store.
//
// Only cells of `region` (global coordinates, inside the compute region) of dst are written: halos, row padding, the
// guard and cells outside a sub-region keep their bytes. The halos of dst are therefore stale afterwards; exchange
// before the next stencil reads them.
//
// With `stats` the same launch accumulates the FieldStats of the values it stored (e = double(v) for v as rounded to
// T, dot = 0) exactly as field_reduce does: double accumulators per lane in a fixed order, the shuffle tree, LDS in
// wave order, one partial per block, the one-block combine launch on the same stream. No atomics: the same call
// returns the same bits every time.
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "stencil/core/geometry.hpp"
#include "stencil/domain/local_domain.hpp"
#include "stencil/kernels/field_reduce.hpp"

namespace stencil {

// one buffer of one quantity; q < 0: no operand
struct FieldRef {
  int64_t q = -1;
  bool curr = true;
  FieldRef() = default;
  FieldRef(int64_t q_, bool curr_ = true) : q(q_), curr(curr_) {}
};

// What field_axpby_enqueue would run (nothing is launched; the same refusals raise)
struct AxpbyLaunchInfo {
  int path = 0;       // -1 nothing (empty region), 0 host loop, 1 one thread per cell, 2 the row kernel
  int64_t blocks = 0; // blocks of the launch (0: host / empty)
  int64_t items = 0;  // (row, plane) pairs of the region
};

// fp32 / fp64 quantities (or opaque 4- / 8-byte elements, taken as fp32 / fp64) of a realized domain, all of the same
// element size and row pitch
bool field_axpby_supported(const LocalDomain &dom, int64_t qdst, int64_t qx, int64_t qy = -1);
// Asynchronous on `stream` (Backend::Host: done before the call returns). Device sub-domains in the aligned vector
// layout run the row kernel: each wave takes whole (row, plane) items in 16-B chunks, several rows in flight; head and
// tail chunks of a region off the chunk grid are loaded whole (inside the row's read limit) and stored cell by cell
// for the cells inside the region only. Any other device layout (set_padding(false), set_x_halo_align(true)) runs one
// thread per cell. maxBlocks: 0 = one round of resident blocks capped by the number of (row, plane) items; otherwise
// exactly that many blocks (blocks without work store the identity partial). stats: the FieldStats of the stored
// values land in stats->result() once the stream has reached the combine launch; null: no slab is touched.
// nontemporal: the row kernel's 16-B stores carry the nt hint. Refused on the host before any launch: other dtypes,
// operands of different element size or row pitch, a region outside the compute region, an unrealized domain,
// maxBlocks outside [0, 2^20].
void field_axpby_enqueue(const LocalDomain &dom, FieldRef dst, double a, FieldRef x, double b, FieldRef y,
                         const Rect3 &region, hipStream_t stream, ReduceScratch *stats = nullptr, int maxBlocks = 0,
                         bool nontemporal = false);
AxpbyLaunchInfo field_axpby_launch_info(const LocalDomain &dom, FieldRef dst, double a, FieldRef x, double b, FieldRef y,
                                        const Rect3 &region, bool stats = false, int maxBlocks = 0,
                                        bool nontemporal = false);

} // namespace stencil
