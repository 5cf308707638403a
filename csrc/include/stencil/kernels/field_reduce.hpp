#pragma once
// Read-only reductions over one quantity (or the difference and dot product of two) of one LocalDomain:
// count, non-finite cells, sum, sum of magnitudes, sum of squares, min, max and dot (field_reduce.hip).
//
// An operand is (quantity, curr or next). With one operand a, e = double(a); with two, e = double(a) - double(b)
// (exact for fp32, one IEEE rounding for fp64) and dot = sum of double(a) * double(b). Everything accumulates in
// double. Only cells of `region` (global coordinates, inside the compute region) are read for their value: halos, row
// padding, the guard and cells outside a sub-region never influence the result.
//
// Reproducible: no floating-point atomics; which lane and block reduces which cell and the order in which partials are
// combined depend only on the layout, the region and the launch shape (blocks), never on timing, so the same call
// returns the same bits every time. The summation order itself is not part of the contract (it differs between the
// host loop, the generic kernel, the fast kernel and between grids).
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <limits>

#include "stencil/core/geometry.hpp"
#include "stencil/domain/local_domain.hpp"

namespace stencil {

struct FieldStats {
  int64_t count = 0;     // cells reduced
  int64_t nonfinite = 0; // cells whose e is NaN or +-Inf
  double sum = 0, sum_abs = 0, sum_sq = 0; // sum of e, |e|, e * e
  double min = std::numeric_limits<double>::infinity();  // over the cells whose e is not NaN (Inf takes part);
  double max = -std::numeric_limits<double>::infinity(); // the sign of a zero min / max is unspecified
  double dot = 0; // sum of a * b with two operands, 0 with one
  // count / nonfinite / sums / dot added, min / max combined
  void merge(const FieldStats &o) {
    count += o.count;
    nonfinite += o.nonfinite;
    sum += o.sum;
    sum_abs += o.sum_abs;
    sum_sq += o.sum_sq;
    dot += o.dot;
    min = o.min < min ? o.min : min;
    max = o.max > max ? o.max : max;
  }
};
static_assert(sizeof(FieldStats) == 64, "FieldStats is the device partial: 8 words of 8 bytes");

// The per-block partial slab (device memory) and the pinned host result of reductions on one device; allocated on
// first use and grown as needed. One reduction may be in flight per scratch object: the result is valid once the stream
// has reached the reduction, and the next enqueue overwrites it.
class ReduceScratch {
public:
  ReduceScratch() = default;
  ~ReduceScratch();
  ReduceScratch(const ReduceScratch &) = delete;
  ReduceScratch &operator=(const ReduceScratch &) = delete;
  const FieldStats &result() const { return host_ ? *host_ : hostOnly_; }
  // device backend: the slab of at least `blocks` partials on device `dev` and the result word (device pointer of
  // the pinned host struct); dev < 0 (host backend): only the plain host result
  FieldStats *slab(int dev, int64_t blocks);
  FieldStats *result_device() const { return hostDev_; }
  FieldStats *result_host() { return host_ ? host_ : &hostOnly_; }

private:
  void release();
  int dev_ = -1;
  int64_t cap_ = 0;
  FieldStats *slab_ = nullptr;
  FieldStats *host_ = nullptr, *hostDev_ = nullptr;
  FieldStats hostOnly_;
};

// What field_reduce_enqueue would run (nothing is launched; the same refusals raise)
struct ReduceLaunchInfo {
  int path = 0;       // -1 nothing (empty region), 0 host loop, 1 one thread per cell, 2 the row kernel
  int64_t blocks = 0; // blocks of the reduction launch (0: host / empty)
  int64_t items = 0;  // (row, plane) pairs of the region
};

// fp32 / fp64 quantities (or opaque 4- / 8-byte elements, taken as fp32 / fp64) of a realized domain; with a second
// operand (qb >= 0) both of the same type and element size
bool field_reduce_supported(const LocalDomain &dom, int64_t qa, int64_t qb = -1);
// Asynchronous: the reduction of `region` is enqueued on `stream` and lands in scratch.result() once the stream has
// reached it (Backend::Host: computed before the call returns). qb = -1: one operand. Device sub-domains in the
// aligned vector layout (stencil7_apply's predicate: the padded layouts with the interior on a 64- / 128-B unit) run
// the row kernel: each wave takes whole rows in 16-B chunks, rows dealt round-robin to the waves of the grid, head and
// tail chunks of a region off the chunk grid masked per cell; any other device layout (set_padding(false),
// set_x_halo_align(true)) one thread per cell. Each block stores one partial; a second one-block launch on the same
// stream combines them in a fixed tree. maxBlocks: 0 = one round of resident blocks (occupancy query) capped by the
// number of (row, plane) items; otherwise exactly that many blocks (blocks without work store the identity).
// Refused on the host before any launch: other dtypes, operands of different type or size, a region outside the
// compute region, an unrealized domain.
void field_reduce_enqueue(const LocalDomain &dom, int64_t qa, bool currA, int64_t qb, bool currB, const Rect3 &region,
                          ReduceScratch &scratch, hipStream_t stream, int maxBlocks = 0);
// Blocking: enqueue on `stream`, wait for it, return the result
FieldStats field_reduce(const LocalDomain &dom, int64_t qa, bool currA, int64_t qb, bool currB, const Rect3 &region,
                        ReduceScratch &scratch, hipStream_t stream = nullptr, int maxBlocks = 0);
ReduceLaunchInfo field_reduce_launch_info(const LocalDomain &dom, int64_t qa, bool currA, int64_t qb, bool currB,
                                          const Rect3 &region, int maxBlocks = 0);

} // namespace stencil
