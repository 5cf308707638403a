#pragma once
// Grid transfer between two resolutions (grid_transfer.hip): cell-centred coarsening by a factor of 2, the pair of
// operators of a geometric multigrid cycle. The fine sub-domain F has compute-region origin o and size s, all six
// numbers even; the coarse sub-domain C has origin o / 2 and size s / 2, sits on the same device and backend and has
// the same element type T (fp32 or fp64). The walls of boundary_fill lie between the last interior cell and the first
// ghost cell, so the coarse grid's walls sit where the fine grid's do. F and C belong to two DistributedDomains.
//
// Restriction, for coarse cell (K, J, I), every sum rounded on its own in T, no halo read:
//   sx(dz, dy) = f(2K + dz, 2J + dy, 2I) + f(2K + dz, 2J + dy, 2I + 1)
//   sy(dz)     = sx(dz, 0) + sx(dz, 1)
//   c          = T(0.125) * (sy(0) + sy(1))
//
// Prolongation is trilinear and separable, x, then y, then z. Along an axis the fine index i = 2I + p has near = I
// and far = I - 1 (p = 0) or I + 1 (p = 1), and the interpolated value is T(0.75) * near + T(0.25) * far: two
// products and one sum, each rounded on its own in T (no FMA contraction, device or host):
//   tx(K', J') = 0.75 c(K', J', near_x) + 0.25 c(K', J', far_x)
//   ty(K')     = 0.75 tx(K', near_y)    + 0.25 tx(K', far_y)
//   v          = 0.75 ty(near_z)        + 0.25 ty(far_z)
// then dst = v, or with `add` (add.q >= 0) dst = add + v: one more rounded sum, add the left operand. `add` is a
// buffer of the fine domain and may be the same (quantity, buffer) as dst: the correction u <- u + P e. far reaches
// one cell into the coarse halos in all 26 directions: every direction radius of C must be >= 1 and its halos valid
// (exchange, then apply_boundary); walls need no case in the kernel.
//
// Both results are bitwise equal to stencil2_amd.ops.restrict_reference / prolong_reference. Only the cells of the
// region (global coordinates of the destination grid, inside its compute region) are written: halos, padding and
// every other byte of the destination buffer keep their bytes.
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "stencil/core/geometry.hpp"
#include "stencil/domain/local_domain.hpp"
#include "stencil/kernels/field_axpby.hpp"

namespace stencil {

// What grid_restrict_enqueue / grid_prolong_enqueue would run (nothing is launched; the same refusals raise)
struct TransferLaunchInfo {
  int path = 0;       // -1 nothing (empty region), 0 host loop, 1 one thread per destination cell, 2 the chunk kernel
  int64_t blocks = 0; // blocks of the launch (0: host / empty)
  int64_t items = 0;  // wave items: coarse (row, plane) pairs (restriction); (64 fine chunks, coarse row, z chunk)
                      // triples (prolongation)
  int zchunk = 0;     // coarse planes a prolongation wave marches (path 2; else 0)
};

// fp32 / fp64 quantities (or opaque 4- / 8-byte elements) of one element size in two realized sub-domains, the coarse
// one the factor-2 image of the fine one on the same device and backend
bool grid_transfer_supported(const LocalDomain &fine, int64_t qf, const LocalDomain &coarse, int64_t qc);

// coarse dst(coarseRegion) = R fine src. Asynchronous on `stream` (Backend::Host: done before the call returns).
// Device sub-domains in the aligned vector layout run the chunk kernel: a lane loads 2 x 16 B from each of 4 fine rows
// (2 rows x 2 planes) and stores one 16-B coarse chunk; chunks that reach outside the region are loaded whole (inside
// the rows' read limit) and stored cell by cell for the cells inside only. Any other device layout runs one thread per
// coarse cell. Refused on the host before any launch: dtypes other than fp32 / fp64, different element types,
// origins or sizes that are not the factor-2 image of each other, different devices or backends, a region outside the
// coarse compute region, an unrealized domain.
void grid_restrict_enqueue(const LocalDomain &fine, FieldRef src, const LocalDomain &coarse, FieldRef dst,
                           const Rect3 &coarseRegion, hipStream_t stream);
TransferLaunchInfo grid_restrict_launch_info(const LocalDomain &fine, FieldRef src, const LocalDomain &coarse,
                                             FieldRef dst, const Rect3 &coarseRegion);

// fine dst(fineRegion) = P coarse src, or add + P coarse src. Asynchronous on `stream` (Backend::Host: done before the
// call returns). The chunk kernel of the aligned vector layout: a lane owns one 16-B fine chunk per fine row, that is
// the 8 B of the coarse row under it, so every fine access of a wave is one contiguous run. It marches `zchunk` coarse
// planes of one coarse row (0: chosen by the launch), keeping the x- and y-interpolated rows of planes K - 1, K, K + 1
// in registers; the x neighbours of its coarse cells come from the adjacent lanes (the cell beyond a wave's end is
// loaded), the y neighbours from the lane's own loads of rows J - 1 and J + 1. Per coarse plane it writes two fine
// planes x two fine rows as 16-B stores, every `add` chunk loaded by the lane that stores it and before that store.
// Fine regions off the chunk grid (odd starts and ends included) are stored cell by cell. Refused as above, plus a
// coarse direction radius of 0, an `add` of another element type and zchunk < 0.
void grid_prolong_enqueue(const LocalDomain &coarse, FieldRef src, const LocalDomain &fine, FieldRef dst, FieldRef add,
                          const Rect3 &fineRegion, hipStream_t stream, int zchunk = 0);
TransferLaunchInfo grid_prolong_launch_info(const LocalDomain &coarse, FieldRef src, const LocalDomain &fine,
                                            FieldRef dst, FieldRef add, const Rect3 &fineRegion, int zchunk = 0);

} // namespace stencil
