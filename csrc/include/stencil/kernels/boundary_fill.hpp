#pragma once
// Ghost-cell fill for the non-periodic faces of the global grid (boundary_fill.hip): per face and per quantity the
// ghost cells of one LocalDomain are set from a BoundaryConditions (stencil/core/boundary.hpp) after the exchange.
//
// The fill is defined as three passes in the order x, y, z, each over the whole raw extent of the other two axes, on
// top of the exchanged halos. The per-axis maps compose in closed form, so it runs as ONE pass: for a ghost cell
// resolve z, then y, then x --
//   a coordinate beyond a Constant face ends the chain with T(v);
//   beyond a Mirror / AntiMirror face it is replaced by its reflection (2 lo - 1 - c at the low face, 2 hi - 1 - c at
//   the high face, lo / hi the raw coordinates of the interior's first cell / one past its last);
//   a coordinate inside the grid, in an exchanged halo, or (once an earlier axis resolved) beyond an Open face stays;
// then load the source cell and apply the AntiMirror subtractions innermost first (x, then y, then z): v = c - v with
// c = T(2.0 * value), converted once on the host; one subtraction in T rounds once.
// A ghost cell is a raw cell with at least one coordinate beyond a non-periodic, non-Open face of the global grid; the
// first face (z, y, x order) a cell lies beyond decides it, and where that face is Open the cell is left alone. So the
// fill reads only cells that are not ghost cells and writes only ghost cells: one launch needs no ordering between
// its items. A ghost cell whose source is a halo cell the radius does not exchange receives that cell's content.
//
// Paths: Backend::Host the definition cell by cell; device sub-domains in the aligned vector layout (the padded
// layouts with the interior on a 16-B boundary and a 16-B row pitch, not the halo-aligned x layout) the fast kernel;
// every other device layout one thread per ghost cell. All device work of one call is ONE launch of one work-table
// kernel: the ghost cells of every item are cut into at most six disjoint boxes (z slabs over the full raw x and y,
// y slabs over the full raw x and the non-ghost z, x slabs over the non-ghost y and z), a host-built table deals them
// to 256-thread blocks, and quantities of 4- and 8-byte elements are two template instances inside that kernel.
// A call with more than kFillMaxItems items is split into one launch per kFillMaxItems items.
// The table is built and uploaded on the first call with a given item list and kept in the BoundaryFillCache; buffer
// pointers travel by value with every launch (swap() stays a host pointer swap), so later calls allocate, upload and
// synchronise nothing and can be captured on a stream.
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "stencil/core/boundary.hpp"
#include "stencil/domain/local_domain.hpp"

namespace stencil {

constexpr int kFillMaxItems = 16; // buffer pointers passed by value per launch

// one request: fill the ghost cells of quantity q (curr or next buffer) under bc
struct FillRequest {
  int64_t q = 0;
  bool curr = true;
  BoundaryConditions bc;
};

// one axis of one item in raw coordinates: c < lo lies beyond the low physical face, c >= hi beyond the high one
// (lo = 0 / hi = raw extent where this sub-domain does not touch a non-periodic face on that side)
struct FillAxis {
  int lo, hi;
  int kind[2];   // FaceKind of the low / high side (Open where the side is not physical)
  double val[2]; // Constant: T(v); AntiMirror: T(2.0 * v); both widened to double (exact)
};
struct FillItem {
  int slot; // index of the buffer pointer in the launch arguments
  int es;   // 4 or 8
  int64_t px, pxy;
  int raw[3];
  int ilo, ihi; // raw x range of the interior (the 16-B chunk grid of the fast kernel starts at ilo)
  FillAxis ax[3];
};
// a box of ghost cells [lo, hi) in raw coordinates. kind 0: rows (z and y slabs) moved in 16-B chunks over the
// interior's x range, the row ends cell by cell; 1: x slabs, one row per thread (both sides of the row); 2: one thread
// per cell (the generic layouts)
struct FillBox {
  int item, kind;
  int lo[3], hi[3];
};
// the work of one 256-thread block: `count` rows (kinds 0, 1) or cells (kind 2) of `box` from `first` on
struct FillWork {
  uint32_t box, first, count, pad;
};
constexpr uint32_t kFillRowsPerBlock = 4, kFillColsPerBlock = 256, kFillCellsPerBlock = 1024;

struct FillTable {
  std::vector<FillItem> items;
  std::vector<FillBox> boxes;
  std::vector<FillWork> work;
};
// the cells of a box: [lo, hi), less the non-ghost x of a kind 1 box that spans both sides of its rows
inline bool fill_box_holds(const FillTable &t, const FillBox &b, int x, int y, int z) {
  if (x < b.lo[0] || x >= b.hi[0] || y < b.lo[1] || y >= b.hi[1] || z < b.lo[2] || z >= b.hi[2]) return false;
  const FillAxis &X = t.items[size_t(b.item)].ax[0];
  return b.kind != 1 || x < X.lo || x >= X.hi;
}
// host only: the items, disjoint boxes and work table of `reqs` on `dom` (fast: kinds 0 / 1, else kind 2). Requests
// that touch no filled face of this sub-domain produce no item.
FillTable boundary_fill_table(const LocalDomain &dom, const Dim3 &gridSize, const std::vector<FillRequest> &reqs,
                              bool fast);
// the definition, cell by cell, on host memory (`base`: raw [0,0,0] of the buffer); returns true where the cell is
// a ghost cell that the fill writes
bool boundary_fill_cell_host(const FillItem &it, void *base, int x, int y, int z);

// device tables of one sub-domain, keyed by the item list; grown on first use
class BoundaryFillCache {
public:
  BoundaryFillCache() = default;
  ~BoundaryFillCache();
  BoundaryFillCache(const BoundaryFillCache &) = delete;
  BoundaryFillCache &operator=(const BoundaryFillCache &) = delete;
  struct Entry {
    std::string key;
    int dev = -1;
    void *dmem = nullptr; // items, boxes, work in one allocation
    int64_t nitems = 0, nboxes = 0, nwork = 0;
    std::vector<std::pair<uint32_t, uint32_t>> groups; // per launch: [first, last) of the work table
  };
  const Entry *find(const std::string &key) const;
  const Entry &insert(Entry &&e);

private:
  std::vector<Entry> entries_;
};

struct FillLaunchInfo {
  int path = -1;       // -1 none, 0 host loop, 1 one thread per cell, 2 the fast kernel
  int64_t boxes = 0;   // disjoint boxes of ghost cells over all items
  int64_t blocks = 0;  // blocks over all launches (0: host / none)
  int64_t launches = 0;
};

// fp32 / fp64 quantities (or opaque 4- / 8-byte elements, taken as such) of a realized domain whose extent along
// every Mirror / AntiMirror face the sub-domain touches is at least that side's face radius
bool boundary_fill_supported(const LocalDomain &dom, const Dim3 &gridSize, int64_t q, const BoundaryConditions &bc);
// Asynchronous on `stream` (Backend::Host: done before the call returns). One launch for everything `reqs` asks of
// this sub-domain (per kFillMaxItems items); none where it touches no filled face. Refused on the host before any
// launch: an unrealized domain, other dtypes, a quantity index out of range, a mirrored extent below the radius.
void boundary_fill_enqueue(const LocalDomain &dom, const Dim3 &gridSize, const std::vector<FillRequest> &reqs,
                           BoundaryFillCache &cache, hipStream_t stream);
// what boundary_fill_enqueue would run (nothing is launched; the same refusals raise)
FillLaunchInfo boundary_fill_launch_info(const LocalDomain &dom, const Dim3 &gridSize,
                                         const std::vector<FillRequest> &reqs);
// measurement knob: non-temporal stores in the fast kernel's 16-B row chunks (default off: the next sweep reads the
// ghost cells at once, and on one MI355X both measured the same at 256^3 and 512^3; BASELINE.md, "Boundary fill")
void set_boundary_fill_nontemporal(bool on);

} // namespace stencil
