// Ghost-cell fill for non-periodic faces on gfx950. See stencil/kernels/boundary_fill.hpp for the definition (the
// composed z, y, x map) and the paths.
//   kind 0 boxes (z and y slabs, contiguous rows): a wave takes a row, resolves z and y once for the row (wave-uniform)
//     and moves the chunks over the interior's x range as 16-B loads and stores -- same x, reflected y / z, the
//     AntiMirror subtractions per lane element -- then its first lanes the row's x-halo cells (and the cells of a
//     last partial chunk) one by one through the full map;
//   kind 1 boxes (x slabs, strided columns): one row per lane, both sides of the row;
//   kind 2 boxes (layouts without the 16-B chunk grid): one thread per cell.
// Every block reads its FillWork entry, its box and its item with scalar loads; buffer pointers are kernel arguments.
#include <hip/hip_runtime.h>

#include <cstring>

#include "stencil_common.hpp"
#include "stencil/kernels/boundary_fill.hpp"
#include "stencil/rt/hip_check.hpp"

namespace stencil {

constexpr int kFillThreads = 256, kFillWaves = kFillThreads / 64;
constexpr int kFillChunksInFlight = 4, kFillColBatch = 4;
constexpr int kOpen = int(FaceKind::Open), kConstant = int(FaceKind::Constant), kMirror = int(FaceKind::Mirror),
              kAntiMirror = int(FaceKind::AntiMirror);

struct FillArgs {
  const FillItem *items;
  const FillBox *boxes;
  const FillWork *work;
  char *base[kFillMaxItems];
  int nt;
};

// how the axes from `last` up to z resolve for a cell: the source coordinates, or a constant, and the subtractions
template <typename T> struct FillChain {
  int c[3];
  T cc[3];
  T v;
  unsigned anti = 0;
  bool seen = false, isConst = false, skip = false;
};
// resolve axes 2 .. last (z first) of cell (x, y, z); ch.skip: the first face the cell lies beyond is Open
template <typename T>
__host__ __device__ __forceinline__ void fill_resolve(const FillItem &it, int x, int y, int z, int last, FillChain<T> &ch) {
  ch.c[0] = x;
  ch.c[1] = y;
  ch.c[2] = z;
#pragma unroll
  for (int a = 2; a >= 0; --a) {
    if (a < last || ch.isConst || ch.skip) continue;
    const FillAxis &A = it.ax[a];
    const int side = ch.c[a] < A.lo ? 0 : (ch.c[a] >= A.hi ? 1 : -1);
    if (side < 0) continue;
    const int k = A.kind[side];
    if (k == kOpen) {
      ch.skip = !ch.seen; // beyond an Open face after an earlier axis resolved: the coordinate stays
      continue;
    }
    ch.seen = true;
    if (k == kConstant) {
      ch.v = T(A.val[side]);
      ch.isConst = true;
      continue;
    }
    ch.c[a] = (side == 0 ? 2 * A.lo : 2 * A.hi) - 1 - ch.c[a];
    if (k == kAntiMirror) {
      ch.anti |= 1u << a;
      ch.cc[a] = T(A.val[side]);
    }
  }
}
template <typename T> __host__ __device__ __forceinline__ T fill_subtract(const FillChain<T> &ch, T v) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if ((ch.anti >> a) & 1u) v = ch.cc[a] - v;
  return v;
}
// the whole map for one cell; false: not a ghost cell this item writes
template <typename T>
__host__ __device__ __forceinline__ bool fill_cell(const FillItem &it, T *base, int x, int y, int z) {
  FillChain<T> ch;
  fill_resolve<T>(it, x, y, z, 0, ch);
  if (ch.skip || !ch.seen) return false;
  T v = ch.isConst ? ch.v : base[int64_t(ch.c[2]) * it.pxy + int64_t(ch.c[1]) * it.px + ch.c[0]];
  base[int64_t(z) * it.pxy + int64_t(y) * it.px + x] = fill_subtract<T>(ch, v);
  return true;
}

template <typename T>
__device__ __forceinline__ void fill_rows(const FillItem &it, const FillBox &b, const FillWork &w, T *base, int nt) {
  using NV = typename Vec16<T>::native;
  constexpr int V = Vec16<T>::N;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ny = b.hi[1] - b.lo[1];
  const int nvec = (it.ihi - it.ilo) / V;
  const int xv = it.ilo + nvec * V;         // first cell behind the whole chunks
  const int nend = it.ilo + (it.raw[0] - xv); // cells in front of and behind them
  for (uint32_t r = w.first + uint32_t(wave); r < w.first + w.count; r += kFillWaves) {
    const int y = b.lo[1] + int(r % uint32_t(ny)), z = b.lo[2] + int(r / uint32_t(ny));
    FillChain<T> ch;
    fill_resolve<T>(it, 0, y, z, 1, ch); // z and y: uniform over the row
    if (ch.skip || !ch.seen) continue;   // never for the rows of a kind 0 box
    T *dst = base + int64_t(z) * it.pxy + int64_t(y) * it.px;
    const T *src = base + int64_t(ch.c[2]) * it.pxy + int64_t(ch.c[1]) * it.px;
    // kFillChunksInFlight chunks per lane: every load before the first store (source and ghost rows never overlap)
    for (int c0 = lane; c0 < nvec; c0 += 64 * kFillChunksInFlight) {
      NV v[kFillChunksInFlight];
#pragma unroll
      for (int u = 0; u < kFillChunksInFlight; ++u) {
        const int c = c0 + 64 * u;
        if (c >= nvec) continue;
        if (ch.isConst) {
#pragma unroll
          for (int e = 0; e < V; ++e) v[u][e] = ch.v;
        } else {
          v[u] = *reinterpret_cast<const NV *>(src + it.ilo + c * V);
        }
      }
#pragma unroll
      for (int u = 0; u < kFillChunksInFlight; ++u) {
        const int c = c0 + 64 * u;
        if (c >= nvec) continue;
#pragma unroll
        for (int e = 0; e < V; ++e) v[u][e] = fill_subtract<T>(ch, v[u][e]);
        NV *p = reinterpret_cast<NV *>(dst + it.ilo + c * V);
        if (nt)
          __builtin_nontemporal_store(v[u], p);
        else
          *p = v[u];
      }
    }
    for (int i = lane; i < nend; i += 64) fill_cell<T>(it, base, i < it.ilo ? i : xv + (i - it.ilo), y, z);
  }
}

template <typename T>
__device__ __forceinline__ void fill_cols(const FillItem &it, const FillBox &b, const FillWork &w, T *base) {
  const uint32_t r = w.first + threadIdx.x;
  if (r >= w.first + w.count) return;
  const int ny = b.hi[1] - b.lo[1];
  const int y = b.lo[1] + int(r % uint32_t(ny)), z = b.lo[2] + int(r / uint32_t(ny));
  // y and z of an x slab's rows lie beyond no face, so only x resolves. Side s has the ghost cells [g0, g1) and the
  // mirror cell m[s] - x; batches of kFillColBatch cells per side, every load of both sides before the first store
  const FillAxis &X = it.ax[0];
  T *row = base + int64_t(z) * it.pxy + int64_t(y) * it.px;
  const int g0[2] = {b.lo[0], max(X.hi, b.lo[0])}, g1[2] = {min(X.lo, b.hi[0]), b.hi[0]};
  const int m[2] = {2 * X.lo - 1, 2 * X.hi - 1};
  for (int o = 0; g0[0] + o < g1[0] || g0[1] + o < g1[1]; o += kFillColBatch) {
    T v[2][kFillColBatch];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < kFillColBatch; ++j) {
        const int x = g0[s] + o + j;
        if (x >= g1[s]) continue;
        const int k = X.kind[s];
        const T c = T(X.val[s]);
        T t = k == kConstant ? c : row[m[s] - x];
        v[s][j] = k == kAntiMirror ? c - t : t;
      }
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int j = 0; j < kFillColBatch; ++j) {
        const int x = g0[s] + o + j;
        if (x < g1[s]) row[x] = v[s][j];
      }
  }
}

template <typename T>
__device__ __forceinline__ void fill_cells(const FillItem &it, const FillBox &b, const FillWork &w, T *base) {
  const uint32_t nx = uint32_t(b.hi[0] - b.lo[0]), ny = uint32_t(b.hi[1] - b.lo[1]);
  for (uint32_t i = w.first + threadIdx.x; i < w.first + w.count; i += kFillThreads) {
    const int x = b.lo[0] + int(i % nx), y = b.lo[1] + int((i / nx) % ny), z = b.lo[2] + int(i / (nx * ny));
    fill_cell<T>(it, base, x, y, z);
  }
}

template <typename T>
__device__ __forceinline__ void fill_block(const FillItem &it, const FillBox &b, const FillWork &w, char *base, int nt) {
  T *p = reinterpret_cast<T *>(base);
  if (b.kind == 0)
    fill_rows<T>(it, b, w, p, nt);
  else if (b.kind == 1)
    fill_cols<T>(it, b, w, p);
  else
    fill_cells<T>(it, b, w, p);
}

__global__ __launch_bounds__(kFillThreads) void boundary_fill_kernel(FillArgs a, uint32_t work0) {
  const FillWork w = a.work[work0 + blockIdx.x];
  const FillBox &b = a.boxes[w.box];
  const FillItem &it = a.items[b.item];
  char *base = a.base[it.slot];
  if (it.es == 4)
    fill_block<float>(it, b, w, base, a.nt);
  else
    fill_block<double>(it, b, w, base, a.nt);
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static bool g_fillNontemporal = false;
void set_boundary_fill_nontemporal(bool on) { g_fillNontemporal = on; }

bool boundary_fill_cell_host(const FillItem &it, void *base, int x, int y, int z) {
  return it.es == 4 ? fill_cell<float>(it, static_cast<float *>(base), x, y, z)
                    : fill_cell<double>(it, static_cast<double *>(base), x, y, z);
}

static bool filled_kind(int k) { return k == kConstant || k == kMirror || k == kAntiMirror; }

// the item of one request; false: the sub-domain touches no face the request fills. why != null: refusals are
// reported there instead of thrown (boundary_fill_supported)
static bool make_fill_item(const LocalDomain &dom, const Dim3 &grid, const FillRequest &rq, FillItem &it, std::string *why) {
  auto refuse = [&](const std::string &m) {
    if (why) {
      *why = m;
      return;
    }
    STENCIL_REQUIRE(false, m);
  };
  if (!dom.realized()) {
    refuse("boundary fill of an unrealized domain");
    return false;
  }
  if (rq.q < 0 || rq.q >= dom.num_data()) {
    refuse("boundary fill: quantity " + std::to_string(rq.q) + " of " + std::to_string(dom.num_data()));
    return false;
  }
  rq.bc.validate();
  it = FillItem{};
  const Dim3 raw = dom.raw_size(), o = dom.origin(), s = dom.size(), p = dom.pitch(rq.q);
  const Radius &rad = dom.radius();
  const int64_t org[3] = {o.x, o.y, o.z}, sz[3] = {s.x, s.y, s.z}, g[3] = {grid.x, grid.y, grid.z};
  const int64_t rw[3] = {raw.x, raw.y, raw.z};
  const int64_t rlo[3] = {rad.x(-1), rad.y(-1), rad.z(-1)}, rhi[3] = {rad.x(1), rad.y(1), rad.z(1)};
  it.es = int(dom.elem_size(rq.q));
  it.px = p.x;
  it.pxy = p.x * p.y;
  it.ilo = int(rlo[0]);
  it.ihi = int(rlo[0] + sz[0]);
  bool any = false;
  for (int a = 0; a < 3; ++a) {
    FillAxis &A = it.ax[a];
    it.raw[a] = int(rw[a]);
    A.lo = 0;
    A.hi = int(rw[a]);
    A.kind[0] = A.kind[1] = kOpen;
    A.val[0] = A.val[1] = 0;
    for (int side = 0; side < 2; ++side) {
      const FaceCondition &fc = rq.bc.at(a, side);
      if (fc.kind == FaceKind::Periodic) continue;
      const bool physical = side == 0 ? org[a] == 0 : org[a] + sz[a] == g[a];
      const int64_t r = side == 0 ? rlo[a] : rhi[a];
      if (!physical || r == 0) continue;
      if (side == 0)
        A.lo = int(rlo[a]);
      else
        A.hi = int(rlo[a] + sz[a]);
      A.kind[side] = int(fc.kind);
      if (!filled_kind(A.kind[side])) continue;
      any = true;
      if ((fc.kind == FaceKind::Mirror || fc.kind == FaceKind::AntiMirror) && sz[a] < r) {
        refuse("boundary fill: the sub-domain is " + std::to_string(sz[a]) + " cells thin along axis " + std::to_string(a) +
               ", below the face radius " + std::to_string(r) + " of its mirrored face");
        return false;
      }
      const double v = fc.kind == FaceKind::AntiMirror ? 2.0 * fc.value : fc.value;
      A.val[side] = it.es == 4 ? double(float(v)) : v; // converted to T once, here
    }
  }
  if (!any) return false;
  int64_t es = 0;
  if (!fp_quantity(dom, rq.q, &es)) {
    refuse("boundary fills take fp32 / fp64 quantities (quantity " + std::to_string(rq.q) +
           "): give it Open faces with set_boundary_conditions(q, ...)");
    return false;
  }
  return true;
}

static bool fill_fast_layout(const LocalDomain &dom, int64_t q) {
  return dom.backend() == Backend::Device && !dom.x_halo_align() && aligned_vector_layout(dom, q, dom.radius().x(-1));
}

FillTable boundary_fill_table(const LocalDomain &dom, const Dim3 &gridSize, const std::vector<FillRequest> &reqs,
                              bool fast) {
  FillTable t;
  for (const FillRequest &rq : reqs) {
    FillItem it;
    if (!make_fill_item(dom, gridSize, rq, it, nullptr)) continue;
    const int item = int(t.items.size());
    it.slot = item % kFillMaxItems;
    t.items.push_back(it);
    auto add = [&](int kind, int x0, int x1, int y0, int y1, int z0, int z1) {
      if (x1 <= x0 || y1 <= y0 || z1 <= z0) return;
      FillBox b{};
      b.item = item;
      b.kind = fast ? kind : 2;
      b.lo[0] = x0, b.lo[1] = y0, b.lo[2] = z0;
      b.hi[0] = x1, b.hi[1] = y1, b.hi[2] = z1;
      const uint32_t box = uint32_t(t.boxes.size());
      t.boxes.push_back(b);
      const uint64_t rows = uint64_t(y1 - y0) * uint64_t(z1 - z0);
      const uint64_t n = b.kind == 2 ? rows * uint64_t(x1 - x0) : rows;
      const uint64_t per = b.kind == 0 ? kFillRowsPerBlock : (b.kind == 1 ? kFillColsPerBlock : kFillCellsPerBlock);
      STENCIL_REQUIRE(n < (uint64_t(1) << 32), "boundary fill: box of " << n << " items");
      for (uint64_t f = 0; f < n; f += per) t.work.push_back(FillWork{box, uint32_t(f), uint32_t(std::min(per, n - f)), 0});
    };
    const FillAxis &X = it.ax[0], &Y = it.ax[1], &Z = it.ax[2];
    const bool xl = filled_kind(X.kind[0]) && X.lo > 0, xh = filled_kind(X.kind[1]) && X.hi < it.raw[0];
    // z slabs: the full raw x and y
    if (filled_kind(Z.kind[0])) add(0, 0, it.raw[0], 0, it.raw[1], 0, Z.lo);
    if (filled_kind(Z.kind[1])) add(0, 0, it.raw[0], 0, it.raw[1], Z.hi, it.raw[2]);
    // y slabs: the full raw x, the non-ghost z
    if (filled_kind(Y.kind[0])) add(0, 0, it.raw[0], 0, Y.lo, Z.lo, Z.hi);
    if (filled_kind(Y.kind[1])) add(0, 0, it.raw[0], Y.hi, it.raw[1], Z.lo, Z.hi);
    // x slabs: the non-ghost y and z; the fast kernel takes both sides of a row in one item
    if (fast && xl && xh) {
      add(1, 0, it.raw[0], Y.lo, Y.hi, Z.lo, Z.hi);
    } else {
      if (xl) add(1, 0, X.lo, Y.lo, Y.hi, Z.lo, Z.hi);
      if (xh) add(1, X.hi, it.raw[0], Y.lo, Y.hi, Z.lo, Z.hi);
    }
  }
  return t;
}

BoundaryFillCache::~BoundaryFillCache() {
  for (Entry &e : entries_)
    if (e.dmem) {
      (void)hipSetDevice(e.dev);
      (void)hipFree(e.dmem);
    }
}
const BoundaryFillCache::Entry *BoundaryFillCache::find(const std::string &key) const {
  for (const Entry &e : entries_)
    if (e.key == key) return &e;
  return nullptr;
}
const BoundaryFillCache::Entry &BoundaryFillCache::insert(Entry &&e) {
  entries_.push_back(std::move(e));
  return entries_.back();
}

// what identifies a table: the quantities and their conditions (not curr / next: the pointers travel by value)
static std::string fill_key(const std::vector<FillRequest> &reqs) {
  std::string k;
  for (const FillRequest &rq : reqs) {
    k.append(reinterpret_cast<const char *>(&rq.q), sizeof(rq.q));
    for (int a = 0; a < 3; ++a)
      for (int s = 0; s < 2; ++s) {
        const FaceCondition &fc = rq.bc.at(a, s);
        const int kind = int(fc.kind);
        k.append(reinterpret_cast<const char *>(&kind), sizeof(kind));
        k.append(reinterpret_cast<const char *>(&fc.value), sizeof(fc.value));
      }
  }
  return k;
}

// the items' requests (in item order) and whether every item has the fast layout
static bool fill_plan(const LocalDomain &dom, const Dim3 &grid, const std::vector<FillRequest> &reqs, std::vector<int> &req) {
  bool fast = true;
  req.clear();
  for (size_t i = 0; i < reqs.size(); ++i) {
    FillItem it;
    if (!make_fill_item(dom, grid, reqs[i], it, nullptr)) continue;
    req.push_back(int(i));
    fast = fast && fill_fast_layout(dom, reqs[i].q);
  }
  return fast;
}

bool boundary_fill_supported(const LocalDomain &dom, const Dim3 &gridSize, int64_t q, const BoundaryConditions &bc) {
  FillRequest rq;
  rq.q = q;
  rq.bc = bc;
  FillItem it;
  std::string why;
  try {
    make_fill_item(dom, gridSize, rq, it, &why);
  } catch (const std::exception &) {
    return false;
  }
  return why.empty();
}

// groups of at most kFillMaxItems items: [first, last) of the work table (entries are in item order)
static std::vector<std::pair<uint32_t, uint32_t>> fill_groups(const FillTable &t) {
  std::vector<std::pair<uint32_t, uint32_t>> g;
  const size_t ngroups = (t.items.size() + kFillMaxItems - 1) / kFillMaxItems;
  size_t w = 0;
  for (size_t gi = 0; gi < ngroups; ++gi) {
    const size_t w0 = w;
    while (w < t.work.size() && size_t(t.boxes[t.work[w].box].item) / kFillMaxItems == gi) ++w;
    if (w > w0) g.emplace_back(uint32_t(w0), uint32_t(w));
  }
  return g;
}

FillLaunchInfo boundary_fill_launch_info(const LocalDomain &dom, const Dim3 &gridSize,
                                         const std::vector<FillRequest> &reqs) {
  std::vector<int> req;
  const bool fast = fill_plan(dom, gridSize, reqs, req);
  FillLaunchInfo info;
  if (req.empty()) return info;
  const FillTable t = boundary_fill_table(dom, gridSize, reqs, fast);
  info.boxes = int64_t(t.boxes.size());
  if (dom.backend() == Backend::Host) {
    info.path = 0;
    return info;
  }
  info.path = fast ? 2 : 1;
  info.blocks = int64_t(t.work.size());
  info.launches = int64_t(fill_groups(t).size());
  return info;
}

void boundary_fill_enqueue(const LocalDomain &dom, const Dim3 &gridSize, const std::vector<FillRequest> &reqs,
                           BoundaryFillCache &cache, hipStream_t stream) {
  std::vector<int> req;
  const bool fast = fill_plan(dom, gridSize, reqs, req); // every refusal, before anything is written
  if (req.empty()) return;
  auto base_of = [&](int ri) {
    const FillRequest &rq = reqs[size_t(ri)];
    return static_cast<char *>(rq.curr ? dom.curr_data(rq.q) : dom.next_data(rq.q));
  };
  if (dom.backend() == Backend::Host) {
    for (int ri : req) {
      FillItem it;
      make_fill_item(dom, gridSize, reqs[size_t(ri)], it, nullptr);
      char *base = base_of(ri);
      for (int z = 0; z < it.raw[2]; ++z)
        for (int y = 0; y < it.raw[1]; ++y)
          for (int x = 0; x < it.raw[0]; ++x) boundary_fill_cell_host(it, base, x, y, z);
    }
    return;
  }
  const std::string key = fill_key(reqs);
  const BoundaryFillCache::Entry *e = cache.find(key);
  dom.set_device();
  if (!e) {
    const FillTable t = boundary_fill_table(dom, gridSize, reqs, fast);
    BoundaryFillCache::Entry ne;
    ne.key = key;
    ne.dev = dom.gpu();
    ne.nitems = int64_t(t.items.size());
    ne.nboxes = int64_t(t.boxes.size());
    ne.nwork = int64_t(t.work.size());
    ne.groups = fill_groups(t);
    const size_t bi = t.items.size() * sizeof(FillItem), bb = t.boxes.size() * sizeof(FillBox),
                 bw = t.work.size() * sizeof(FillWork);
    std::vector<char> host(bi + bb + bw);
    std::memcpy(host.data(), t.items.data(), bi);
    std::memcpy(host.data() + bi, t.boxes.data(), bb);
    std::memcpy(host.data() + bi + bb, t.work.data(), bw);
    HIP_CHECK(hipMalloc(&ne.dmem, host.size()));
    HIP_CHECK(hipMemcpy(ne.dmem, host.data(), host.size(), hipMemcpyHostToDevice));
    e = &cache.insert(std::move(ne));
  }
  STENCIL_REQUIRE(size_t(e->nitems) == req.size(), "boundary fill: cached table of " << e->nitems << " items for "
                                                                                       << req.size());
  FillArgs a{};
  char *d = static_cast<char *>(e->dmem);
  a.items = reinterpret_cast<const FillItem *>(d);
  a.boxes = reinterpret_cast<const FillBox *>(d + size_t(e->nitems) * sizeof(FillItem));
  a.work = reinterpret_cast<const FillWork *>(d + size_t(e->nitems) * sizeof(FillItem) + size_t(e->nboxes) * sizeof(FillBox));
  a.nt = g_fillNontemporal ? 1 : 0;
  for (size_t gi = 0; gi < e->groups.size(); ++gi) {
    // every item has work, so group gi holds the items from gi * kFillMaxItems on; slot = item index modulo the group
    for (int s = 0; s < kFillMaxItems; ++s) a.base[s] = nullptr;
    const size_t g = gi * size_t(kFillMaxItems);
    for (size_t i = g; i < std::min(req.size(), g + size_t(kFillMaxItems)); ++i) a.base[i % kFillMaxItems] = base_of(req[i]);
    const uint32_t w0 = e->groups[gi].first, n = e->groups[gi].second - w0;
    hipLaunchKernelGGL(boundary_fill_kernel, dim3(n), dim3(kFillThreads), 0, stream, a, w0);
    HIP_CHECK(hipGetLastError());
  }
}

} // namespace stencil
