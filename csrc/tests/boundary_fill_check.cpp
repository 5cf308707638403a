// Stand-alone host check of the boundary fill's index arithmetic (stencil/kernels/boundary_fill.hpp): the host loop and
// the box / work-table builder on host-backend LocalDomains, over radii 1-3, an asymmetric radius, a sub-domain
// exactly r wide, sub-domains that touch one face of an axis only, and the shared-halo-line / unpadded layouts.
//   1. every ghost cell (as the host loop decides it) lies in exactly one box, and no box holds another cell;
//   2. the work table covers every row / cell of every box exactly once;
//   3. the host loop equals sequential padding x, y, z of the same buffer, and writes nothing outside the raw cells.
// Built for the CPU (it launches nothing); ci/sanitize.sh runs it under ASan + UBSan.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "stencil/kernels/boundary_fill.hpp"

using namespace stencil;

static int g_failed = 0;
#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      ++g_failed;                                                                                                      \
      std::printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond);                                                  \
      std::printf(__VA_ARGS__);                                                                                        \
      std::printf("\n");                                                                                               \
    }                                                                                                                  \
  } while (0)

static uint32_t g_seed = 12345;
static uint32_t next_u32() { return g_seed = g_seed * 1664525u + 1013904223u; }

static FaceCondition random_cond(bool allowOpen) {
  const double v = double(next_u32() % 1000) / 250.0 - 2.0;
  switch (next_u32() % (allowOpen ? 4 : 3)) {
  case 0: return FaceCondition::constant(v);
  case 1: return FaceCondition::mirror();
  case 2: return FaceCondition::antimirror(v);
  default: return FaceCondition::open();
  }
}

// sequential padding x, y, z on the raw buffer (T = float or double); cells beyond Open faces are left alone
template <typename T> static void pad_sequential(const FillItem &it, T *base) {
  const int n[3] = {it.raw[0], it.raw[1], it.raw[2]};
  for (int a = 0; a < 3; ++a) {
    const FillAxis &A = it.ax[a];
    for (int z = 0; z < n[2]; ++z)
      for (int y = 0; y < n[1]; ++y)
        for (int x = 0; x < n[0]; ++x) {
          int c[3] = {x, y, z};
          const int side = c[a] < A.lo ? 0 : (c[a] >= A.hi ? 1 : -1);
          if (side < 0) continue;
          const int k = A.kind[side];
          const int64_t dst = int64_t(z) * it.pxy + int64_t(y) * it.px + x;
          if (k == int(FaceKind::Constant)) {
            base[dst] = T(A.val[side]);
          } else if (k == int(FaceKind::Mirror) || k == int(FaceKind::AntiMirror)) {
            c[a] = (side == 0 ? 2 * A.lo : 2 * A.hi) - 1 - c[a];
            const T m = base[int64_t(c[2]) * it.pxy + int64_t(c[1]) * it.px + c[0]];
            base[dst] = k == int(FaceKind::Mirror) ? m : T(A.val[side]) - m;
          }
        }
  }
}

struct Case {
  Dim3 grid, origin, size;
  Radius radius;
  bool pad = true, shared = false;
  bool fp64 = false;
  bool allowOpen = false;
};

static void run_case(const Case &cs, int idx) {
  LocalDomain dom(cs.size, cs.origin, -1, Backend::Host);
  dom.set_radius(cs.radius);
  dom.set_padding(cs.pad);
  dom.set_shared_halo_line(cs.shared);
  const int64_t q = cs.fp64 ? dom.add_data<double>("u").id() : dom.add_data<float>("u").id();
  dom.realize();
  FillRequest rq;
  rq.q = q;
  for (int a = 0; a < 3; ++a) rq.bc.set_axis(a, random_cond(cs.allowOpen), random_cond(cs.allowOpen));
  const std::vector<FillRequest> reqs{rq};
  const Dim3 raw = dom.raw_size();
  const int64_t es = dom.elem_size(q);
  const int64_t bytes = dom.buffer_bytes(q);
  const int64_t frontBytes = dom.pad_x(q) * es;

  for (int fast = 0; fast < 2; ++fast) {
    const FillTable t = boundary_fill_table(dom, cs.grid, reqs, fast != 0);
    if (t.items.empty()) continue;
    CHECK(t.boxes.size() <= 6, "case %d: %zu boxes", idx, t.boxes.size());
    const FillItem &it = t.items[0];
    // 1. ghost cells against boxes. The host loop runs on a scratch copy and tells which cells it writes.
    std::vector<char> scratch(dom.buffer_to_host(q, true).size() + 64, 0);
    void *sbase = scratch.data() + frontBytes;
    int64_t ghosts = 0;
    for (int z = 0; z < raw.z; ++z)
      for (int y = 0; y < raw.y; ++y)
        for (int x = 0; x < raw.x; ++x) {
          const bool ghost = boundary_fill_cell_host(it, sbase, x, y, z);
          int holds = 0;
          for (const FillBox &b : t.boxes) holds += fill_box_holds(t, b, x, y, z) ? 1 : 0;
          ghosts += ghost ? 1 : 0;
          CHECK(holds == (ghost ? 1 : 0), "case %d fast %d: cell (%d, %d, %d) ghost %d in %d boxes", idx, fast, x, y, z,
                int(ghost), holds);
        }
    CHECK(ghosts > 0, "case %d: no ghost cell", idx);
    // 2. the work table covers every box item once
    for (size_t bi = 0; bi < t.boxes.size(); ++bi) {
      const FillBox &b = t.boxes[bi];
      CHECK(b.lo[0] >= 0 && b.lo[1] >= 0 && b.lo[2] >= 0 && b.hi[0] <= raw.x && b.hi[1] <= raw.y && b.hi[2] <= raw.z,
            "case %d: box %zu leaves the raw cells", idx, bi);
      const uint64_t rows = uint64_t(b.hi[1] - b.lo[1]) * uint64_t(b.hi[2] - b.lo[2]);
      const uint64_t n = b.kind == 2 ? rows * uint64_t(b.hi[0] - b.lo[0]) : rows;
      uint64_t nextFirst = 0;
      for (const FillWork &w : t.work) {
        if (w.box != bi) continue;
        CHECK(w.first == nextFirst && w.count > 0, "case %d: work of box %zu not contiguous", idx, bi);
        nextFirst = uint64_t(w.first) + w.count;
      }
      CHECK(nextFirst == n, "case %d: work of box %zu covers %llu of %llu", idx, bi, (unsigned long long)nextFirst,
            (unsigned long long)n);
    }
  }

  // 3. the enqueue's host loop on the real buffer against sequential padding, and nothing outside the raw cells
  {
    FillItem it;
    const FillTable t = boundary_fill_table(dom, cs.grid, reqs, false);
    if (t.items.empty()) return;
    it = t.items[0];
    char *curr = static_cast<char *>(dom.curr_data(q));
    // a sentinel byte pattern in every byte of the buffer (padding and tail included), seeded raw cells
    dom.fill_bytes(q, 0xAB, true, true);
    for (int z = 0; z < raw.z; ++z)
      for (int y = 0; y < raw.y; ++y)
        for (int x = 0; x < raw.x; ++x) {
          const int64_t o = int64_t(z) * it.pxy + int64_t(y) * it.px + x;
          const double v = double(next_u32() % 100000) / 100000.0;
          if (cs.fp64)
            reinterpret_cast<double *>(curr)[o] = v;
          else
            reinterpret_cast<float *>(curr)[o] = float(v);
        }
    const std::vector<unsigned char> before = dom.buffer_to_host(q, true), beforeNext = dom.buffer_to_host(q, false);
    CHECK(int64_t(before.size()) >= bytes, "case %d: buffer_to_host %zu < %lld", idx, before.size(), (long long)bytes);
    std::vector<unsigned char> want = before;
    if (cs.fp64)
      pad_sequential<double>(it, reinterpret_cast<double *>(want.data() + frontBytes));
    else
      pad_sequential<float>(it, reinterpret_cast<float *>(want.data() + frontBytes));
    BoundaryFillCache cache;
    boundary_fill_enqueue(dom, cs.grid, reqs, cache, nullptr);
    const std::vector<unsigned char> after = dom.buffer_to_host(q, true);
    CHECK(dom.buffer_to_host(q, false) == beforeNext, "case %d: next changed", idx);
    // with Open faces the one-pass rule leaves more cells alone than sequential passes would (header): bitwise equality
    // with sequential padding holds for the other kinds
    if (!cs.allowOpen) CHECK(after == want, "case %d: host loop differs from sequential padding", idx);
    // cells the definition does not write, and every padding byte, are unchanged
    std::vector<char> probe(before.size() + 64, 0);
    int64_t changedOutside = 0;
    std::vector<char> isGhost(before.size(), 0);
    for (int z = 0; z < raw.z; ++z)
      for (int y = 0; y < raw.y; ++y)
        for (int x = 0; x < raw.x; ++x)
          if (boundary_fill_cell_host(it, probe.data() + frontBytes, x, y, z)) {
            const int64_t o = frontBytes + (int64_t(z) * it.pxy + int64_t(y) * it.px + x) * es;
            for (int64_t b = 0; b < es; ++b) isGhost.at(size_t(o + b)) = 1;
          }
    for (size_t b = 0; b < before.size(); ++b)
      if (!isGhost[b] && after[b] != before[b]) ++changedOutside;
    CHECK(changedOutside == 0, "case %d: %lld bytes outside the ghost cells changed", idx, (long long)changedOutside);
  }
}

int main() {
  std::vector<Case> cases;
  for (int fp64 = 0; fp64 < 2; ++fp64) {
    for (int r = 1; r <= 3; ++r) {
      Case c;
      c.fp64 = fp64 != 0;
      c.radius = Radius::face_edge_corner(r, 0, 0);
      // the whole grid in one sub-domain
      c.grid = c.size = Dim3(11, 6, 5);
      c.origin = Dim3(0, 0, 0);
      cases.push_back(c);
      // exactly r wide on every axis
      c.grid = c.size = Dim3(r, r, r);
      cases.push_back(c);
      // all 26 directions, shared halo lines, unpadded
      c.grid = c.size = Dim3(9, 5, 4);
      c.radius = Radius::constant(r);
      cases.push_back(c);
      c.shared = true;
      cases.push_back(c);
      c.shared = false;
      c.pad = false;
      cases.push_back(c);
      c.pad = true;
      // Open faces among the kinds
      c.allowOpen = true;
      cases.push_back(c);
      cases.push_back(c);
      c.allowOpen = false;
      // sub-domains of a larger grid: low corner, middle (no physical face along x), high corner
      c.grid = Dim3(30, 12, 8);
      c.size = Dim3(10, 6, 4);
      c.origin = Dim3(0, 0, 0);
      cases.push_back(c);
      c.origin = Dim3(10, 6, 0);
      cases.push_back(c);
      c.origin = Dim3(20, 6, 4);
      cases.push_back(c);
    }
    // the asymmetric radius: -x 1, +x 3, -y 2, +y 0
    Case c;
    c.fp64 = fp64 != 0;
    c.radius = Radius::face_edge_corner(2, 0, 0);
    c.radius.dir(-1, 0, 0) = 1;
    c.radius.dir(1, 0, 0) = 3;
    c.radius.dir(0, 1, 0) = 0;
    c.grid = c.size = Dim3(13, 4, 3);
    c.origin = Dim3(0, 0, 0);
    cases.push_back(c);
    c.shared = true;
    cases.push_back(c);
  }
  for (size_t i = 0; i < cases.size(); ++i) run_case(cases[i], int(i));
  // a sub-domain thinner than the radius of a mirrored face is refused
  {
    LocalDomain dom(Dim3(2, 4, 4), Dim3(0, 0, 0), -1, Backend::Host);
    dom.set_radius(Radius::face_edge_corner(3, 0, 0));
    const int64_t q = dom.add_data<float>("u").id();
    dom.realize();
    BoundaryConditions bc;
    bc.set_axis(0, FaceCondition::mirror(), FaceCondition::constant(1));
    CHECK(!boundary_fill_supported(dom, Dim3(2, 4, 4), q, bc), "thin mirrored sub-domain accepted");
    bc.set_axis(0, FaceCondition::constant(0), FaceCondition::constant(1));
    CHECK(boundary_fill_supported(dom, Dim3(2, 4, 4), q, bc), "thin constant sub-domain refused");
  }
  if (g_failed) {
    std::printf("boundary_fill_check: %d checks FAILED\n", g_failed);
    return 1;
  }
  std::printf("boundary_fill_check: %zu cases ok\n", cases.size());
  return 0;
}
