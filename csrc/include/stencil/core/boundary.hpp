#pragma once
// Boundary: per-direction global boundary condition of the distributed grid.
// Parity: reference include/stencil/boundary.hpp:7-25 (a per-direction "periodic" flag, default periodic). The
// reference never consults it and only supports periodic grids (src/stencil.cu:155-157). Here it is honoured by
// DistributedDomain::set_boundary: across a non-periodic face of the global grid no halo message is planned. What
// the ghost cells beyond such a face hold is chosen per face and per quantity with BoundaryConditions (below):
// left as the application wrote them (Open, the default of set_boundary alone), a constant, the mirror image of the
// interior (zero normal gradient) or its anti-mirror image (a value at the face). DistributedDomain::apply_boundary
// fills them after the exchange (stencil/kernels/boundary_fill.hpp).
#include <stdexcept>
#include <string>

#include "stencil/core/geometry.hpp"

class Boundary {
  DirectionMap<bool> periodic_;

public:
  // default: periodic in every direction
  Boundary() {
    for (int z = -1; z <= 1; ++z)
      for (int y = -1; y <= 1; ++y)
        for (int x = -1; x <= 1; ++x) periodic_.at_dir(x, y, z) = true;
  }
  static Boundary periodic() { return Boundary(); }
  // per-axis flags (both faces of an axis share the flag)
  static Boundary axes(bool px, bool py, bool pz) {
    Boundary b;
    b.set_axis(0, px);
    b.set_axis(1, py);
    b.set_axis(2, pz);
    return b;
  }
  static Boundary none() { return axes(false, false, false); }

  void set_face(int x, int y, int z, bool p) { periodic_.at_dir(x, y, z) = p; }
  void set_axis(int axis, bool p) {
    const int d[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    periodic_.at_dir(d[axis][0], d[axis][1], d[axis][2]) = p;
    periodic_.at_dir(-d[axis][0], -d[axis][1], -d[axis][2]) = p;
  }
  // face flag (one of x/y/z non-zero)
  bool face_periodic(int x, int y, int z) const { return periodic_.at_dir(x, y, z); }
  // a direction (face, edge or corner) wraps iff every face it crosses is periodic
  bool wraps(const Dim3 &dir) const {
    if (dir.x != 0 && !periodic_.at_dir(int(dir.x), 0, 0)) return false;
    if (dir.y != 0 && !periodic_.at_dir(0, int(dir.y), 0)) return false;
    if (dir.z != 0 && !periodic_.at_dir(0, 0, int(dir.z))) return false;
    return true;
  }
  bool all_periodic() const {
    for (int a = -1; a <= 1; a += 2)
      if (!face_periodic(a, 0, 0) || !face_periodic(0, a, 0) || !face_periodic(0, 0, a)) return false;
    return true;
  }
  // does stepping from sub-domain `idx` along `dir` stay inside a grid of `dim` sub-domains, or wrap periodically?
  bool reachable(const Dim3 &idx, const Dim3 &dir, const Dim3 &dim) const {
    const int64_t p[3] = {idx.x + dir.x, idx.y + dir.y, idx.z + dir.z};
    const int64_t n[3] = {dim.x, dim.y, dim.z};
    const int64_t dd[3] = {dir.x, dir.y, dir.z};
    for (int a = 0; a < 3; ++a) {
      if (p[a] >= 0 && p[a] < n[a]) continue;
      const int s = int(dd[a]);
      const bool per = a == 0 ? face_periodic(s, 0, 0) : (a == 1 ? face_periodic(0, s, 0) : face_periodic(0, 0, s));
      if (!per) return false;
    }
    return true;
  }
  bool operator==(const Boundary &o) const { return periodic_ == o.periodic_; }
};

// ---- physical boundary conditions: how the ghost cells beyond a non-periodic face of the global grid are filled ----
// A ghost cell at distance k = 1..r outside a face has its mirror cell at the same distance inside.
//   Periodic       the face wraps (halo exchange); both faces of an axis or neither
//   Open           not written
//   Constant(v)    ghost = T(v)
//   Mirror         ghost = mirror cell (zero normal gradient at the face of a cell-centred grid)
//   AntiMirror(v)  ghost = T(2.0 * v) - mirror cell (the field takes the value v at the face, to second order)
enum class FaceKind : int { Periodic = 0, Open = 1, Constant = 2, Mirror = 3, AntiMirror = 4 };

struct FaceCondition {
  FaceKind kind = FaceKind::Periodic;
  double value = 0;
  static FaceCondition periodic() { return FaceCondition{FaceKind::Periodic, 0}; }
  static FaceCondition open() { return FaceCondition{FaceKind::Open, 0}; }
  static FaceCondition constant(double v) { return FaceCondition{FaceKind::Constant, v}; }
  static FaceCondition mirror() { return FaceCondition{FaceKind::Mirror, 0}; }
  static FaceCondition antimirror(double v) { return FaceCondition{FaceKind::AntiMirror, v}; }
  bool operator==(const FaceCondition &o) const { return kind == o.kind && value == o.value; }
};

class BoundaryConditions {
  FaceCondition f_[3][2]; // [axis][0 = low face, 1 = high face]

  static void face_index(int x, int y, int z, int *axis, int *side) {
    if ((x != 0) + (y != 0) + (z != 0) != 1 || x < -1 || x > 1 || y < -1 || y > 1 || z < -1 || z > 1)
      throw std::invalid_argument("BoundaryConditions: a face is one of (+-1, 0, 0), (0, +-1, 0), (0, 0, +-1)");
    *axis = x ? 0 : (y ? 1 : 2);
    *side = (x + y + z) > 0 ? 1 : 0;
  }

public:
  // default: periodic everywhere
  BoundaryConditions() {}
  static BoundaryConditions all_periodic_conditions() { return BoundaryConditions(); }
  // every face of the non-periodic axes of `b` Open: what set_boundary(b) alone means
  static BoundaryConditions open_where_nonperiodic(const Boundary &b) {
    BoundaryConditions c;
    if (!b.face_periodic(1, 0, 0)) c.f_[0][0] = c.f_[0][1] = FaceCondition::open();
    if (!b.face_periodic(0, 1, 0)) c.f_[1][0] = c.f_[1][1] = FaceCondition::open();
    if (!b.face_periodic(0, 0, 1)) c.f_[2][0] = c.f_[2][1] = FaceCondition::open();
    return c;
  }
  void set_face(int x, int y, int z, const FaceCondition &c) {
    int a, s;
    face_index(x, y, z, &a, &s);
    f_[a][s] = c;
  }
  void set_axis(int axis, const FaceCondition &lo, const FaceCondition &hi) {
    if (axis < 0 || axis > 2) throw std::invalid_argument("BoundaryConditions: axis 0..2");
    if ((lo.kind == FaceKind::Periodic) != (hi.kind == FaceKind::Periodic))
      throw std::invalid_argument("BoundaryConditions: both faces of an axis are periodic, or neither");
    f_[axis][0] = lo;
    f_[axis][1] = hi;
  }
  const FaceCondition &face(int x, int y, int z) const {
    int a, s;
    face_index(x, y, z, &a, &s);
    return f_[a][s];
  }
  const FaceCondition &at(int axis, int side) const { return f_[axis][side]; }
  // refuses an axis with one periodic face (set_face sets one face at a time)
  void validate() const {
    for (int a = 0; a < 3; ++a)
      if ((f_[a][0].kind == FaceKind::Periodic) != (f_[a][1].kind == FaceKind::Periodic))
        throw std::invalid_argument("BoundaryConditions: both faces of an axis are periodic, or neither (axis " +
                                    std::string(a == 0 ? "x" : (a == 1 ? "y" : "z")) + ")");
  }
  // the periodic flags these conditions imply
  Boundary boundary() const {
    validate();
    return Boundary::axes(f_[0][0].kind == FaceKind::Periodic, f_[1][0].kind == FaceKind::Periodic,
                          f_[2][0].kind == FaceKind::Periodic);
  }
  bool all_periodic() const {
    for (int a = 0; a < 3; ++a)
      for (int s = 0; s < 2; ++s)
        if (f_[a][s].kind != FaceKind::Periodic) return false;
    return true;
  }
  // a face that apply_boundary writes (Constant, Mirror or AntiMirror)
  bool any_filled() const {
    for (int a = 0; a < 3; ++a)
      for (int s = 0; s < 2; ++s)
        if (f_[a][s].kind != FaceKind::Periodic && f_[a][s].kind != FaceKind::Open) return true;
    return false;
  }
  bool operator==(const BoundaryConditions &o) const {
    for (int a = 0; a < 3; ++a)
      for (int s = 0; s < 2; ++s)
        if (!(f_[a][s] == o.f_[a][s])) return false;
    return true;
  }
};
