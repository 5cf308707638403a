// DistributedDomain: physical boundary conditions and apply_boundary (stencil/kernels/boundary_fill.hpp).
#include "distributed_domain_impl.hpp"

namespace stencil {

void DistributedDomain::set_boundary_conditions(const BoundaryConditions &bc) {
  STENCIL_REQUIRE(!realized_, "set_boundary_conditions after realize");
  const Boundary b = bc.boundary(); // refuses an axis with one periodic face
  for (const auto &kv : bcQuantity_)
    STENCIL_REQUIRE(kv.second.boundary() == b, "the conditions of quantity " << kv.first
                                                   << " are periodic along other axes than the grid's");
  bc_ = bc;
  bcSet_ = true;
  boundary_ = b;
}

void DistributedDomain::set_boundary_conditions(int64_t q, const BoundaryConditions &bc) {
  STENCIL_REQUIRE(!realized_, "set_boundary_conditions after realize");
  STENCIL_REQUIRE(q >= 0 && q < int64_t(elemSize_.size()), "set_boundary_conditions: quantity " << q << " of "
                                                                                                 << elemSize_.size());
  STENCIL_REQUIRE(bc.boundary() == boundary_,
                  "the conditions of quantity " << q << " are periodic along other axes than the grid's");
  bcQuantity_[q] = bc;
}

BoundaryConditions DistributedDomain::boundary_conditions(int64_t q) const {
  auto it = bcQuantity_.find(q);
  if (it != bcQuantity_.end()) return it->second;
  return bcSet_ ? bc_ : BoundaryConditions::open_where_nonperiodic(boundary_);
}

// realize(), once the placement is known and before anything is allocated. The same on every rank: every sub-domain of
// the grid is checked, not only the local ones.
void DistributedDomain::check_boundary_conditions() const {
  const Dim3 dim = placement_->dim();
  const int64_t n[3] = {size_.x, size_.y, size_.z};
  for (int64_t q = 0; q < int64_t(elemSize_.size()); ++q) {
    const BoundaryConditions bc = boundary_conditions(q);
    STENCIL_REQUIRE(bc.boundary() == boundary_,
                    "the conditions of quantity " << q << " are periodic along other axes than the grid's");
    if (!bc.any_filled()) continue;
    const DType dt = dtypes_[size_t(q)];
    const bool fp = dt == DType::F32 || dt == DType::F64 || (dt == DType::Bytes && (elemSize_[size_t(q)] == 4 || elemSize_[size_t(q)] == 8));
    STENCIL_REQUIRE(fp, "quantity " << q << " (" << names_[size_t(q)] << ") is not fp32 / fp64 and cannot take Constant, "
                            "Mirror or AntiMirror faces: give it Open faces with set_boundary_conditions(" << q << ", ...)");
    for (int64_t iz = 0; iz < dim.z; ++iz)
      for (int64_t iy = 0; iy < dim.y; ++iy)
        for (int64_t ix = 0; ix < dim.x; ++ix) {
          const Dim3 idx(ix, iy, iz);
          const Dim3 o = placement_->subdomain_origin(idx), s = placement_->subdomain_size(idx);
          const int64_t org[3] = {o.x, o.y, o.z}, sz[3] = {s.x, s.y, s.z};
          for (int a = 0; a < 3; ++a)
            for (int side = 0; side < 2; ++side) {
              const FaceKind k = bc.at(a, side).kind;
              if (k != FaceKind::Mirror && k != FaceKind::AntiMirror) continue;
              if (side == 0 ? org[a] != 0 : org[a] + sz[a] != n[a]) continue;
              const int sgn = side == 0 ? -1 : 1;
              const int64_t r = a == 0 ? radius_.x(sgn) : (a == 1 ? radius_.y(sgn) : radius_.z(sgn));
              STENCIL_REQUIRE(sz[a] >= r, "sub-domain " << idx << " is " << sz[a] << " cells thin along axis " << a
                                                        << ", below the face radius " << r << " of its mirrored face (quantity "
                                                        << q << ")");
            }
        }
  }
}

BoundaryFillCache &DistributedDomain::fill_cache(size_t di) {
  STENCIL_REQUIRE(realized_, "apply_boundary before realize");
  STENCIL_REQUIRE(di < domains_.size(), "local domain " << di << " of " << domains_.size());
  if (fillCache_.size() < domains_.size()) fillCache_.resize(domains_.size());
  if (!fillCache_[di]) fillCache_[di] = std::make_unique<BoundaryFillCache>();
  return *fillCache_[di];
}

void DistributedDomain::apply_boundary(hipStream_t stream) {
  STENCIL_REQUIRE(realized_, "apply_boundary before realize");
  std::vector<FillRequest> reqs;
  for (int64_t q = 0; q < int64_t(elemSize_.size()); ++q) {
    FillRequest rq;
    rq.q = q;
    rq.curr = true;
    rq.bc = boundary_conditions(q);
    if (rq.bc.any_filled()) reqs.push_back(rq);
  }
  if (reqs.empty()) return;
  for (const LocalDomain &d : domains_) (void)boundary_fill_launch_info(d, size_, reqs); // every refusal first
  for (size_t di = 0; di < domains_.size(); ++di) boundary_fill_enqueue(domains_[di], size_, reqs, fill_cache(di), stream);
}

void DistributedDomain::apply_boundary(int64_t q, bool curr, hipStream_t stream) {
  STENCIL_REQUIRE(realized_, "apply_boundary before realize");
  STENCIL_REQUIRE(q >= 0 && q < int64_t(elemSize_.size()), "apply_boundary: quantity " << q << " of " << elemSize_.size());
  FillRequest rq;
  rq.q = q;
  rq.curr = curr;
  rq.bc = boundary_conditions(q);
  if (!rq.bc.any_filled()) return;
  const std::vector<FillRequest> reqs{rq};
  for (const LocalDomain &d : domains_) (void)boundary_fill_launch_info(d, size_, reqs);
  for (size_t di = 0; di < domains_.size(); ++di) boundary_fill_enqueue(domains_[di], size_, reqs, fill_cache(di), stream);
}

} // namespace stencil
