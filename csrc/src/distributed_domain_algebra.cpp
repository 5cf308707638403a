// DistributedDomain::axpby: field linear combinations over every local sub-domain (stencil/kernels/field_axpby.hpp),
// with the stats of the stored values merged over the sub-domains and the ranks.
#include "distributed_domain_impl.hpp"

namespace stencil {

FieldStats DistributedDomain::axpby(FieldRef dst, double a, FieldRef x, double b, FieldRef y, bool stats, bool local,
                                    hipStream_t stream) {
  STENCIL_REQUIRE(realized_, "axpby before realize");
  STENCIL_REQUIRE(!stats || poisoned_.empty(), "field reduction refused after an earlier exchange failure: " << poisoned_);
  // every refusal before anything is enqueued
  for (const LocalDomain &d : domains_) (void)field_axpby_launch_info(d, dst, a, x, b, y, d.get_compute_region(), stats);
  for (size_t di = 0; di < domains_.size(); ++di)
    field_axpby_enqueue(domains_[di], dst, a, x, b, y, domains_[di].get_compute_region(), stream,
                        stats ? &reduce_scratch(di) : nullptr);
  FieldStats mine;
  if (!stats) return mine;
  if (backend_ == Backend::Device)
    for (const LocalDomain &d : domains_) {
      d.set_device();
      HIP_CHECK(hipStreamSynchronize(stream));
    }
  for (size_t di = 0; di < domains_.size(); ++di) mine.merge(reduce_scratch(di).result());
  if (local || pg_->size() == 1) return mine;
  std::vector<FieldStats> all(size_t(pg_->size()));
  pg_->allgather(&mine, sizeof(FieldStats), all.data());
  FieldStats r;
  for (const FieldStats &s : all) r.merge(s);
  return r;
}

} // namespace stencil
