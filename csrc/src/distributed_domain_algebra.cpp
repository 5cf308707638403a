// DistributedDomain::axpby and convert_from: field linear combinations (stencil/kernels/field_axpby.hpp) and
// type-converting copies from another domain (stencil/kernels/field_convert.hpp) over every local sub-domain, with the
// stats of the stored values merged over the sub-domains and the ranks.
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
  return stats ? merged_stats(local, stream) : FieldStats();
}

FieldStats DistributedDomain::convert_from(const DistributedDomain &srcDom, FieldRef dst, FieldRef src, double scale,
                                           bool stats, bool local, hipStream_t stream) {
  STENCIL_REQUIRE(realized_ && srcDom.realized(), "convert_from before realize");
  STENCIL_REQUIRE(!stats || poisoned_.empty(), "field reduction refused after an earlier exchange failure: " << poisoned_);
  const std::vector<LocalDomain> &from = srcDom.domains();
  STENCIL_REQUIRE(from.size() == domains_.size(), "convert_from: " << from.size() << " local sub-domains in the source, "
                                                                    << domains_.size() << " in the destination");
  // every refusal before anything is enqueued
  for (size_t di = 0; di < domains_.size(); ++di)
    (void)field_convert_launch_info(from[di], src, domains_[di], dst, scale, domains_[di].get_compute_region(), stats);
  for (size_t di = 0; di < domains_.size(); ++di)
    field_convert_enqueue(from[di], src, domains_[di], dst, scale, domains_[di].get_compute_region(), stream,
                          stats ? &reduce_scratch(di) : nullptr);
  return stats ? merged_stats(local, stream) : FieldStats();
}

// the stats a launch per sub-domain left in the scratches: waits for `stream` on every device, merges the sub-domains
// in index order and, unless `local`, the ranks in rank order
FieldStats DistributedDomain::merged_stats(bool local, hipStream_t stream) {
  FieldStats mine;
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
