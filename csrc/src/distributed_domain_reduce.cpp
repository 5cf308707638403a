// DistributedDomain::reduce: field reductions over every local sub-domain and every rank.
#include "distributed_domain_impl.hpp"

namespace stencil {

ReduceScratch &DistributedDomain::reduce_scratch(size_t di) {
  STENCIL_REQUIRE(realized_, "reduce before realize");
  STENCIL_REQUIRE(di < domains_.size(), "local domain " << di << " of " << domains_.size());
  if (reduceScratch_.size() < domains_.size()) reduceScratch_.resize(domains_.size());
  if (!reduceScratch_[di]) reduceScratch_[di] = std::make_unique<ReduceScratch>();
  return *reduceScratch_[di];
}

FieldStats DistributedDomain::reduce(int64_t qa, bool currA, int64_t qb, bool currB, bool local) {
  STENCIL_REQUIRE(realized_, "reduce before realize");
  STENCIL_REQUIRE(poisoned_.empty(), "field reduction refused after an earlier exchange failure: " << poisoned_);
  Impl &I = *impl_;
  // every refusal before anything is enqueued
  for (const LocalDomain &d : domains_)
    (void)field_reduce_launch_info(d, qa, currA, qb, currB, d.get_compute_region());
  FieldStats mine;
  if (backend_ == Backend::Host) {
    for (size_t di = 0; di < domains_.size(); ++di)
      mine.merge(field_reduce(domains_[di], qa, currA, qb, currB, domains_[di].get_compute_region(), reduce_scratch(di)));
  } else {
    // the comm streams already follow the last comm-stream exchange; join a caller-stream exchange, then the producers
    if (I.callerPending) {
      HIP_CHECK(hipSetDevice(I.devs[0].dev));
      I.callerDone.wait_on(I.devs[0].comm);
    }
    bool anyMissing = false;
    for (size_t di = 0; di < domains_.size(); ++di) anyMissing |= !I.readyPending[di];
    if (anyMissing && topt_.nullStreamProducers && I.devs.size() == 1) {
      HIP_CHECK(hipSetDevice(I.devs[0].dev));
      I.nullReady.record(nullptr);
      I.nullReady.wait_on(I.devs[0].comm);
    } else if (anyMissing) {
      for (auto &d : I.devs) {
        HIP_CHECK(hipSetDevice(d.dev));
        HIP_CHECK(hipDeviceSynchronize());
      }
    }
    // the ready events stay pending: the next exchange still waits for them
    for (size_t di = 0; di < domains_.size(); ++di) {
      DevCtx &ctx = I.devs[size_t(I.devIndex.at(domains_[di].gpu()))];
      HIP_CHECK(hipSetDevice(ctx.dev));
      if (I.readyPending[di]) I.ready[di].wait_on(ctx.comm);
      field_reduce_enqueue(domains_[di], qa, currA, qb, currB, domains_[di].get_compute_region(), reduce_scratch(di),
                           ctx.comm);
    }
    sync_exchange();
    for (size_t di = 0; di < domains_.size(); ++di) mine.merge(reduce_scratch(di).result());
  }
  if (local || pg_->size() == 1) return mine;
  std::vector<FieldStats> all(size_t(pg_->size()));
  pg_->allgather(&mine, sizeof(FieldStats), all.data());
  FieldStats r;
  for (const FieldStats &s : all) r.merge(s);
  return r;
}

} // namespace stencil
