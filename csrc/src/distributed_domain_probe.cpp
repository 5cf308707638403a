// DistributedDomain pre-flight probes, both called from realize(): the transport self-test (a coordinate-encoded
// probe domain run on a forked process group) and the HIP-IPC mapping probe between co-located ranks.
#include "stencil/domain/distributed_domain.hpp"

#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "stencil/rt/hip_check.hpp"
#include "stencil/rt/trace.hpp"

namespace stencil {

// ------------------------------------------------------------------------------------------------
// transport self-test (opt-in): coordinate oracle on a probe domain, ladder Colocated -> Rccl -> Staged
// ------------------------------------------------------------------------------------------------
namespace {
constexpr int32_t kProbePoison = -1;
int32_t probe_key(int64_t gx, int64_t gy, int64_t gz, const Dim3 &L, int32_t offset) {
  return int32_t((gx + L.x * (gy + L.y * gz)) % 1000000007) + offset;
}
} // namespace

int64_t DistributedDomain::probe_transports(MethodFlags m) {
  // same group, radius, boundary, placement, cut costs, devices, backend and transport options; every axis
  // shrunk ~16x (at least 6 cells per stencil reach) so the probe is cheap but spans the same rank pairs
  int64_t rmax = 1;
  for (int i = 0; i < 27; ++i) rmax = std::max<int64_t>(rmax, radius_.dir(dir_from_index(i)));
  auto shrink = [&](int64_t n) { return std::min<int64_t>(n, std::max<int64_t>((n + 15) / 16, 6 * rmax + 2)); };
  // the probe runs on a fork of the group: a rank whose probe fails (an exception anywhere in realize / exchange)
  // abandons the fork mid-sequence and goes straight to the verdict below; the other ranks' next receive on the
  // fork then times out after waitTimeout, they fail too and join the verdict, and this group's own collective
  // sequence never goes out of step
  const double forkTimeout = std::max(1.0, topt_.waitTimeout);
  std::shared_ptr<comm::ProcGroup> grp = pg_->size() > 1 ? pg_->fork(forkTimeout) : pg_;
  int64_t bad = 0;
  {
    DistributedDomain p(shrink(size_.x), shrink(size_.y), shrink(size_.z), grp);
    p.set_radius(radius_);
    p.set_boundary(boundary_);
    p.set_methods(m);
    p.set_placement(strategy_);
    p.set_axis_cost(axisCost_);
    p.set_partition_objective(objective_);
    if (!gpus_.empty()) p.set_gpus(gpus_);
    if (backendSet_) p.set_backend(backend_);
    p.set_transport_options(topt_);
    p.set_plan_file("");
    p.set_x_halo_align(xHaloAlign_);
    p.set_shared_halo_line(sharedHaloLine_);
    p.set_interior_align(interiorAlign_);
    p.add_data(4, "probe", DType::I32);
    try {
      p.realize();
      if (topt_.failProbeRank == rank() && probeFailures_++ == 0) // test hook: this rank's first probe fails alone
        LOG_FATAL("TransportOptions::failProbeRank: probe failure forced on rank " << rank());
      const Dim3 L = p.size();
      for (int it = 0; it < 2; ++it) {
        const int32_t off = 7 * it;
        for (auto &d : p.domains_) {
          const Dim3 raw = d.raw_size(), org = d.accessor_origin();
          std::vector<int32_t> v(size_t(raw.flatten()), kProbePoison);
          const Rect3 cr = d.get_compute_region();
          for (int64_t z = 0; z < raw.z; ++z)
            for (int64_t y = 0; y < raw.y; ++y)
              for (int64_t x = 0; x < raw.x; ++x)
                if (cr.contains(Dim3(org.x + x, org.y + y, org.z + z)))
                  v[size_t(x + raw.x * (y + raw.y * z))] = probe_key(org.x + x, org.y + y, org.z + z, L, off);
          d.region_from_host(Dim3(0, 0, 0), raw, 0, v.data(), true);
          d.region_from_host(Dim3(0, 0, 0), raw, 0, v.data(), false);
        }
        p.exchange();
        for (auto &d : p.domains_) {
          const Dim3 raw = d.raw_size(), org = d.accessor_origin();
          const Rect3 cr = d.get_compute_region();
          const auto bytes = d.region_to_host(Dim3(0, 0, 0), raw, 0, true);
          const int32_t *got = reinterpret_cast<const int32_t *>(bytes.data());
          for (int64_t z = 0; z < raw.z; ++z)
            for (int64_t y = 0; y < raw.y; ++y)
              for (int64_t x = 0; x < raw.x; ++x) {
                const int64_t g[3] = {org.x + x, org.y + y, org.z + z};
                const int64_t lo[3] = {cr.lo.x, cr.lo.y, cr.lo.z}, hi[3] = {cr.hi.x, cr.hi.y, cr.hi.z};
                const int64_t n[3] = {L.x, L.y, L.z};
                int dd[3];
                bool crossesClosed = false;
                for (int a = 0; a < 3; ++a) {
                  dd[a] = g[a] >= hi[a] ? 1 : (g[a] < lo[a] ? -1 : 0);
                  if ((g[a] < 0 || g[a] >= n[a]) &&
                      !boundary_.face_periodic(a == 0 ? dd[a] : 0, a == 1 ? dd[a] : 0, a == 2 ? dd[a] : 0))
                    crossesClosed = true;
                }
                const bool filled = (dd[0] == 0 && dd[1] == 0 && dd[2] == 0) ||
                                    (radius_.dir(Dim3(dd[0], dd[1], dd[2])) != 0 && !crossesClosed);
                const int32_t want =
                    filled ? probe_key(((g[0] % n[0]) + n[0]) % n[0], ((g[1] % n[1]) + n[1]) % n[1],
                                       ((g[2] % n[2]) + n[2]) % n[2], L, off)
                           : kProbePoison;
                bad += got[size_t(x + raw.x * (y + raw.y * z))] != want;
              }
        }
        p.swap();
      }
    } catch (const std::exception &e) {
      LOG_WARN("rank " << rank() << ": transport probe with " << to_string(m) << " failed: " << e.what());
      bad += int64_t(1) << 40;
      p.poison("transport probe failed"); // its destructor must not wait on work stuck behind an absent peer
    }
  } // the probe domain (and its bounded destructor barrier on the fork) is gone before the verdict
  return int64_t(pg_->allreduce_sum_u64(uint64_t(bad)));
}

// HIP-IPC pre-flight: every rank maps a small uncached block of every co-located rank and reads it back.
// If any mapping fails anywhere, Colocated is disabled on all ranks (they then agree on RCCL/staged).
// Reads gpus_, flags_ and the probe options; may drop Colocated from flags_.
void DistributedDomain::probe_ipc() {
  comm::ProcGroup &pg = *pg_;
  const int myRank = pg.rank();
  if (backend_ != Backend::Device || !any_methods(MethodFlags::Colocated) || pg.size() == 1 ||
      pg.colocated_size() <= 1 || !topt_.ipcProbe)
    return;
  TraceRange trp("ipc probe");
  // up to 3 collective attempts with a growing pause between them (50, 200 ms): a transient open/map failure on a
  // busy node must not cost the transport. Every failed attempt logs the call that failed on this rank.
  bool allOk = false;
  for (int attempt = 0; attempt < 3 && !allOk; ++attempt) {
    if (attempt > 0) std::this_thread::sleep_for(std::chrono::milliseconds(50 * (1 << (2 * (attempt - 1)))));
    int ok = 1;
    const char *failed = "";
    int failedPeer = -1;
    char *blk = nullptr;
    HIP_CHECK(hipSetDevice(gpus_[0]));
    if (hipExtMallocWithFlags((void **)&blk, 256, hipDeviceMallocUncached) != hipSuccess) {
      (void)hipGetLastError();
      ok = 0;
      failed = "hipExtMallocWithFlags(uncached)";
    }
    hipIpcMemHandle_t mine{};
    if (ok && hipIpcGetMemHandle(&mine, blk) != hipSuccess) {
      (void)hipGetLastError();
      ok = 0;
      failed = "hipIpcGetMemHandle";
    }
    if (ok) {
      const uint64_t tag = 0x57e9c11000000000ull + uint64_t(myRank);
      HIP_CHECK(hipMemcpy(blk, &tag, sizeof(tag), hipMemcpyHostToDevice));
    }
    std::vector<hipIpcMemHandle_t> all(pg.size());
    pg.allgather(&mine, sizeof(mine), all.data());
    std::vector<int> oks(pg.size());
    pg.allgather(&ok, sizeof(int), oks.data());
    for (int r = 0; r < pg.size() && ok; ++r) {
      if (r == myRank || !pg.colocated(r) || !oks[r]) continue;
      char *peer = nullptr;
      if (hipIpcOpenMemHandle((void **)&peer, all[r], hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
        (void)hipGetLastError();
        ok = 0;
        failed = "hipIpcOpenMemHandle";
        failedPeer = r;
        break;
      }
      uint64_t got = 0;
      if (hipMemcpy(&got, peer, sizeof(got), hipMemcpyDeviceToHost) != hipSuccess ||
          got != 0x57e9c11000000000ull + uint64_t(r)) {
        (void)hipGetLastError();
        ok = 0;
        failed = "readback of the mapped block";
        failedPeer = r;
      }
      (void)hipIpcCloseMemHandle(peer);
    }
    if (topt_.failIpcProbe) { // rehearses the fallback (tests)
      ok = 0;
      failed = "STENCIL_IPC_PROBE_FAIL";
    }
    if (!ok)
      LOG_INFO("IPC pre-flight attempt " << attempt + 1 << "/3 failed on rank " << myRank << ": " << failed
                                         << (failedPeer >= 0 ? " (peer rank " + std::to_string(failedPeer) + ")" : ""));
    allOk = pg.allreduce_min_i64(ok) == 1;
    pg.barrier(); // peers are done with our block
    if (blk) (void)hipFree(blk);
  }
  if (!allOk) {
    if (myRank == 0) LOG_WARN("HIP IPC between co-located ranks is unavailable; Colocated transport disabled");
    flags_ = without(flags_, MethodFlags::Colocated);
  }
}

} // namespace stencil
