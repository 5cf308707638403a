// DistributedDomain implementation: placement, message planning, transport setup and the exchange engine.
// See distributed_domain.hpp for the design; reference call stacks: SURVEY §3.2 (realize) and §3.3 (exchange).
#include "stencil/domain/distributed_domain.hpp"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <fstream>
#include <functional>
#include <sstream>

#include "stencil/comm/rccl_comm.hpp"
#include "stencil/comm/tags.hpp"
#include "stencil/rt/env.hpp"
#include "stencil/rt/hip_check.hpp"
#include "stencil/rt/trace.hpp"
#include "stencil/topo/gpu_topology.hpp"

#include "distributed_domain_impl.hpp"

namespace stencil {


std::string to_string(MethodFlags m) {
  std::string s;
  auto add = [&](MethodFlags f, const char *n) {
    if (m && f) s += (s.empty() ? "" : "/") + std::string(n);
  };
  add(MethodFlags::Staged, "staged");
  add(MethodFlags::Rccl, "rccl");
  add(MethodFlags::Colocated, "colo");
  add(MethodFlags::PeerCopy, "peer");
  add(MethodFlags::Kernel, "kernel");
  return s.empty() ? "none" : s;
}

MethodFlags select_method(MethodFlags flags, const PairInfo &p) {
  auto on = [&](MethodFlags m) { return (int(flags) & int(m)) != 0; };
  if (!p.device) {
    if (p.sameRank && (on(MethodFlags::Kernel) || on(MethodFlags::PeerCopy)))
      return p.sameDevice && on(MethodFlags::Kernel) ? MethodFlags::Kernel : MethodFlags::PeerCopy;
    return on(MethodFlags::Staged) ? MethodFlags::Staged : MethodFlags::None;
  }
  if (on(MethodFlags::Kernel) && p.sameRank && p.sameDevice) return MethodFlags::Kernel;
  if (on(MethodFlags::PeerCopy) && p.sameRank && p.peer) return MethodFlags::PeerCopy;
  if (on(MethodFlags::Colocated) && !p.sameRank && p.sameHost && p.canAccess) return MethodFlags::Colocated;
  if (on(MethodFlags::Rccl) && !p.sharedGpu) return MethodFlags::Rccl;
  if (on(MethodFlags::Staged)) return MethodFlags::Staged;
  if (on(MethodFlags::Rccl) && p.sharedGpu) return MethodFlags::Staged;
  return MethodFlags::None;
}

// ------------------------------------------------------------------------------------------------
// construction / configuration
// ------------------------------------------------------------------------------------------------
DistributedDomain::DistributedDomain(int64_t x, int64_t y, int64_t z, std::shared_ptr<comm::ProcGroup> pg)
    : size_(x, y, z), pg_(pg ? pg : comm::default_group()), impl_(new Impl) {
  radius_ = Radius::constant(0);
#ifdef STENCIL_EXCHANGE_STATS
  exchangeStats_ = STENCIL_EXCHANGE_STATS != 0;
#endif
  topt_.waitTimeout = env_wait_timeout(60.0);
  if (env::get_int("STENCIL_PLAN_FILE", 1) == 0) planPrefix_.clear();
}

void DistributedDomain::set_transport_options(const TransportOptions &o) {
  STENCIL_REQUIRE(!realized_, "set_transport_options after realize");
  topt_ = o;
  if (topt_.waitTimeout <= 0) topt_.waitTimeout = env_wait_timeout(60.0);
}

// whole-line x faces for the translate s -> d: where asked for explicitly, else only on a device whose same-GPU x
// faces reached the auto threshold and only for its same-GPU translates (the threshold was measured there; a
// PeerCopy store across xGMI is left as w-cell pieces)
bool DistributedDomain::x_face_lines(const LocalDomain &s, const LocalDomain &d) const {
  if (topt_.xFaceSectors) return true;
  return s.gpu() == d.gpu() && impl_->xLineDevs.count(s.gpu()) > 0;
}

void DistributedDomain::poison(const std::string &why) {
  if (poisoned_.empty()) poisoned_ = why;
}

DistributedDomain::~DistributedDomain() {
  if (!impl_) return;
  Impl &I = *impl_;
  // a poisoned domain may have work stuck behind a dead peer: do not block on it (the process is going down)
  if (poisoned_.empty()) {
    try {
      for (auto &d : I.devs) {
        (void)HIP_TRY(hipSetDevice(d.dev));
        (void)HIP_TRY(hipStreamSynchronize(d.comm));
      }
      // the Acks no later record consumes: the next IpcEvent domain on this group reuses the channel tags
      if (!drain_ipc_acks(topt_.waitTimeout)) LOG_WARN("IPC-event acks not drained within the wait timeout");
    } catch (...) {
    }
  }
  for (auto &pp : I.pipes) {
    if (pp.sbuf) (void)hipFree(pp.sbuf);
    if (pp.rbuf) (void)hipFree(pp.rbuf);
  }
  for (auto &c : I.chans) {
    if (c.dbuf) (void)hipFree(c.dbuf);
    if (c.hbuf) (void)hipHostFree(c.hbuf);
    if (c.ipcEvent) (void)hipEventDestroy(c.ipcEvent);
    for (auto &r : c.ipcRetired) {
      if (r.fence) (void)hipEventDestroy(r.fence);
      (void)hipEventDestroy(r.event);
    }
    if (c.remoteFlag) (void)hipIpcCloseMemHandle(c.remoteFlag);
    if (c.remoteData) (void)hipIpcCloseMemHandle(c.remoteData);
  }
  // make sure peers closed their mappings of our blocks before freeing them; bounded, so a dead or stalled peer
  // cannot hold this rank in its destructor (the blocks then simply stay allocated until the process exits)
  bool peersDone = true;
  try {
    if (realized_ && pg_->size() > 1) peersDone = pg_->barrier_for(topt_.waitTimeout);
  } catch (...) {
    peersDone = false;
  }
  for (auto &c : I.chans) {
    if (!peersDone) break;
    if (c.ownFlag) (void)hipFree(c.ownFlag);
    if (c.ownData) (void)hipFree(c.ownData);
  }
  for (auto &d : I.devs) {
    d.release();
    if (d.nccl) {
      if (poisoned_.empty())
        rccl::destroy(d.nccl);
      else
        rccl::abort(d.nccl);
    }
  }
  if (I.errHost) (void)hipHostFree(I.errHost);
  if (I.doneHost) (void)hipHostFree(I.doneHost);
}

int64_t DistributedDomain::add_data(int64_t elemSize, const std::string &name, DType dtype) {
  STENCIL_REQUIRE(!realized_, "add_data after realize");
  elemSize_.push_back(elemSize);
  names_.push_back(name);
  dtypes_.push_back(dtype);
  return int64_t(elemSize_.size()) - 1;
}


// ------------------------------------------------------------------------------------------------
// RCCL communicator (or the host-staged fallback)
// ------------------------------------------------------------------------------------------------
// RCCL communicator over all (rank, device) pairs, created only if some rank needs it. An init error on any
// rank (or TransportOptions::failRcclInit) is agreed on collectively and every RCCL channel falls back to the
// host-staged transport (the reference's ladder also ends at the MPI path, src/stencil.cu:185-194).
// Reads I.chans, I.devs and I.sharedDev; leaves the communicators, ncclPeer and I.rccl, or the fallback in I.chans,
// plan_ and flags_.
void DistributedDomain::init_rccl() {
  Impl &I = *impl_;
  comm::ProcGroup &pg = *pg_;
  const int myRank = pg.rank();
  int64_t rcclChans = 0;
  for (auto &c : I.chans) rcclChans += c.method == MethodFlags::Rccl;
  if (pg.allreduce_sum_u64(uint64_t(rcclChans)) == 0) return;
  TraceRange trr("rccl init");
  // members: every (rank, device) whose GPU no other rank drives (pairs touching a shared GPU are staged)
  const int nLocal = int(I.devs.size());
  std::vector<int> counts, mine(size_t(nLocal), -1);
  for (int k = 0; k < nLocal; ++k)
    if (!I.shared_dev(myRank, I.devs[size_t(k)].dev)) mine[size_t(k)] = I.devs[size_t(k)].dev;
  const std::vector<int> allDevs = allgather_padded(pg, mine, -1, &counts);
  const int maxN = int(allDevs.size()) / pg.size();
  // RCCL rank of (rank r, slot k) = number of members before it
  std::vector<int> ncclRankOf(allDevs.size(), -1);
  int total = 0, root = -1;
  for (int r = 0; r < pg.size(); ++r)
    for (int k = 0; k < maxN; ++k)
      if (allDevs[size_t(r) * size_t(maxN) + size_t(k)] >= 0) {
        ncclRankOf[size_t(r) * size_t(maxN) + size_t(k)] = total++;
        if (root < 0) root = r;
      }
  STENCIL_REQUIRE(root >= 0, "RCCL channels planned but no rank owns an exclusive GPU");

  // every failure is collected and agreed on before anyone falls back, so no rank is left blocked in a
  // communicator the others abandoned. The unique id travels with the root's status.
  std::string why;
  struct {
    int ok;
    rccl::UniqueId id;
  } boot{1, {}};
  if (myRank == root) {
    why = rccl::get_unique_id(&boot.id);
    boot.ok = why.empty();
  }
  pg.bcast(&boot, sizeof(boot), root);
  int ok = boot.ok && !topt_.failRcclInit;
  if (!boot.ok && why.empty()) why = "the root rank could not create an RCCL id";
  if (topt_.failRcclInit) why = "TransportOptions::failRcclInit";
  // local preconditions (the id, the forced-failure hook, every member device selectable) are agreed on BEFORE any
  // rank enters ncclCommInitRank: a rank that would skip or abort creation must not leave the others blocked inside
  // RCCL waiting for it. What remains is a failure inside RCCL itself, reported by the watch thread.
  for (int k = 0; k < nLocal && ok; ++k) {
    if (ncclRankOf[size_t(myRank) * size_t(maxN) + size_t(k)] < 0) continue;
    if (hipSetDevice(I.devs[size_t(k)].dev) != hipSuccess) {
      (void)hipGetLastError();
      ok = 0;
      why = "hipSetDevice(" + std::to_string(I.devs[size_t(k)].dev) + ") before RCCL init";
    }
  }
  if (pg.allreduce_min_i64(ok) != 1) {
    if (ok) why = "another rank cannot create its RCCL communicator";
    ok = 0;
  }
  if (ok) {
    // non-blocking creation polled against the wait timeout: a member that never joins (a rank died or stalled
    // between the bcast and here) costs every other member the timeout and an abort of its communicators, after which
    // the failure is agreed on below like any other -- never a hang inside RCCL
    std::vector<int> ranks, devices, slots;
    for (int k = 0; k < nLocal; ++k) {
      const int nr = ncclRankOf[size_t(myRank) * size_t(maxN) + size_t(k)];
      if (nr < 0) continue;
      ranks.push_back(nr);
      devices.push_back(I.devs[size_t(k)].dev);
      slots.push_back(k);
    }
    std::vector<rccl::Comm> comms;
    const double t0 = now_s();
    why = rccl::init_ranks(&comms, total, boot.id, ranks, devices, topt_.waitTimeout,
                           topt_.stallRcclInitRank == myRank);
    for (size_t j = 0; j < slots.size(); ++j) I.devs[size_t(slots[j])].nccl = comms[j];
    ok = why.empty();
    if (!ok)
      LOG_ERROR("RCCL communicator creation failed after " << now_s() - t0 << " s (" << why << "); plan:\n"
                                                           << plan_summary());
  }
  if (!ok) LOG_WARN("rank " << myRank << ": RCCL unavailable (" << why << ")");
  const bool allOk = pg.allreduce_min_i64(ok) == 1;
  rcclStatus_ = allOk ? "ok" : (ok ? "failed on another rank" : why);
  if (allOk) {
    // translate remote (rank, device) into RCCL ranks
    for (auto &c : I.chans) {
      if (c.method != MethodFlags::Rccl) continue;
      int peer = -1;
      for (int k = 0; k < maxN; ++k)
        if (allDevs[size_t(c.remoteRank) * size_t(maxN) + size_t(k)] == c.remoteDev)
          peer = ncclRankOf[size_t(c.remoteRank) * size_t(maxN) + size_t(k)];
      STENCIL_REQUIRE(peer >= 0, "RCCL peer device not found");
      STENCIL_REQUIRE(I.devs[size_t(I.devIndex[c.localDev])].nccl != nullptr, "RCCL channel on a shared GPU");
      c.ncclPeer = peer;
    }
    I.rccl = true;
    return;
  }
  // fallback: every RCCL channel (and plan entry) becomes host-staged on every rank
  for (auto &d : I.devs)
    if (d.nccl) {
      rccl::abort(d.nccl);
      d.nccl = nullptr;
    }
  if (myRank == 0) LOG_WARN("RCCL communicator creation failed on some rank; RCCL halos are host-staged instead");
  for (auto &c : I.chans)
    if (c.method == MethodFlags::Rccl) c.method = MethodFlags::Staged;
  for (auto &e : plan_)
    if (e.method == MethodFlags::Rccl) e.method = MethodFlags::Staged;
  flags_ = without(flags_, MethodFlags::Rccl) | MethodFlags::Staged;
}

// ------------------------------------------------------------------------------------------------
// realize
// ------------------------------------------------------------------------------------------------
// setup timers (reference STENCIL_SETUP_STATS, stencil.cu:31-538): max over ranks, or local and collective-free
// when the option is compiled out
static double setup_time(comm::ProcGroup &pg, double local) {
  return STENCIL_SETUP_STATS ? pg.allreduce_max(local) : local;
}

// The stages below run in this order on every rank, in lock-step: each holds its process-group calls and its device
// allocations in a fixed order, so neither may move between stages or inside one.
void DistributedDomain::realize() {
  STENCIL_REQUIRE(!realized_, "realize() called twice");
  STENCIL_REQUIRE(!elemSize_.empty(), "add_data() before realize()");
  TraceRange tr0("DistributedDomain::realize");
  resolve_backend_and_self_test();
  select_gpus();
  place();
  create_local_domains();
  probe_ipc();
  gather_shared_devices();
  plan_messages();
  const double t0 = now_s();
  TraceRange trc("DistributedDomain::realize: create");
  if (backend_ == Backend::Device)
    create_device_transports();
  else
    create_host_transports();
  finish_plan(t0);
}

// Reads backendSet_, selfTest_ and flags_; leaves backend_, flags_ narrowed to the set that passed the self-test, and
// selfTestReport_.
void DistributedDomain::resolve_backend_and_self_test() {
  comm::ProcGroup &pg = *pg_;
  if (!backendSet_) backend_ = gpu_topo::device_count() > 0 ? Backend::Device : Backend::Host;
  if (selfTest_ && pg.size() > 1) {
    // ladder: as configured -> without Colocated -> without Rccl (host-staged); the last rung always runs
    TraceRange trs("transport self-test");
    std::vector<MethodFlags> ladder{flags_};
    if (flags_ && MethodFlags::Colocated) ladder.push_back(without(ladder.back(), MethodFlags::Colocated));
    if (ladder.back() && MethodFlags::Rccl)
      ladder.push_back(without(ladder.back(), MethodFlags::Rccl) | MethodFlags::Staged);
    std::ostringstream rep;
    bool found = false;
    for (size_t k = 0; k < ladder.size() && !found; ++k) {
      const int64_t bad = probe_transports(ladder[k]);
      rep << (k ? "; " : "") << to_string(ladder[k]) << ": " << (bad == 0 ? "ok" : std::to_string(bad) + " bad");
      if (bad == 0) {
        found = true;
        flags_ = ladder[k];
      }
    }
    selfTestReport_ = rep.str();
    if (pg.rank() == 0) LOG_INFO("transport self-test: " << selfTestReport_);
    STENCIL_REQUIRE(found, "no transport set passed the self-test: " << selfTestReport_);
  }
  if (backend_ == Backend::Device)
    STENCIL_REQUIRE(gpu_topo::device_count() > 0, "Device backend requested but no GPU is visible");
}

// node topology / GPU selection (reference stencil.hpp:158-245). Reads backend_ and gpus_ as configured; leaves
// gpus_, peer access among them, numaNode_ and the three topology timers.
void DistributedDomain::select_gpus() {
  comm::ProcGroup &pg = *pg_;
  const bool dev = backend_ == Backend::Device;
  double t0 = now_s();
  const int coloSize = pg.colocated_size();
  const int coloRank = pg.colocated_rank();
  timeMpiTopo_ = setup_time(pg, now_s() - t0);
  t0 = now_s();
  if (gpus_.empty()) {
    if (dev) {
      const int n = gpu_topo::device_count();
      if (coloSize >= n) {
        gpus_ = {coloRank % n};
      } else {
        const int per = n / coloSize;
        for (int i = 0; i < per; ++i) gpus_.push_back(coloRank * per + i);
      }
    } else {
      gpus_ = {0};
    }
  }
  timeNodeGpus_ = setup_time(pg, now_s() - t0);
  t0 = now_s();
  if (dev) {
    for (int a : gpus_)
      for (int b : gpus_)
        if (a != b) gpu_topo::enable_peer(a, b);
  }
  timePeerEn_ = setup_time(pg, now_s() - t0);
  if (dev && topt_.numaAffinity) {
    int node = -2;
    for (int g : gpus_) {
      const int n = gpu_topo::numa_node(g);
      node = node == -2 ? n : (node == n ? node : -1);
    }
    if (node >= 0 && gpu_topo::bind_thread_to_numa(node)) {
      numaNode_ = node;
      LOG_DEBUG("rank " << pg.rank() << " bound to NUMA node " << node << " of its GPU(s)");
    }
  }
}

// Reads gpus_, the radius and the placement options; leaves placement_ and timePlacement_, then refuses boundary
// conditions the placement cannot serve.
void DistributedDomain::place() {
  const double t0 = now_s();
  {
    TraceRange tr("placement");
    if (strategy_ == PlacementStrategy::NodeAware) {
      BandwidthFn bw = backend_ == Backend::Device ? BandwidthFn([](int a, int b) { return gpu_topo::bandwidth(a, b); })
                                                   : BandwidthFn([](int a, int b) { return a == b ? 10.0 : 1.0; });
      placement_.reset(new NodeAwarePlacement(size_, *pg_, radius_, gpus_, bw, axisCost_, objective_));
    } else {
      placement_.reset(new TrivialPlacement(size_, *pg_, gpus_));
    }
  }
  timePlacement_ = setup_time(*pg_, now_s() - t0);
  check_boundary_conditions();
}

// Reads placement_ and the layout options; leaves domains_ realized (one per entry of gpus_) and timeRealize_.
void DistributedDomain::create_local_domains() {
  const double t0 = now_s();
  const bool dev = backend_ == Backend::Device;
  domains_.reserve(gpus_.size());
  for (size_t di = 0; di < gpus_.size(); ++di) {
    const Dim3 idx = placement_->get_idx(rank(), int(di));
    const int device = placement_->get_device(idx);
    domains_.emplace_back(placement_->subdomain_size(idx), placement_->subdomain_origin(idx), dev ? device : -1, backend_);
    LocalDomain &d = domains_.back();
    d.set_radius(radius_);
    d.set_padding(pad_);
    d.set_x_halo_align(xHaloAlign_);
    d.set_shared_halo_line(sharedHaloLine_);
    d.set_interior_align(interiorAlign_);
    d.set_row_pad_lines(rowPadLines_);
    for (size_t q = 0; q < elemSize_.size(); ++q) d.add_data(elemSize_[q], names_[q], dtypes_[q]);
    LOG_INFO("rank " << rank() << " domain " << di << " idx " << idx << " size " << d.size() << " origin " << d.origin()
                     << " device " << device);
  }
  for (auto &d : domains_) d.realize();
  timeRealize_ = setup_time(*pg_, now_s() - t0);
}

// physical device identity of every (rank, device ordinal): ranks may number devices differently, and RCCL
// refuses a communicator in which two ranks drive one GPU. Pairs with an endpoint on a GPU that another rank of
// the same host also drives never use RCCL (select_method); everything else keeps its transport.
// Reads gpus_; leaves Impl::sharedDev (empty on the host backend and on one rank).
void DistributedDomain::gather_shared_devices() {
  comm::ProcGroup &pg = *pg_;
  if (backend_ != Backend::Device || pg.size() == 1) return;
  struct DevId {
    int64_t ordinal;
    uint64_t bus;
  };
  std::vector<DevId> mine;
  for (int g : gpus_) {
    char bus[64] = {0};
    HIP_CHECK(hipDeviceGetPCIBusId(bus, sizeof(bus), g));
    mine.push_back(DevId{g, uint64_t(std::hash<std::string>()(std::string(bus)))});
  }
  std::vector<int> counts;
  const std::vector<DevId> all = allgather_padded(pg, mine, DevId{-1, 0}, &counts);
  const size_t maxN = all.size() / size_t(pg.size());
  for (int r = 0; r < pg.size(); ++r)
    for (int k = 0; k < counts[size_t(r)]; ++k) {
      const DevId &a = all[size_t(r) * maxN + size_t(k)];
      bool sh = false;
      for (int r2 = 0; r2 < pg.size() && !sh; ++r2) {
        if (r2 == r || pg.hostname(r2) != pg.hostname(r)) continue;
        for (int k2 = 0; k2 < counts[size_t(r2)]; ++k2) sh |= all[size_t(r2) * maxN + size_t(k2)].bus == a.bus;
      }
      impl_->sharedDev[{r, int(a.ordinal)}] = sh;
    }
}

// the channel of (method, direction, local sub-domain, remote sub-domain), appended to `chans` on first use
static Channel &channel_for(std::vector<Channel> &chans, const Placement &pl, MethodFlags m, bool send, int localDom,
                            const Dim3 &localIdx, const Dim3 &remoteIdx) {
  for (Channel &c : chans)
    if (c.method == m && c.send == send && c.localDom == localDom && c.remoteIdx == remoteIdx) return c;
  const Dim3 gdim = pl.dim();
  const int64_t numSub = gdim.flatten();
  Channel c;
  c.method = m;
  c.send = send;
  c.localDom = localDom;
  c.localIdx = localIdx;
  c.remoteIdx = remoteIdx;
  c.remoteRank = pl.get_rank(remoteIdx);
  c.remoteId = pl.get_subdomain_id(remoteIdx);
  c.remoteDev = pl.get_device(remoteIdx);
  c.localDev = pl.get_device(localIdx);
  // order key and tag name the (source, destination) pair of sub-domains: the same on both ends of the channel
  const int64_t sl = linearize(send ? localIdx : remoteIdx, gdim), dl = linearize(send ? remoteIdx : localIdx, gdim);
  c.orderKey = sl * numSub + dl;
  c.tag = comm::make_tag(comm::MsgKind::Data, sl, dl, numSub);
  chans.push_back(c);
  return chans.back();
}

// plan messages (reference src/stencil.cu:132-239). Reads placement_, domains_, flags_ and Impl::sharedDev; leaves
// plan_, remoteHalo_, I.chans (messages sorted, bytes set), I.localTranslates, I.pipeMsgs and timePlan_.
void DistributedDomain::plan_messages() {
  Impl &I = *impl_;
  comm::ProcGroup &pg = *pg_;
  const int myRank = pg.rank();
  const bool dev = backend_ == Backend::Device;
  const double t0 = now_s();
  const Dim3 gdim = placement_->dim();
  auto can_access = [&](int a, int b) {
    if (a == b) return true;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, a, b) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    return can != 0;
  };
  bool warnedShared = false;
  auto choose = [&](int srcRank, int srcDev, int dstRank, int dstDev) -> MethodFlags {
    const bool sameRank = srcRank == dstRank;
    PairInfo pi;
    pi.device = dev;
    pi.sameRank = sameRank;
    pi.sameDevice = srcDev == dstDev;
    pi.sameHost = pg.hostname(srcRank) == pg.hostname(dstRank);
    if (dev) {
      pi.peer = sameRank && gpu_topo::peer(srcDev, dstDev);
      pi.canAccess = !sameRank && pi.sameHost && (any_methods(MethodFlags::Colocated)) && can_access(srcDev, dstDev);
      pi.sharedGpu = !sameRank && (I.shared_dev(srcRank, srcDev) || I.shared_dev(dstRank, dstDev));
    }
    const MethodFlags m = select_method(flags_, pi);
    if (m == MethodFlags::Staged && pi.sharedGpu && any_methods(MethodFlags::Rccl) && !warnedShared) {
      warnedShared = true;
      LOG_WARN("rank " << srcRank << " dev " << srcDev << " -> rank " << dstRank << " dev " << dstDev
                       << ": a GPU driven by two ranks cannot use RCCL; host-staged for such pairs");
    }
    return m;
  };

  plan_.clear();
  remoteHalo_.assign(domains_.size(), std::array<uint8_t, 27>{});
  for (size_t di = 0; di < domains_.size(); ++di) {
    const Dim3 myIdx = placement_->get_idx(myRank, int(di));
    const int myDev = placement_->get_device(myIdx);
    for (int i = 0; i < 27; ++i) {
      const Dim3 dir = dir_from_index(i);
      if (dir == Dim3(0, 0, 0) || radius_.dir(-dir) == 0) continue;
      // send (nothing crosses a non-periodic face of the global grid)
      if (boundary_.reachable(myIdx, dir, gdim)) {
        const Dim3 dstIdx = (myIdx + dir).wrap(gdim);
        const int dstRank = placement_->get_rank(dstIdx), dstId = placement_->get_subdomain_id(dstIdx),
                  dstDev = placement_->get_device(dstIdx);
        const MethodFlags m = choose(myRank, myDev, dstRank, dstDev);
        if (m == MethodFlags::None) LOG_FATAL("no method available to send " << myIdx << " -> " << dstIdx << " dir " << dir);
        int64_t bytes = 0;
        for (int64_t q = 0; q < domains_[di].num_data(); ++q) bytes += domains_[di].halo_bytes(-dir, q);
        plan_.push_back({m, myIdx, dstIdx, myRank, dstRank, myDev, dstDev, dir, bytes});
        if (m == MethodFlags::PeerCopy && topt_.peerCopy == TransportOptions::Copy::Engine && dstId != int(di) && dev)
          I.pipeMsgs[{int(di), dstId}].push_back(Message{dir, int(di), dstId});
        else if (m == MethodFlags::Kernel || m == MethodFlags::PeerCopy)
          I.localTranslates.emplace_back(int(di), dstId, dir);
        else
          channel_for(I.chans, *placement_, m, true, int(di), myIdx, dstIdx).msgs.push_back(Message{dir, int(di), dstId});
      }
      // recv
      if (boundary_.reachable(myIdx, -dir, gdim)) {
        const Dim3 srcIdx = (myIdx - dir).wrap(gdim);
        const int srcRank = placement_->get_rank(srcIdx), srcId = placement_->get_subdomain_id(srcIdx),
                  srcDev = placement_->get_device(srcIdx);
        const MethodFlags m = choose(srcRank, srcDev, myRank, myDev);
        if (m == MethodFlags::None) LOG_FATAL("no method available to recv " << srcIdx << " -> " << myIdx);
        // the halo on side -dir is valid after the same-device translate only for Kernel messages
        if (m != MethodFlags::Kernel) remoteHalo_[di][size_t(dir_index(-dir))] = 1;
        if (m == MethodFlags::Kernel || m == MethodFlags::PeerCopy) continue; // written by the sender directly
        channel_for(I.chans, *placement_, m, false, int(di), myIdx, srcIdx).msgs.push_back(Message{dir, srcId, int(di)});
      }
    }
  }
  for (auto &c : I.chans) {
    std::sort(c.msgs.begin(), c.msgs.end());
    c.bytes = packed_size(domains_[c.localDom], c.msgs);
  }
  timePlan_ = setup_time(pg, now_s() - t0);
}

// pack (send channels) or unpack segments of the channels `cis` into variant parity * slots + slot of `out`, against
// the buffer buf(channel, slot) (reference wire layout: messages sorted by dir, each quantity aligned to its element
// size, reference packer.cuh:136-160)
template <typename BufFn>
static void build_channel_segs(const std::vector<LocalDomain> &doms, std::vector<Channel> &chans,
                               const std::vector<int> &cis, SegList &out, int slots, BufFn buf) {
  for (int ci : cis) {
    Channel &c = chans[size_t(ci)];
    for (int p = 0; p < 2; ++p)
      for (int slot = 0; slot < slots; ++slot)
        (c.send ? build_pack_segs : build_unpack_segs)(doms[size_t(c.localDom)], c.msgs, buf(c, slot), p == 0,
                                                       out.host[p * slots + slot]);
  }
}
// the channel's own buffer of `bytes`: dbuf on the device, hostBuf on the host backend
static char *staging_buffer(Channel &c, int) { return c.dbuf ? c.dbuf : c.hostBuf.data(); }

// host backend: translate + staged only, all executed on the host. Reads I.localTranslates and I.chans; leaves the
// channels' host buffers and the three host segment lists.
void DistributedDomain::create_host_transports() {
  Impl &I = *impl_;
  for (const auto &t : I.localTranslates) {
    const LocalDomain &s = domains_[std::get<0>(t)], &d = domains_[std::get<1>(t)];
    for (int p = 0; p < 2; ++p)
      build_translate_segs(s, d, std::get<2>(t), p == 0, I.hostTranslate.host[p], topt_.xFaceSectors);
  }
  for (int ci = 0; ci < int(I.chans.size()); ++ci) {
    Channel &c = I.chans[size_t(ci)];
    STENCIL_REQUIRE(c.method == MethodFlags::Staged, "host backend supports only Kernel/Staged transports");
    c.hostBuf.resize(size_t(std::max<int64_t>(c.bytes, 1)));
    build_channel_segs(domains_, I.chans, {ci}, c.send ? I.hostStagedPack : I.hostStagedUnpack, 1, staging_buffer);
  }
  I.hostTranslate.upload(-1);
  I.hostStagedPack.upload(-1);
  I.hostStagedUnpack.upload(-1);
}

// device backend. Reads domains_, I.chans, I.localTranslates, I.pipeMsgs and I.sharedDev; every step reads what the
// steps before it left in Impl.
void DistributedDomain::create_device_transports() {
  create_device_contexts();
  init_rccl();
  build_local_translates();
  create_pipes();
  allocate_channel_buffers();
  ipc_handshake();
  build_channel_lists();
}

// Leaves one DevCtx per distinct local device (stream, events, its sub-domains), the ready events per sub-domain and
// the host-mapped error and done words.
void DistributedDomain::create_device_contexts() {
  Impl &I = *impl_;
  for (size_t di = 0; di < domains_.size(); ++di) {
    const int d = domains_[di].gpu();
    if (!I.devIndex.count(d)) {
      I.devIndex[d] = int(I.devs.size());
      I.devs.emplace_back();
      DevCtx &c = I.devs.back();
      c.dev = d;
      c.comm = Stream(d, Priority::HIGH);
      c.done = Event(d);
      c.translated = Event(d);
      if (!I.callerDone) I.callerDone = Event(d);
    }
    I.devs[I.devIndex[d]].doms.push_back(int(di));
    I.ready.emplace_back(d);
    I.readyPending.push_back(false);
  }
  HIP_CHECK(hipHostMalloc((void **)&I.errHost, sizeof(int), hipHostMallocMapped));
  *I.errHost = 0;
  HIP_CHECK(hipHostGetDevicePointer((void **)&I.errDev, I.errHost, 0));
  HIP_CHECK(hipHostMalloc((void **)&I.doneHost, sizeof(uint64_t) * I.devs.size(), hipHostMallocMapped));
  for (size_t k = 0; k < I.devs.size(); ++k) I.doneHost[k] = 0;
  HIP_CHECK(hipHostGetDevicePointer((void **)&I.doneDev, I.doneHost, 0));
  I.nullReady = Event(I.devs[0].dev);
}

void DistributedDomain::build_translates(int slot, int skipAxes) {
  Impl &I = *impl_;
  for (const auto &t : I.localTranslates) {
    const Dim3 dir = std::get<2>(t);
    if (crosses(dir, skipAxes)) continue;
    const LocalDomain &s = domains_[std::get<0>(t)], &d = domains_[std::get<1>(t)];
    DevCtx &ctx = I.devs[I.devIndex[s.gpu()]];
    SegList &list = slot == 0 ? ctx.translate : ctx.translateSkip;
    for (int p = 0; p < 2; ++p) build_translate_segs(s, d, dir, p == 0, list.host[p], x_face_lines(s, d));
  }
}

// same-process direct stores; x faces as whole lines where asked for or where their lines outgrow the cache.
// Reads I.localTranslates; leaves I.xLineDevs, the translate lists (uploaded with the channel lists) and peerWriters.
void DistributedDomain::build_local_translates() {
  Impl &I = *impl_;
  std::map<int, int64_t> xLineBytes;
  for (const auto &t : I.localTranslates) {
    const LocalDomain &s = domains_[std::get<0>(t)], &d = domains_[std::get<1>(t)];
    const Dim3 dir = std::get<2>(t);
    if (dir.x != 0 && dir.y == 0 && dir.z == 0 && s.gpu() == d.gpu())
      xLineBytes[s.gpu()] += s.size().y * s.size().z * s.num_data() * 192;
    if (d.gpu() != s.gpu()) I.devs[I.devIndex[d.gpu()]].peerWriters.insert(s.gpu());
  }
  for (auto &kv : xLineBytes)
    if (topt_.xFaceSectors || (topt_.xFaceLinesAutoBytes > 0 && kv.second >= topt_.xFaceLinesAutoBytes))
      I.xLineDevs.insert(kv.first);
  if (!I.xLineDevs.empty() && !topt_.xFaceSectors)
    LOG_DEBUG("x faces as whole lines (auto) on " << I.xLineDevs.size() << " device(s)");
  build_translates(0, 0);
}

void DistributedDomain::build_pipe_segs(int slot, int skipAxes) {
  Impl &I = *impl_;
  for (auto &pp : I.pipes) {
    std::vector<Message> keep;
    for (const Message &m : pp.msgs)
      if (!crosses(m.dir, skipAxes)) keep.push_back(m);
    pp.bytes[slot] = keep.empty() ? 0 : packed_size(domains_[size_t(pp.srcDom)], keep);
    if (keep.empty()) continue;
    DevCtx &sc = I.devs[size_t(I.devIndex[pp.srcDev])];
    DevCtx &dc = I.devs[size_t(I.devIndex[pp.dstDev])];
    for (int p = 0; p < 2; ++p) {
      build_pack_segs(domains_[size_t(pp.srcDom)], keep, pp.sbuf, p == 0, sc.pipePack[slot].host[p]);
      build_unpack_segs(domains_[size_t(pp.dstDom)], keep, pp.rbuf, p == 0, dc.pipeUnpack[slot].host[p]);
    }
  }
}

// Reads I.pipeMsgs; leaves I.pipes with their buffers and the pipe lists [0] uploaded, then per device the pipe
// events, sharedGpu and the zeroed block counters.
void DistributedDomain::create_pipes() {
  Impl &I = *impl_;
  for (auto &kv : I.pipeMsgs) {
    PeerPipe pp;
    pp.srcDom = kv.first.first;
    pp.dstDom = kv.first.second;
    pp.srcDev = domains_[size_t(pp.srcDom)].gpu();
    pp.dstDev = domains_[size_t(pp.dstDom)].gpu();
    pp.msgs = kv.second;
    std::sort(pp.msgs.begin(), pp.msgs.end());
    pp.bytes[0] = pp.bytes[1] = packed_size(domains_[size_t(pp.srcDom)], pp.msgs);
    const size_t nb = size_t(std::max<int64_t>(pp.bytes[0], 1));
    HIP_CHECK(hipSetDevice(pp.srcDev));
    HIP_CHECK(hipMalloc(&pp.sbuf, nb));
    HIP_CHECK(hipSetDevice(pp.dstDev));
    HIP_CHECK(hipMalloc(&pp.rbuf, nb));
    const int k = int(I.pipes.size());
    I.devs[size_t(I.devIndex[pp.srcDev])].pipesOut.push_back(k);
    I.devs[size_t(I.devIndex[pp.dstDev])].pipesIn.push_back(k);
    I.pipes.push_back(std::move(pp));
  }
  build_pipe_segs(0, 0);
  for (auto &ctx : I.devs) {
    ctx.sharedGpu = I.shared_dev(rank(), ctx.dev);
    ctx.pipePack[0].upload(ctx.dev);
    ctx.pipeUnpack[0].upload(ctx.dev);
    if (!ctx.pipesOut.empty()) ctx.pipeSent = Event(ctx.dev);
    if (!ctx.pipesIn.empty()) ctx.pipeUnpacked = Event(ctx.dev);
    HIP_CHECK(hipSetDevice(ctx.dev));
    HIP_CHECK(hipMalloc(&ctx.syncCounter, 2 * sizeof(uint32_t)));
    HIP_CHECK(hipMemset(ctx.syncCounter, 0, 2 * sizeof(uint32_t)));
  }
  // copy streams for DMA-engine copies are created on first use (forked_copies): every stream can take a hardware
  // queue, and ranks that share a GPU slow down by orders of magnitude once their queues oversubscribe the
  // device (profiles/r3/cliff/)
}

// Reads I.chans (method, bytes); leaves every channel's device and pinned buffers and the per-device channel index
// lists, and the devices synchronized (the memsets have landed before a handle leaves the process).
void DistributedDomain::allocate_channel_buffers() {
  Impl &I = *impl_;
  for (int ci = 0; ci < int(I.chans.size()); ++ci) {
    Channel &c = I.chans[ci];
    DevCtx &ctx = I.devs[I.devIndex[c.localDev]];
    HIP_CHECK(hipSetDevice(c.localDev));
    const size_t nb = size_t(std::max<int64_t>(c.bytes, 1));
    if (c.method == MethodFlags::Staged) {
      HIP_CHECK(hipMalloc(&c.dbuf, nb));
      // pinned on the GPU's NUMA node when realize() bound this thread there (pages follow the thread's policy)
      HIP_CHECK(hipHostMalloc((void **)&c.hbuf, nb, numaNode_ >= 0 ? hipHostMallocNumaUser : hipHostMallocDefault));
      (c.send ? ctx.stagedSend : ctx.stagedRecv).push_back(ci);
    } else if (c.method == MethodFlags::Rccl) {
      HIP_CHECK(hipMalloc(&c.dbuf, nb));
      (c.send ? ctx.rcclSend : ctx.rcclRecv).push_back(ci);
    } else if (c.method == MethodFlags::Colocated) {
      // flag words (arrival on the receiver, credit on the sender) in uncached memory: polled across processes
      // and GPUs, written remotely
      HIP_CHECK(hipExtMallocWithFlags((void **)&c.ownFlag, 256, hipDeviceMallocUncached));
      HIP_CHECK(hipMemset(c.ownFlag, 0, 256));
      c.slotStride = round_up(int64_t(nb), 256);
      if (!c.send) {
        const size_t dataBytes = size_t(2 * c.slotStride);
        switch (topt_.inbox) {
        case TransportOptions::Inbox::Uncached:
          HIP_CHECK(hipExtMallocWithFlags((void **)&c.ownData, dataBytes, hipDeviceMallocUncached));
          break;
        case TransportOptions::Inbox::Fine:
          HIP_CHECK(hipExtMallocWithFlags((void **)&c.ownData, dataBytes, hipDeviceMallocFinegrained));
          break;
        case TransportOptions::Inbox::Coarse:
          HIP_CHECK(hipMalloc((void **)&c.ownData, dataBytes));
          break;
        }
        HIP_CHECK(hipMemset(c.ownData, 0, dataBytes));
      } else {
        HIP_CHECK(hipMalloc(&c.dbuf, nb)); // Engine copies: the packed message before the DMA copy
      }
      (c.send ? ctx.coloSend : ctx.coloRecv).push_back(ci);
    }
  }
  HIP_CHECK(hipDeviceSynchronize());
}

// IPC handshake for colocated channels: every side sends its handles first (non-blocking), then receives.
// receiver -> sender: {arrival flag block, data block}; sender -> receiver: {credit flag block}.
// Reads the Colocated channels' own blocks; leaves their remote mappings and, with Completion::IpcEvent, their
// interprocess events. Ends with a barrier.
void DistributedDomain::ipc_handshake() {
  Impl &I = *impl_;
  comm::ProcGroup &pg = *pg_;
  TraceRange tri("ipc handshake");
  for (auto &c : I.chans) {
    if (c.method != MethodFlags::Colocated) continue;
    hipIpcMemHandle_t h[2] = {};
    HIP_CHECK(hipSetDevice(c.localDev));
    HIP_CHECK(hipIpcGetMemHandle(&h[0], c.ownFlag));
    if (!c.send) HIP_CHECK(hipIpcGetMemHandle(&h[1], c.ownData));
    pg.send(c.remoteRank, retag(c.tag, c.send ? comm::MsgKind::IpcCredit : comm::MsgKind::IpcInbox), h,
            c.send ? sizeof(h[0]) : sizeof(h));
  }
  for (auto &c : I.chans) {
    if (c.method != MethodFlags::Colocated) continue;
    hipIpcMemHandle_t h[2] = {};
    // a sender needs the receiver's flag + data blocks, a receiver the sender's credit block
    pg.recv(c.remoteRank, retag(c.tag, c.send ? comm::MsgKind::IpcInbox : comm::MsgKind::IpcCredit), h,
            c.send ? sizeof(h) : sizeof(h[0]));
    HIP_CHECK(hipSetDevice(c.localDev));
    HIP_CHECK(hipIpcOpenMemHandle((void **)&c.remoteFlag, h[0], hipIpcMemLazyEnablePeerAccess));
    if (c.send) HIP_CHECK(hipIpcOpenMemHandle((void **)&c.remoteData, h[1], hipIpcMemLazyEnablePeerAccess));
  }
  // Completion::IpcEvent: sender -> receiver, the handle of the sender's interprocess event per channel
  if (topt_.completion == TransportOptions::Completion::IpcEvent) {
    for (auto &c : I.chans) {
      if (c.method != MethodFlags::Colocated || !c.send) continue;
      HIP_CHECK(hipSetDevice(c.localDev));
      HIP_CHECK(hipEventCreateWithFlags(&c.ipcEvent, hipEventDisableTiming | hipEventInterprocess));
      hipIpcEventHandle_t h{};
      HIP_CHECK(hipIpcGetEventHandle(&h, c.ipcEvent));
      pg.send(c.remoteRank, retag(c.tag, comm::MsgKind::IpcEvent), &h, sizeof(h));
    }
    for (auto &c : I.chans) {
      if (c.method != MethodFlags::Colocated || c.send) continue;
      hipIpcEventHandle_t h{};
      pg.recv(c.remoteRank, retag(c.tag, comm::MsgKind::IpcEvent), &h, sizeof(h));
      HIP_CHECK(hipSetDevice(c.localDev));
      HIP_CHECK(hipIpcOpenEventHandle(&c.ipcEvent, h));
    }
    I.ipcEvents = true;
    I.ipcEventFirstEpoch = 1;
  }
  pg.barrier();
}

// segment lists per device. Reads the channels' buffers and mappings; leaves every channel list and the translate
// list uploaded, and the RCCL channels in matching order.
void DistributedDomain::build_channel_lists() {
  Impl &I = *impl_;
  // a Colocated sender packs into the receiver's mapped inbox slots (or, for engine copies, its own staging buffer), and
  // the receiver unpacks its own slots
  auto remote_slot = [](Channel &c, int slot) { return c.remoteData + slot * c.slotStride; };
  auto own_slot = [](Channel &c, int slot) { return c.ownData + slot * c.slotStride; };
  for (auto &ctx : I.devs) {
    build_channel_segs(domains_, I.chans, ctx.coloSend, ctx.coloPack, 2, remote_slot);
    build_channel_segs(domains_, I.chans, ctx.coloSend, ctx.coloPackLocal, 1, staging_buffer);
    build_channel_segs(domains_, I.chans, ctx.coloRecv, ctx.coloUnpack, 2, own_slot);
    build_channel_segs(domains_, I.chans, ctx.rcclSend, ctx.rcclPack, 1, staging_buffer);
    build_channel_segs(domains_, I.chans, ctx.rcclRecv, ctx.rcclUnpack, 1, staging_buffer);
    build_channel_segs(domains_, I.chans, ctx.stagedSend, ctx.stagedPack, 1, staging_buffer);
    build_channel_segs(domains_, I.chans, ctx.stagedRecv, ctx.stagedUnpack, 1, staging_buffer);
    ctx.upload();
    // RCCL matching order: canonical (src, dst) sub-domain order on both sides of every pair
    auto byKey = [&](int a, int b) { return I.chans[a].orderKey < I.chans[b].orderKey; };
    std::sort(ctx.rcclSend.begin(), ctx.rcclSend.end(), byKey);
    std::sort(ctx.rcclRecv.begin(), ctx.rcclRecv.end(), byKey);
  }
}

// bytes per method (after any RCCL -> staged fallback) and the plan file. Leaves bytesPerMethod_, timeCreate_ (the
// transports, from createStart) and realized_; ends with a barrier.
void DistributedDomain::finish_plan(double createStart) {
  comm::ProcGroup &pg = *pg_;
  bytesPerMethod_ = {};
  for (const auto &e : plan_) bytesPerMethod_[size_t(method_slot(e.method))] += uint64_t(e.bytes);
  for (int m = 0; m < 5; ++m) bytesPerMethod_[size_t(m)] = pg.allreduce_sum_u64(bytesPerMethod_[size_t(m)]);
  if (!planPrefix_.empty()) {
    std::ofstream f(planPrefix_ + "_" + std::to_string(pg.rank()) + ".txt");
    f << plan_summary();
  }
  timeCreate_ = setup_time(pg, now_s() - createStart);
  realized_ = true;
  pg.barrier();
}

std::string DistributedDomain::plan_summary() const {
  std::ostringstream ss;
  ss << "rank=" << rank() << "\n\n== domains ==\n";
  for (size_t di = 0; di < domains_.size(); ++di)
    ss << di << ":dev" << domains_[di].gpu() << ":" << placement_->get_idx(rank(), int(di)) << " sz=" << domains_[di].size()
       << " origin=" << domains_[di].origin() << "\n";
  const MethodFlags order[] = {MethodFlags::Kernel, MethodFlags::PeerCopy, MethodFlags::Colocated, MethodFlags::Rccl,
                               MethodFlags::Staged};
  for (MethodFlags m : order) {
    ss << "\n== " << to_string(m) << " ==\n";
    for (const auto &e : plan_)
      if (e.method == m)
        ss << e.srcIdx << "(r" << e.srcRank << " dev" << e.srcDev << ") -> " << e.dstIdx << "(r" << e.dstRank << " dev"
           << e.dstDev << ") dir=" << e.dir << " " << e.bytes << "B\n";
  }
  ss << "\n== bytes per exchange (all ranks) ==\n";
  for (MethodFlags m : order) ss << to_string(m) << " " << bytesPerMethod_[method_slot(m)] << "\n";
  return ss.str();
}

std::vector<ForwardTarget> DistributedDomain::forward_targets(size_t di) const {
  STENCIL_REQUIRE(realized_, "forward_targets before realize()");
  const Dim3 myIdx = placement_->get_idx(rank(), int(di));
  const Dim3 gdim = placement_->dim();
  const LocalDomain &src = domains_.at(di);
  std::vector<ForwardTarget> out;
  for (const auto &e : plan_) {
    if (e.srcIdx != myIdx || (e.method != MethodFlags::Kernel && e.method != MethodFlags::PeerCopy)) continue;
    const LocalDomain &dst = domains_.at(size_t(placement_->get_subdomain_id(e.dstIdx)));
    // global coordinate of the receiving halo cell = sender's cell - wrap, where wrap = +-global size when the
    // step crosses the periodic boundary
    const Dim3 step = myIdx + e.dir;
    Dim3 wrap(0, 0, 0);
    wrap.x = step.x >= gdim.x ? size_.x : (step.x < 0 ? -size_.x : 0);
    wrap.y = step.y >= gdim.y ? size_.y : (step.y < 0 ? -size_.y : 0);
    wrap.z = step.z >= gdim.z ? size_.z : (step.z < 0 ? -size_.z : 0);
    out.push_back(ForwardTarget{e.dir, &dst, src.accessor_origin() - dst.accessor_origin() - wrap});
  }
  return out;
}

uint64_t DistributedDomain::exchange_bytes_for_method(MethodFlags m) const {
  uint64_t r = 0;
  const MethodFlags all[] = {MethodFlags::Staged, MethodFlags::Rccl, MethodFlags::Colocated, MethodFlags::PeerCopy,
                             MethodFlags::Kernel};
  for (MethodFlags f : all)
    if (m && f) r += bytesPerMethod_[method_slot(f)];
  return r;
}

// ------------------------------------------------------------------------------------------------
// interior / exterior (reference src/stencil.cu:567-666)
// ------------------------------------------------------------------------------------------------
std::vector<Rect3> DistributedDomain::get_interior() const {
  std::vector<Rect3> ret(domains_.size());
  for (size_t di = 0; di < domains_.size(); ++di) {
    const Rect3 com = domains_[di].get_compute_region();
    Rect3 in = com;
    for (int i = 0; i < 27; ++i) {
      const Dim3 d = dir_from_index(i);
      if (d == Dim3(0, 0, 0)) continue;
      const int64_t r = radius_.dir(d);
      if (d.x < 0) in.lo.x = std::max(com.lo.x + r, in.lo.x);
      if (d.x > 0) in.hi.x = std::min(com.hi.x - r, in.hi.x);
      if (d.y < 0) in.lo.y = std::max(com.lo.y + r, in.lo.y);
      if (d.y > 0) in.hi.y = std::min(com.hi.y - r, in.hi.y);
      if (d.z < 0) in.lo.z = std::max(com.lo.z + r, in.lo.z);
      if (d.z > 0) in.hi.z = std::min(com.hi.z - r, in.hi.z);
    }
    ret[di] = in;
  }
  return ret;
}

std::vector<Rect3> DistributedDomain::get_local_interior(int reach) const {
  STENCIL_REQUIRE(realized_, "get_local_interior before realize()");
  std::vector<Rect3> ret(domains_.size());
  for (size_t di = 0; di < domains_.size(); ++di) {
    const Rect3 com = domains_[di].get_compute_region();
    const auto &rh = remoteHalo_[di];
    // shrink[axis][side]: cells to drop at the low (0) / high (1) face of each axis
    int64_t sh[3][2] = {{0, 0}, {0, 0}, {0, 0}};
    auto comp = [](const Dim3 &d, int a) { return a == 0 ? d.x : (a == 1 ? d.y : d.z); };
    // remote faces: the stencil reaches `reach` cells along an axis
    for (int i = 0; i < 27; ++i) {
      const Dim3 d = dir_from_index(i);
      const int nz = (d.x != 0) + (d.y != 0) + (d.z != 0);
      if (nz != 1 || !rh[size_t(i)]) continue;
      for (int a = 0; a < 3; ++a)
        if (comp(d, a) != 0) sh[a][comp(d, a) > 0] = std::max<int64_t>(sh[a][comp(d, a) > 0], std::min<int64_t>(reach, radius_.dir(d)));
    }
    // remote edges / corners: a cell reads them only when it is within reach of all their faces at once, so one
    // shrunk face among them covers the rest; with none, drop every face of the direction (conservative)
    for (int i = 0; i < 27; ++i) {
      const Dim3 d = dir_from_index(i);
      const int nz = (d.x != 0) + (d.y != 0) + (d.z != 0);
      if (nz < 2 || !rh[size_t(i)] || radius_.dir(d) == 0) continue;
      bool covered = false;
      for (int a = 0; a < 3; ++a)
        if (comp(d, a) != 0 && sh[a][comp(d, a) > 0] > 0) covered = true;
      if (covered) continue;
      for (int a = 0; a < 3; ++a)
        if (comp(d, a) != 0) sh[a][comp(d, a) > 0] = std::max<int64_t>(sh[a][comp(d, a) > 0], 1);
    }
    // measurement knob: treat the faces of these axes (mask 1=x, 2=y, 4=z) as remote, so one GPU runs the split
    // (local interior during the transfers, slabs after) of a multi-GPU decomposition
    if (topt_.fakeRemoteAxes != 0)
      for (int a = 0; a < 3; ++a)
        if (topt_.fakeRemoteAxes >> a & 1)
          for (int s = 0; s < 2; ++s) {
            const Dim3 d(a == 0 ? 2 * s - 1 : 0, a == 1 ? 2 * s - 1 : 0, a == 2 ? 2 * s - 1 : 0);
            sh[a][s] = std::max<int64_t>(sh[a][s], std::min<int64_t>(reach, radius_.dir(d)));
          }
    Rect3 in = com;
    in.lo.x += sh[0][0];
    in.hi.x -= sh[0][1];
    in.lo.y += sh[1][0];
    in.hi.y -= sh[1][1];
    in.lo.z += sh[2][0];
    in.hi.z -= sh[2][1];
    if (in.hi.x < in.lo.x || in.hi.y < in.lo.y || in.hi.z < in.lo.z) in = Rect3(com.lo, com.lo);
    ret[di] = in;
  }
  return ret;
}

std::vector<std::vector<Rect3>> DistributedDomain::get_exterior() const {
  std::vector<std::vector<Rect3>> ret(domains_.size());
  const auto ins = get_interior();
  for (size_t di = 0; di < domains_.size(); ++di) {
    const Rect3 &in = ins[di];
    Rect3 c = domains_[di].get_compute_region();
    if (in.hi.x != c.hi.x) {
      ret[di].push_back(Rect3(Dim3(in.hi.x, c.lo.y, c.lo.z), c.hi));
      c.hi.x = in.hi.x;
    }
    if (in.hi.y != c.hi.y) {
      ret[di].push_back(Rect3(Dim3(c.lo.x, in.hi.y, c.lo.z), c.hi));
      c.hi.y = in.hi.y;
    }
    if (in.hi.z != c.hi.z) {
      ret[di].push_back(Rect3(Dim3(c.lo.x, c.lo.y, in.hi.z), c.hi));
      c.hi.z = in.hi.z;
    }
    if (in.lo.x != c.lo.x) {
      ret[di].push_back(Rect3(c.lo, Dim3(in.lo.x, c.hi.y, c.hi.z)));
      c.lo.x = in.lo.x;
    }
    if (in.lo.y != c.lo.y) {
      ret[di].push_back(Rect3(c.lo, Dim3(c.hi.x, in.lo.y, c.hi.z)));
      c.lo.y = in.lo.y;
    }
    if (in.lo.z != c.lo.z) {
      ret[di].push_back(Rect3(c.lo, Dim3(c.hi.x, c.hi.y, in.lo.z)));
      c.lo.z = in.lo.z;
    }
  }
  return ret;
}

} // namespace stencil
