#include "stencil/models/stencil_model.hpp"

#include <algorithm>

#include "stencil/rt/hip_check.hpp"
#include "stencil/rt/trace.hpp"

namespace stencil {

int spanned_axes(const Rect3 &compute, const Rect3 &swept) {
  int w = 7;
  if (swept.lo.x != compute.lo.x || swept.hi.x != compute.hi.x) w &= ~1;
  if (swept.lo.y != compute.lo.y || swept.hi.y != compute.hi.y) w &= ~2;
  if (swept.lo.z != compute.lo.z || swept.hi.z != compute.hi.z) w &= ~4;
  return w;
}

bool spheres_clear_of_faces(const Spheres &sph, const Dim3 &L, int64_t lo, int64_t hi) {
  for (const Dim3 &c : {sph.hot, sph.cold}) {
    const int64_t cc[3] = {c.x, c.y, c.z}, ll[3] = {L.x, L.y, L.z};
    for (int a = 0; a < 3; ++a)
      if (cc[a] - sph.radius < lo || cc[a] + sph.radius > ll[a] - hi) return false;
  }
  return true;
}

// the shell of `c` around `in`: z slabs over the whole xy extent, y slabs between them, x slabs between those
static std::vector<Rect3> shell_slabs(const Rect3 &c, const Rect3 &in) {
  std::vector<Rect3> out;
  for (const Rect3 &r : {Rect3(c.lo, Dim3(c.hi.x, c.hi.y, in.lo.z)), Rect3(Dim3(c.lo.x, c.lo.y, in.hi.z), c.hi),
                         Rect3(Dim3(c.lo.x, c.lo.y, in.lo.z), Dim3(c.hi.x, in.lo.y, in.hi.z)),
                         Rect3(Dim3(c.lo.x, in.hi.y, in.lo.z), Dim3(c.hi.x, c.hi.y, in.hi.z)),
                         Rect3(Dim3(c.lo.x, in.lo.y, in.lo.z), Dim3(in.lo.x, in.hi.y, in.hi.z)),
                         Rect3(Dim3(in.hi.x, in.lo.y, in.lo.z), Dim3(c.hi.x, in.hi.y, in.hi.z))})
    if (!r.empty()) out.push_back(r);
  return out;
}

StencilModel::StencilModel(const StencilModelConfig &cfg, std::shared_ptr<comm::ProcGroup> pg) : cfg_(cfg) {
  dd_.reset(new DistributedDomain(cfg.size.x, cfg.size.y, cfg.size.z, pg));
  pubDepth_ = cfg.temporal >= 3 ? 3 : 2;
  Radius r = Radius::constant(0);
  if (cfg.allDirections) {
    r = Radius::constant(cfg.radius);
  } else {
    r.set_face(cfg.radius);
  }
  if (cfg.temporal >= 2) {
    // S o S of a 7-point stencil reaches 2 cells along an axis and 1 cell diagonally (edges), never corners;
    // S o S o S 3 along an axis, (1, 2) / (2, 1) on edges and (1, 1, 1) in corners (an edge / corner halo spans the
    // face depths of its axes, LocalDomain::halo_extent, so a nonzero radius is enough). Corners matter only where x
    // is read from halos (the triples' XH form); wherever x wraps in-kernel their messages are skipped with the other
    // self copies or carry a few hundred bytes
    const int64_t face = cfg.temporal >= 3 ? 3 : 2;
    for (int i = 0; i < 27; ++i) {
      const Dim3 d = dir_from_index(i);
      const int nz = (d.x != 0) + (d.y != 0) + (d.z != 0);
      if (nz == 1) r.dir(d) = std::max<int64_t>(r.dir(d), face);
      if (nz == 2 || (nz == 3 && cfg.temporal >= 3)) r.dir(d) = std::max<int64_t>(r.dir(d), 1);
    }
  }
  dd_->set_radius(r);
  dd_->set_methods(cfg.methods);
  dd_->set_placement(cfg.placement);
  dd_->set_axis_cost(cfg.axisCost);
  dd_->set_partition_objective(cfg.partition);
  if (!cfg.gpus.empty()) dd_->set_gpus(cfg.gpus);
  if (cfg.setBackend) dd_->set_backend(cfg.backend);
  dd_->set_transport_options(cfg.transport);
  dd_->set_x_halo_align(cfg.xHaloAlign);
  dd_->set_shared_halo_line(cfg.sharedHaloLine);
  dd_->set_interior_align(cfg.interiorAlign);
  dd_->set_row_pad_lines(cfg.rowPadLines);
  dd_->set_self_test(cfg.selfTest);
  for (int q = 0; q < cfg.quantities; ++q) {
    const std::string name = cfg.kind == StencilKind::Jacobi && cfg.quantities == 1 ? "d" : "d" + std::to_string(q);
    if (cfg.fp64)
      dd_->add_data<double>(name);
    else
      dd_->add_data<float>(name);
  }
}

StencilModel::~StencilModel() {
  try {
    for (auto &s : compute_) s.sync();
  } catch (...) {
  }
  (void)destroy_graphs();
  if (pubCounter_) (void)hipFree(pubCounter_);
}

int64_t StencilModel::local_cells() const {
  int64_t n = 0;
  for (const auto &d : dd_->domains()) n += d.size().flatten();
  return n;
}

hipStream_t StencilModel::compute_stream(size_t di) const { return compute_.empty() ? nullptr : compute_.at(di).get(); }

bool StencilModel::has_remote_halo(const std::vector<Rect3> &li) const {
  const auto &doms = dd_->domains();
  for (size_t di = 0; di < doms.size(); ++di)
    if (spanned_axes(doms[di].get_compute_region(), li[di]) != 7) return true;
  return false;
}

// Each stage reads what the earlier ones decided, and their side effects on dd_ (set_comm_max_blocks,
// prepare_skip_wrapped, set_translate_max_blocks, the publication counter) feed later decisions: keep the order.
void StencilModel::init() {
  TraceRange tr("StencilModel::init");
  cfg_.tune.wrap = 0; // in-kernel wrap axes are the model's decision (pairTune_ / stepTune_)
  dd_->realize();
  sph_ = cfg_.kind == StencilKind::Jacobi ? Spheres::jacobi(dd_->get_compute_region()) : Spheres();
  decide_overlap_and_forwarding();
  decide_pairs();
  // fused pairs / triples: every compute region shrunk at the faces whose halo arrives from another GPU
  const std::vector<Rect3> li = pairs_ ? dd_->get_local_interior(2) : std::vector<Rect3>();
  decide_pair_overlap(li);
  const bool sameWrap = decide_pair_wrap();
  decide_toggle_and_pipelining(li, sameWrap);
  plan_single_steps();
  decide_triples();
  // graphs: one device sub-domain whose whole step, exchange included, goes on its compute stream
  graphs_ = cfg_.useGraph && !overlap_ && dd_->domains().size() == 1 && on_device() && only_same_gpu_copies() &&
            dd_->world_size() == 1;
  start();
}

// overlap_ as configured, and forward_
void StencilModel::decide_overlap_and_forwarding() {
  overlap_ = cfg_.overlap && !(cfg_.autoOverlap && cfg_.transport.fakeRemoteAxes == 0 && only_same_gpu_copies());
  const auto &doms = dd_->domains();
  forward_ = cfg_.forward && dd_->world_size() == 1 && dd_->all_direct() && !doms.empty();
  for (const auto &d : doms)
    for (int64_t q = 0; q < d.num_data() && forward_; ++q) forward_ = HaloForwarder::supported(d, q);
  if (forward_) overlap_ = false; // the halos travel inside the stencil kernel
}

// pairs_: fused pairs are possible
void StencilModel::decide_pairs() {
  const auto &doms = dd_->domains();
  pairs_ = cfg_.temporal >= 2 && !forward_ && !doms.empty();
  // a fused pair computes the intermediate step on the halo ring too, with the sphere test at the halo cell's
  // unwrapped coordinate: across the global periodic boundary that is -1 / L instead of L-1 / 0. The two agree
  // unless a sphere reaches the first or last plane of an axis (only on grids much thinner in y/z than x/10):
  // then run single steps.
  if (pairs_ && sph_.enabled && !spheres_clear_of_faces(sph_, cfg_.size, 1, 2)) {
    pairs_ = false;
    LOG_WARN("Jacobi spheres reach a periodic face of " << cfg_.size << ": temporal blocking off");
  }
  for (const auto &d : doms)
    for (int64_t q = 0; q < d.num_data() && pairs_; ++q) pairs_ = stencil7x2_supported(d, q);
}

// overlap_ for pairs, pairInteriors_, slabsAfter_; reserves the comm CUs
void StencilModel::decide_pair_overlap(const std::vector<Rect3> &li) {
  // Fused pairs overlap against the REMOTE part of the exchange only: the same-device translate (periodic
  // self-wrap, co-resident sub-domains) runs first, then S o S of the local interior (the compute region shrunk
  // only at faces whose halo arrives over IPC / RCCL / staged transports, get_local_interior) while those
  // transports are in flight, then the thin slabs at the remote faces. Measured on one MI355X (512^3,
  // bench_stencil --only ext): with all six faces shrunk the split costs ~90 us of the ~100 us it could hide
  // (interior 308 us + x/y/z slabs 64 us concurrently = 387 us vs 296 us whole), dominated by the x slabs (lanes
  // along strided rows); y/z slabs are row-contiguous. So `auto` overlaps pairs exactly when some halo is remote
  // and no x face is: 2 GPUs (z split) and 4 GPUs (y, z split) of the weak-scaling ladder, not 2x2x2.
  if (pairs_) {
    const auto &doms = dd_->domains();
    const bool remote = has_remote_halo(li);
    bool xcut = false;
    for (size_t di = 0; di < doms.size(); ++di)
      xcut = xcut || !(spanned_axes(doms[di].get_compute_region(), li[di]) & 1);
    if (cfg_.autoOverlap) overlap_ = overlap_ && remote && !xcut;
    // forced overlap without remote halos (one GPU): the classic full split, exercises every slab kernel
    pairInteriors_ = remote ? li : dd_->get_interior();
    for (const auto &r : pairInteriors_) overlap_ = overlap_ && !r.empty();
    // the sweep leaves x2reserve CUs free and the transports' pack/unpack kernels stay on that many CUs
    if (overlap_) dd_->set_comm_max_blocks(cfg_.tune.x2reserve);
  }
  // overlapped pairs with the slabs after the interior sweep (set_overlap_mode(2)) from the start
  slabsAfter_ = pairs_ && overlap_ && cfg_.overlapMode == 2;
}

// Fused triples where the whole-row kernel cannot wrap x (rows other than 512 fp32 cells: the 1024-wide cbrt shape,
// fp64), given the axes `w` the pairs would wrap: read x from halos (the XH form) and leave the x self copies in the
// exchange, one per three steps, instead of falling back to pairs that wrap x. The exception: ragged rows (a partial
// last column of the XH form's 512 fp32 / 256 fp64 cells, stencil7x3_column_cells) of a sub-domain that is periodic
// onto itself along every axis (one GPU, w == 7). There the pairs that wrap x in-kernel won on most shapes measured on
// one MI355X (Gcells/s, triples vs pairs, 3 interleaved repeats, profiles/ragged_triples/): 645x645x323 940-960 vs
// 1072-1078, 645x323x645 983-987 vs 1098-1138, 323x645x645 940-992 vs 1005-1020, 813x813x204 978-993 vs 1039-1053;
// triples won on 813x407x407 (1041-1047 vs 960-983) and 407x407x813 (1184-1211 vs 1126-1133). The dead lanes of the
// partial column (37 % of 645's two columns) and the x self copies cost more than the third fused step saves, so such a
// sub-domain keeps the pairs. Cut sub-domains (not measured; bench.py times whole-region triples against the
// overlapped pairs and picks) and ragged rows whose x comes from halos anyway (wrap_self off, x cut, rows the pairs
// cannot wrap) take the triples
bool StencilModel::triples_read_x_from_halos(int w) const {
  if (cfg_.temporal < 3 || !(w & 1) || !on_device()) return false;
  StencilTune tw = cfg_.tune, th = cfg_.tune;
  tw.wrap = w;
  th.wrap = w & ~1;
  bool withWrap = true, withHalo = true;
  for (const auto &d : dd_->domains())
    for (int64_t q = 0; q < d.num_data(); ++q) {
      const bool partialColumn = w == 7 && d.size().x % stencil7x3_column_cells(d.elem_size(q)) != 0;
      withWrap = withWrap && stencil7x3_supported(d, q, d.get_compute_region(), tw);
      withHalo = withHalo && stencil7x3_supported(d, q, d.get_compute_region(), th) && !partialColumn;
    }
  return !withWrap && withHalo;
}

// pairTune_ with the axes the fused pairs / triples wrap in-kernel (their self copies leave the exchange:
// prepare_skip_wrapped). Returns whether overlapped and whole-region pairs would wrap the same axes, so that they can
// be switched at run time: the local interior is shrunk only along axes cut across GPUs, which are never
// self-wrapped (set_overlap)
bool StencilModel::decide_pair_wrap() {
  pairTune_ = cfg_.tune;
  pairTune_.wrap = 0;
  if (!pairs_ || !cfg_.wrapSelf) return true;
  const auto &doms = dd_->domains();
  int w = dd_->self_wrap_axes() & cfg_.wrapAxesMask;
  for (const auto &d : doms)
    for (int64_t q = 0; q < d.num_data(); ++q) w &= stencil7x2_wrappable_axes(d, q, cfg_.tune.x2row);
  if (triples_read_x_from_halos(w)) w &= ~1;
  // the swept regions must span every wrapped axis (a forced full split cuts all of them)
  int wOn = w;
  for (size_t di = 0; di < doms.size() && !pairInteriors_.empty(); ++di)
    wOn &= spanned_axes(doms[di].get_compute_region(), pairInteriors_[di]);
  pairTune_.wrap = overlap_ ? wOn : w;
  if (pairTune_.wrap != 0) dd_->prepare_skip_wrapped(pairTune_.wrap);
  return wOn == w;
}

// overlapToggle_, pipeOk_, pipe3Ok_, the publication counter (pubCells_, pubCounter_), pipelined_
void StencilModel::decide_toggle_and_pipelining(const std::vector<Rect3> &li, bool sameWrap) {
  auto &doms = dd_->domains();
  if (pairs_ && sameWrap && !pairInteriors_.empty()) {
    bool ok = true;
    for (const auto &r : pairInteriors_) ok = ok && !r.empty();
    overlapToggle_ = has_remote_halo(li) && ok && on_device();
  }
  // pipelined pairs (overlap mode 3): one device, halos remote along z only (every boundary plane an exchange reads
  // is one of the first / last two z planes of the sweep), the whole-row kernel for every quantity, and a plan the
  // producer gate can start (fused co-located stores only; re-checked per pair since the co-located copy can change)
  if (!overlapToggle_ || doms.size() != 1) return;
  const Rect3 c = doms[0].get_compute_region();
  const bool geom = (spanned_axes(c, li[0]) & 3) == 3 && c.extent().z >= 4 * pubDepth_;
  bool ok = geom && dd_->gated_send_supported(pairTune_.wrap);
  for (int64_t q = 0; q < doms[0].num_data() && ok; ++q) ok = stencil7x2_row_kernel_used(doms[0], q, c, pairTune_);
  pipeOk_ = ok;
  // pipelined triples (mode 4) do not need the pairs' whole-row kernel, and their exchange may keep same-GPU
  // translate copies (triples that read x from halos: ragged rows, 1024-cell rows, fp64): a gated exchange runs those
  // behind the whole sweep, its co-located sends and receives on the published planes
  pipe3Ok_ = ok || (geom && cfg_.temporal >= 3 && dd_->gated_send_supported(pairTune_.wrap, true));
  if (!pipeOk_ && !pipe3Ok_) return;
  const Dim3 e = c.extent();
  pubCells_ = uint64_t(e.x) * uint64_t(e.y) * uint64_t(std::min<int64_t>(e.z, 2 * pubDepth_)) *
              uint64_t(doms[0].num_data());
  doms[0].set_device();
  HIP_CHECK(hipExtMallocWithFlags((void **)&pubCounter_, 256, hipDeviceMallocUncached));
  HIP_CHECK(hipMemset(pubCounter_, 0, 256));
  HIP_CHECK(hipDeviceSynchronize());
  if (pipeOk_ && cfg_.overlapMode == 3 && overlap_) pipelined_ = true;
}

// stepTune_, localSteps_ with stepInteriors_ / stepExteriors_, confinedSelf_; for single steps that overlap, overlap_
void StencilModel::plan_single_steps() {
  // single steps: the self-periodic axes are read in-kernel at their periodic image and their same-GPU copies leave
  // the exchange (a fully periodic sub-domain exchanges nothing; one MI355X at 512^3: the ~25 us copy-plan kernel of
  // a ~225 us step). Overlapped, as for the fused pairs: the same-GPU translate first, the interior shrunk only at
  // faces whose halo arrives from another GPU (get_local_interior) during the remote transfers, the slabs at those
  // faces after them, and the sweep leaves x2reserve CUs to the transports' kernels.
  const auto &doms = dd_->domains();
  stepTune_ = cfg_.tune;
  stepTune_.wrap = 0;
  localSteps_ = false;
  const bool wrapping = !pairs_ && !forward_ && on_device() && cfg_.wrapSelf && cfg_.tune.variant != StencilTune::kMfma;
  if (wrapping && overlap_ && cfg_.localInterior) {
    const auto li = dd_->get_local_interior(1);
    const bool remote = has_remote_halo(li);
    bool ok = true;
    for (const auto &r : li) ok = ok && !r.empty();
    if (remote && ok) {
      localSteps_ = true;
      stepInteriors_ = li;
      stepExteriors_.clear();
      for (size_t di = 0; di < doms.size(); ++di)
        stepExteriors_.push_back(shell_slabs(doms[di].get_compute_region(), li[di]));
      dd_->set_comm_max_blocks(cfg_.tune.x2reserve);
    } else if (!remote && cfg_.autoOverlap) {
      overlap_ = false; // every halo from this GPU: exchange -> whole-region step
    }
  }
  if (wrapping && (!overlap_ || localSteps_)) {
    int w = dd_->self_wrap_axes() & cfg_.wrapAxesMask;
    for (size_t di = 0; di < doms.size(); ++di) {
      const auto &d = doms[di];
      for (int64_t q = 0; q < d.num_data(); ++q) w &= stencil7_wrappable_axes(d, q);
      // the swept regions must span every wrapped axis
      if (localSteps_) w &= spanned_axes(d.get_compute_region(), stepInteriors_[di]);
    }
    stepTune_.wrap = w;
    if (w != 0) dd_->prepare_skip_wrapped(w);
  }
  // forced overlap of single steps whose every halo is a same-GPU copy (one GPU with --no-wrap: BASELINE config 4 as
  // the reference runs it, bin/astaroth_sim.cu:223-274): the copy-plan translate runs confined to x2reserve CUs on
  // the comm stream while the interior sweep leaves those CUs free, then the exterior slabs
  confinedSelf_ = !pairs_ && !forward_ && overlap_ && !localSteps_ && on_device() && cfg_.tune.x2reserve > 0 &&
                  only_same_gpu_copies();
  if (confinedSelf_) dd_->set_translate_max_blocks(cfg_.tune.x2reserve);
}

// triplesOk_, triples_
void StencilModel::decide_triples() {
  // fused triples: device sub-domains of whole 512-cell fp32 rows wrapped in-kernel, or of 512-cell fp32 / 256-cell
  // fp64 columns whose x halos come from the exchange, the last column whole or holding at most 509 / 253 cells
  // (stencil7x3_supported; rows ending 1 or 2 cells short of a column keep pairs); each other axis wraps in-kernel (its
  // self copies leave the exchange) or reads the 3-deep halos of a depth-3 exchange, one per three steps.
  // Whole regions only, so not beside an overlapped exchange (set_overlap switches between the two). The spheres at
  // least 3 cells from the periodic faces (the intermediate steps evaluate them at unwrapped halo coordinates)
  triplesOk_ = pairs_ && cfg_.temporal >= 3 && on_device();
  if (triplesOk_ && sph_.enabled) triplesOk_ = spheres_clear_of_faces(sph_, cfg_.size, 2, 3);
  for (const auto &d : dd_->domains())
    for (int64_t q = 0; triplesOk_ && q < d.num_data(); ++q)
      triplesOk_ = stencil7x3_supported(d, q, d.get_compute_region(), pairTune_);
  triples_ = triplesOk_ && !overlap_;
}

// the classic interior / exterior split, the compute streams, the initial condition, the forwarders
void StencilModel::start() {
  interiors_ = dd_->get_interior();
  exteriors_ = dd_->get_exterior();
  auto &doms = dd_->domains();
  for (size_t di = 0; di < doms.size(); ++di) {
    auto &d = doms[di];
    if (d.backend() == Backend::Device) {
      compute_.emplace_back(d.gpu(), Priority::DEFAULT);
      exteriorDone_.emplace_back(d.gpu());
    }
    hipStream_t s = compute_.empty() ? nullptr : compute_.back().get();
    for (int64_t q = 0; q < d.num_data(); ++q) {
      if (cfg_.kind == StencilKind::Jacobi)
        jacobi_init(d, q, d.get_compute_region(), s);
      else
        astaroth_init(d, q, cfg_.astarothPeriod, s);
    }
  }
  synchronize();
  for (size_t di = 0; di < doms.size(); ++di)
    if (!compute_.empty()) dd_->record_ready(di, compute_[di]);
  if (forward_) {
    // from now on the kernels keep the halos current; fill them once for the initial state
    dd_->exchange();
    fwd_.resize(doms.size());
    for (size_t di = 0; di < doms.size(); ++di) {
      const auto targets = dd_->forward_targets(di);
      for (int64_t q = 0; q < doms[di].num_data(); ++q)
        fwd_[di].emplace_back(new HaloForwarder(doms[di], q, targets));
      stepDone_.emplace_back(doms[di].gpu());
    }
    for (size_t di = 0; di < doms.size(); ++di) stepDone_[di].record(compute_[di]);
  }
}

// whatever `enqueue` puts on compute_[0], captured and instantiated; nothing runs
template <typename Enqueue> hipGraphExec_t StencilModel::capture(Enqueue &&enqueue) {
  hipStream_t s = compute_[0].get();
  hipGraph_t g = nullptr;
  hipGraphExec_t exec = nullptr;
  HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  enqueue();
  HIP_CHECK(hipStreamEndCapture(s, &g));
  HIP_CHECK(hipGraphInstantiate(&exec, g, nullptr, nullptr, 0));
  HIP_CHECK(hipGraphDestroy(g));
  return exec;
}

void StencilModel::advance(int k) {
  enqueue_step(k);
  dd_->swap();
  // the next exchange must follow this step's compute; in single-stream mode stream order already guarantees it
  const size_t n = dd_->domains().size();
  if (!compute_.empty() && (overlap_ || pipelined3_ || n != 1))
    for (size_t di = 0; di < n; ++di) dd_->record_ready(di, compute_[di]);
  steps_ += k;
}

void StencilModel::step() {
  TraceRange tr("StencilModel::step");
  if (!graphs_) return advance(1);
  const int p = dd_->domains()[0].parity();
  if (!graphExec_[p]) graphExec_[p] = capture([&] { enqueue_step(); });
  HIP_CHECK(hipGraphLaunch(graphExec_[p], compute_[0].get()));
  dd_->swap();
  ++steps_;
}

void StencilModel::run(int iters) {
  TraceRange tr("StencilModel::run");
  auto &doms = dd_->domains();
  if (graphs_ && iters > 0) { // a whole run recorded by prepare({iters})
    auto it = runGraph_.find({iters, doms[0].parity()});
    if (it != runGraph_.end()) {
      for (int k = 0; k < it->second.sweeps; ++k) dd_->swap();
      HIP_CHECK(hipGraphLaunch(it->second.exec, compute_[0].get()));
      steps_ += iters;
      return;
    }
  }
  const int per = steps_per_sweep(), gsteps = graph_steps();
  const int sweeps = gsteps / per; // sweeps per graph block (an even number: the block keeps the parity)
  while (graphs_ && iters >= gsteps) {
    const int p = doms[0].parity();
    if (!graphBlock_[p]) capture_block();
    for (int k = 0; k < sweeps; ++k) dd_->swap();
    HIP_CHECK(hipGraphLaunch(graphBlock_[p], compute_[0].get()));
    steps_ += gsteps;
    iters -= gsteps;
  }
  for (; triples_ && iters >= 3; iters -= 3) advance(3);
  for (; pairs_ && iters >= 2; iters -= 2) advance(2);
  for (int i = 0; i < iters; ++i) step();
}

void StencilModel::capture_block() {
  // records kGraphSteps steps starting at the current buffer parity into graphBlock_[parity]; nothing runs, and
  // the swaps done while recording are undone (an even number of sweeps returns to the same parity anyway)
  const int per = steps_per_sweep(), sweeps = graph_steps() / per;
  const int p = dd_->domains()[0].parity();
  graphBlock_[p] = capture([&] {
    for (int k = 0; k < sweeps; ++k) {
      enqueue_step(per);
      dd_->swap(); // pointers only; the captured kernels carry the buffers of each sweep
    }
  });
}

void StencilModel::capture_run(int n) {
  // the sweeps run(n) enqueues (graph blocks, then triples, pairs, single steps: the same kernels in the same order)
  // recorded as one graph; the swaps done while recording are undone
  const int p = dd_->domains()[0].parity();
  RunGraph rg;
  rg.exec = capture([&] {
    for (int left = n; left > 0;) {
      const int k = triples_ && left >= 3 ? 3 : (pairs_ && left >= 2 ? 2 : 1);
      enqueue_step(k);
      dd_->swap();
      ++rg.sweeps;
      left -= k;
    }
  });
  if (rg.sweeps % 2) dd_->swap();
  runGraph_[{n, p}] = rg;
}

void StencilModel::prepare(const std::vector<int> &runs) {
  // instantiate the graph blocks of both buffer parities up front, so the first run() of a timed loop does not pay
  // for stream capture + instantiation (the bench's warm-up may be shorter than one block)
  if (!graphs_) return;
  for (int i = 0; i < 2; ++i) {
    if (!graphBlock_[dd_->domains()[0].parity()]) capture_block();
    for (int n : runs) {
      STENCIL_REQUIRE(n > 0 && n <= 1024, "prepare: run length " << n << " outside [1, 1024]");
      if (!runGraph_.count({n, dd_->domains()[0].parity()})) capture_run(n);
    }
    dd_->swap();
  }
}

// k fused steps of every quantity of sub-domain di over `region`
void StencilModel::sweep(int k, size_t di, const Rect3 &region, hipStream_t s, const StencilTune &tune) {
  const LocalDomain &d = dd_->domains()[di];
  for (int64_t q = 0; q < d.num_data(); ++q) {
    if (k == 1) stencil7_apply(d, q, region, cfg_.kind, sph_, s, tune);
    if (k == 2) stencil7x2_apply(d, q, region, cfg_.kind, sph_, s, tune);
    if (k == 3)
      STENCIL_REQUIRE(stencil7x3_apply(d, q, region, cfg_.kind, sph_, s, tune),
                      "fused triple not supported for quantity " << q);
  }
}

// one exchange (of depth k), then k fused steps of every whole sub-domain. One device sub-domain: the exchange goes on
// the compute stream itself (no cross-stream hand-offs; with every halo read in-kernel at its periodic image it has
// nothing left to copy and only orders the step)
void StencilModel::whole_sweep(int k) {
  auto &doms = dd_->domains();
  const StencilTune &tune = k == 1 ? stepTune_ : pairTune_;
  const bool single = !compute_.empty() && doms.size() == 1;
  dd_->exchange_async(single ? compute_[0].get() : nullptr, tune.wrap);
  for (size_t di = 0; di < doms.size(); ++di) {
    hipStream_t s = compute_stream(di);
    if (!single) dd_->wait_exchange(di, s);
    sweep(k, di, doms[di].get_compute_region(), s, tune);
  }
}

// pipelined pairs (k = 2, mode 3) / triples (k = 3, mode 4): this sweep's exchange was gated on the previous sweep's
// boundary planes (it ran beside the rest of that sweep); the sweep waits for it, leaves x2reserve CUs to the next
// gated exchange and publishes its own first / last pubDepth_ z planes early for it. The triples' gated exchange may
// keep same-GPU translate copies (gated_send_supported(.., true))
void StencilModel::pipelined_sweep(int k, bool gateOk) {
  const bool gate = gateOk && dd_->gated_send_supported(pairTune_.wrap, k == 3);
  if (gate) dd_->set_send_gate(pubCounter_, pubTotal_);
  dd_->exchange_async(nullptr, pairTune_.wrap);
  dd_->wait_exchange(0, compute_[0]);
  StencilTune ti = pairTune_;
  ti.reserveCUs = cfg_.tune.x2reserve;
  const bool pub = dd_->gated_send_supported(pairTune_.wrap, k == 3);
  if (pub) {
    ti.publish = pubCounter_;
    ti.publishDepth = pubDepth_; // the exchange reads this many planes at each z face
    // fixed march directions: the lockstep schedule's outer z parts march away from the domain's z faces, so the
    // boundary planes the next exchange waits for come out at the start of every sweep; the per-pair flip
    // (alternateZ) would write them last on every other pair and leave that exchange nothing to overlap
    ti.alternateZ = false;
  }
  sweep(k, 0, dd_->domains()[0].get_compute_region(), compute_[0].get(), ti);
  if (pub) {
    pubTotal_ += pubCells_;
    lastPublished_ = true;
  }
}

// the slabs around the interior of an overlapped fused pair
void StencilModel::pair_slabs(size_t di, hipStream_t s) {
  const LocalDomain &d = dd_->domains()[di];
  for (int64_t q = 0; q < d.num_data(); ++q)
    stencil7x2_apply_exterior(d, q, pairInteriors_[di], cfg_.kind, sph_, s, pairTune_);
}

// the slabs around the interior of an overlapped single step
void StencilModel::step_slabs(size_t di, const std::vector<Rect3> &slabs, hipStream_t s, const StencilTune &tune) {
  const LocalDomain &d = dd_->domains()[di];
  for (int64_t q = 0; q < d.num_data(); ++q) stencil7_apply_regions(d, q, slabs, cfg_.kind, sph_, s, tune);
}

// The exterior slabs only need the halos, not the interior result: slabs(di, stream) runs them on the comm stream
// right behind the exchange, beside the interior sweep; the compute stream then joins the comm stream
template <typename Slabs> void StencilModel::slabs_on_comm_stream(Slabs &&slabs) {
  const bool device = !compute_.empty();
  for (size_t di = 0; di < dd_->domains().size(); ++di) {
    hipStream_t s = device ? dd_->comm_stream(di) : nullptr;
    slabs(di, s);
    if (device) {
      exteriorDone_[di].record(s);
      exteriorDone_[di].wait_on(compute_[di]);
    }
  }
}

void StencilModel::enqueue_step(int k) {
  auto &doms = dd_->domains();
  const bool gateOk = lastPublished_; // the previous sweep published: the next exchange may start on its planes
  lastPublished_ = false;
  if (k == 2 && pipelined_) return pipelined_sweep(2, gateOk);
  if (k == 2 && overlap_) {
    // temporal blocking, overlapped: interior S o S on the compute stream while the depth-2 exchange runs on the
    // comm stream, then the exterior slabs on the comm stream behind it; the compute stream joins them
    // the interior sweep leaves x2reserve CUs free, so the pack / flag / unpack kernels of the comm stream are
    // not queued behind a grid that holds every CU until it retires
    dd_->exchange_async(nullptr, pairTune_.wrap);
    StencilTune ti = pairTune_;
    ti.reserveCUs = cfg_.tune.x2reserve;
    for (size_t di = 0; di < doms.size(); ++di) {
      dd_->wait_translated(di, compute_[di]);
      sweep(2, di, pairInteriors_[di], compute_[di].get(), ti);
    }
    if (slabsAfter_) { // mode 2: the slabs follow the interior sweep on the compute stream, once the halos are in
      for (size_t di = 0; di < doms.size(); ++di) {
        dd_->wait_exchange(di, compute_[di]);
        pair_slabs(di, compute_[di].get());
      }
      return;
    }
    return slabs_on_comm_stream([&](size_t di, hipStream_t s) { pair_slabs(di, s); });
  }
  if (k == 3 && pipelined3_) return pipelined_sweep(3, gateOk);
  if (k == 2 || k == 3) return whole_sweep(k); // temporal blocking: one exchange per fused pair / triple
  if (forward_) {
    // step i of a sub-domain overwrites halos its neighbours read in step i-1 and reads halos they write in step
    // i-1: with several sub-domains every stream first joins the previous step of all the others
    const bool multi = doms.size() > 1;
    for (size_t di = 0; di < doms.size(); ++di) {
      hipStream_t s = compute_[di].get();
      if (multi)
        for (size_t dj = 0; dj < doms.size(); ++dj)
          if (dj != di) stepDone_[dj].wait_on(s);
      for (int64_t q = 0; q < doms[di].num_data(); ++q) {
        const HaloForwarder *f = fwd_[di][size_t(q)].get();
        stencil7_apply(doms[di], q, doms[di].get_compute_region(), cfg_.kind, sph_, s, cfg_.tune, f);
        f->forward_rest(doms[di].parity(), s);
      }
    }
    if (multi)
      for (size_t di = 0; di < doms.size(); ++di) stepDone_[di].record(compute_[di]);
    return;
  }
  if (localSteps_) {
    // single step, overlapped against the remote part of the exchange only (see plan_single_steps)
    dd_->exchange_async(nullptr, stepTune_.wrap);
    StencilTune ti = stepTune_;
    ti.reserveCUs = cfg_.tune.x2reserve;
    for (size_t di = 0; di < doms.size(); ++di) {
      dd_->wait_translated(di, compute_[di]);
      sweep(1, di, stepInteriors_[di], compute_[di].get(), ti);
    }
    return slabs_on_comm_stream([&](size_t di, hipStream_t s) { step_slabs(di, stepExteriors_[di], s, stepTune_); });
  }
  if (overlap_) {
    // exchange first: its pack/send kernels (high-priority comm stream) get CUs before the interior sweep fills them
    dd_->exchange_async();
    StencilTune ti = cfg_.tune;
    if (confinedSelf_) ti.reserveCUs = cfg_.tune.x2reserve;
    for (size_t di = 0; di < doms.size(); ++di) sweep(1, di, interiors_[di], compute_stream(di), ti);
    return slabs_on_comm_stream([&](size_t di, hipStream_t s) { step_slabs(di, exteriors_[di], s, cfg_.tune); });
  }
  whole_sweep(1);
}

void StencilModel::set_overlap(bool on) {
  STENCIL_REQUIRE(overlapToggle_, "set_overlap: this model's pairs cannot switch overlap (no remote halos, or the "
                                  "overlapped sweep would wrap other axes)");
  if (on == overlap_) return;
  synchronize();
  overlap_ = on;
  triples_ = triplesOk_ && !on; // whole-region sweeps: triples where supported
  dd_->set_comm_max_blocks(on ? cfg_.tune.x2reserve : 0);
  // the same-GPU translate stays confined only while an overlapped sweep leaves it those CUs
  dd_->set_translate_max_blocks(on && confinedSelf_ ? cfg_.tune.x2reserve : 0);
}

void StencilModel::set_overlap_mode(int mode) {
  STENCIL_REQUIRE(mode >= 0 && mode <= 4, "overlap mode " << mode);
  STENCIL_REQUIRE(mode != 3 || pipeOk_, "overlap mode 3 (pipelined pairs) is not possible for this model");
  STENCIL_REQUIRE(mode != 4 || can_pipeline_triples(), "overlap mode 4 (pipelined triples) is not possible for this model");
  if (mode == overlap_mode()) return;
  set_overlap(mode != 0 && mode != 4);
  slabsAfter_ = mode == 2;
  pipelined_ = mode == 3;
  pipelined3_ = mode == 4;
  // the gated exchanges of modes 3 / 4 run beside the sweep on the CUs it leaves free
  dd_->set_comm_max_blocks(mode != 0 ? cfg_.tune.x2reserve : 0);
}

void StencilModel::set_comm_reserve(int cus) {
  STENCIL_REQUIRE(cus >= 0 && cus <= 128, "comm reserve " << cus);
  if (cus == cfg_.tune.x2reserve) return;
  synchronize();
  cfg_.tune.x2reserve = cus;
  pairTune_.x2reserve = cus;
  stepTune_.x2reserve = cus;
  if (overlap_ || pipelined3_) dd_->set_comm_max_blocks(cus);
  if (confinedSelf_ && overlap_) dd_->set_translate_max_blocks(cus);
}

void StencilModel::set_triple_schedule(float sphw, int left, int parts) {
  STENCIL_REQUIRE(left >= 0 && left <= 3 && parts >= 0 && parts <= 8 && sphw >= 0, "triple schedule");
  synchronize();
  for (StencilTune *t : {&cfg_.tune, &pairTune_, &stepTune_}) {
    t->x3sphw = sphw;
    t->x3left = left;
    t->x3parts = parts;
  }
  HIP_CHECK(destroy_graphs()); // run() / prepare() record them again
}

hipError_t StencilModel::destroy_graphs() {
  hipError_t first = hipSuccess;
  auto destroy = [&](hipGraphExec_t &g) {
    if (!g) return;
    const hipError_t e = hipGraphExecDestroy(g);
    if (first == hipSuccess) first = e;
    g = nullptr;
  };
  for (auto &g : graphExec_) destroy(g);
  for (auto &g : graphBlock_) destroy(g);
  for (auto &kv : runGraph_) destroy(kv.second.exec);
  runGraph_.clear();
  return first;
}

void StencilModel::synchronize() {
  // the compute streams join the exchange (wait_exchange / exteriorDone_ / the exchange enqueued on them), so a
  // stalled peer stalls them too: DistributedDomain polls them with its watchdog instead of blocking on them first
  std::vector<hipStream_t> streams;
  for (auto &s : compute_) streams.push_back(s.get());
  if (dd_->realized())
    dd_->sync_streams(streams);
  else
    for (auto &s : compute_) s.sync();
}

} // namespace stencil
