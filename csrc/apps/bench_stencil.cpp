// Compute-kernel micro-benchmark: the 7-point Jacobi update on one MI355X against the HBM streaming roofline.
// No reference counterpart as an app (the reference only cites kernel times, bin/astaroth_sim.cu:130-152); this is
// the tuning harness behind the Jacobi3D numbers in BASELINE.md.
// Prints CSV `kernel,variant,ty,zc,us,gcells,eff_TBps` where eff_TBps counts the 8 B/cell minimum traffic.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "stencil/domain/distributed_domain.hpp"
#include "stencil/domain/local_domain.hpp"
#include "stencil/domain/packer.hpp"
#include "stencil/kernels/field_reduce.hpp"
#include "stencil/kernels/grid_transfer.hpp"
#include "stencil/kernels/stencil_ops.hpp"
#include "stencil/rt/argparse.hpp"
#include "stencil/rt/stream.hpp"

using namespace stencil;

// streaming roofline: dst = src over n float4, non-temporal stores, grid-stride
typedef float f4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void stream_copy(const f4 *__restrict__ src, f4 *__restrict__ dst, int64_t n) {
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) {
    f4 v = src[i];
    __builtin_nontemporal_store(v, dst + i);
  }
}
// U independent 16-B loads in flight per lane, contiguous block-sized tiles (each block owns a chunk)
template <int U>
__global__ __launch_bounds__(256) void stream_copy_tiles(const f4 *__restrict__ src, f4 *__restrict__ dst, int64_t n) {
  const int64_t per = (n + gridDim.x - 1) / gridDim.x;
  const int64_t beg = int64_t(blockIdx.x) * per, end = beg + per < n ? beg + per : n;
  for (int64_t i = beg + threadIdx.x; i < end; i += 256 * U) {
    f4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + u * 256 < end) v[u] = src[i + u * 256];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (i + u * 256 < end) __builtin_nontemporal_store(v[u], dst + i + u * 256);
  }
}
// read-only and write-only streams (the two halves of the roofline)
__global__ __launch_bounds__(256) void stream_read(const f4 *__restrict__ src, float *__restrict__ sink, int64_t n) {
  f4 acc = {0, 0, 0, 0};
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256) acc += src[i];
  if (acc.x == 1234.5f) sink[0] = acc.y + acc.z + acc.w;
}
__global__ __launch_bounds__(256) void stream_write(f4 *__restrict__ dst, int64_t n) {
  const f4 v = {1, 2, 3, 4};
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(gridDim.x) * 256)
    __builtin_nontemporal_store(v, dst + i);
}

int main(int argc, char **argv) {
  int64_t n = 512;
  int iters = 20, reps = 1;
  std::string only;
  ArgParser p("7-point stencil kernel sweep on one GPU");
  p.option(&n, "--n", "cube edge").option(&iters, "--iters", "timed launches per config")
      .option(&reps, "--reps", "repetitions of the whole sweep (interleaved)")
      .option(&only, "--only", "run only 'lds', 'reg', 'copy', 'star' (weighted stars of radius 1-3 beside stencil7), 'box' (27-point boxes beside "
                             "stencil7 and the radius-1 star; 'boxzc': their z-chunk sweep) or 'reduce' (field "
                             "reductions beside the single-step sweep) or 'bc' (boundary fill beside the periodic exchange) or "
                             "'axpby' (field algebra beside the field reductions) or 'transfer' (grid transfer n^3 <-> (n/2)^3 "
                             "beside the one-operand reduction and the one-source axpby) or 'varcoef' (the "
                             "variable-coefficient stencil beside the radius-1 star at n^3 and (n/2)^3, fp32 and fp64) or 'relax' (the "
                             "fused variable-coefficient residual / Jacobi sweep beside varcoef and varcoef + axpby)");
  if (!p.parse(argc, argv)) return p.need_help() ? 0 : 1;
  std::setvbuf(stdout, nullptr, _IOLBF, 0); // progress lines reach a redirected log as they are printed
  LocalDomain ld(Dim3(n, n, n), Dim3(0, 0, 0), 0, Backend::Device);
  ld.set_radius(1);
  ld.add_data<float>("d");
  ld.realize();
  Stream s(0);
  const Rect3 reg = ld.get_compute_region();
  const Spheres sph = Spheres::jacobi(reg);
  jacobi_init(ld, 0, ld.get_full_region(), s);
  s.sync();
  const double cells = double(n) * n * n;

  auto timeit = [&](auto &&fn) {
    for (int i = 0; i < 3; ++i) fn();
    Event a(0, true), b(0, true);
    a.record(s);
    for (int i = 0; i < iters; ++i) fn();
    b.record(s);
    b.sync();
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    return double(ms) * 1e3 / iters; // us
  };
  std::printf("kernel,variant,ty,zc,us,gcells,eff_TBps\n");
  if (only.empty() || only == "copy") {
    const int64_t nv = int64_t(n) * n * n / 4;
    for (int blocks : {1024, 2048, 4096, 8192}) {
      const double us = timeit([&] {
        hipLaunchKernelGGL(stream_copy, dim3(blocks), dim3(256), 0, s, (const f4 *)ld.curr_data(0),
                           (f4 *)ld.next_data(0), nv);
      });
      std::printf("copy,%d,0,0,%.2f,%.1f,%.3f\n", blocks, us, cells / us / 1e3, cells * 8 / us / 1e6);
    }
    for (int blocks : {512, 1024, 2048}) {
      const double us4 = timeit([&] {
        hipLaunchKernelGGL(stream_copy_tiles<4>, dim3(blocks), dim3(256), 0, s, (const f4 *)ld.curr_data(0),
                           (f4 *)ld.next_data(0), nv);
      });
      std::printf("copy_tiles4,%d,0,0,%.2f,%.1f,%.3f\n", blocks, us4, cells / us4 / 1e3, cells * 8 / us4 / 1e6);
      const double usr = timeit([&] {
        hipLaunchKernelGGL(stream_read, dim3(blocks), dim3(256), 0, s, (const f4 *)ld.curr_data(0),
                           (float *)ld.next_data(0), nv);
      });
      std::printf("read_only,%d,0,0,%.2f,%.1f,%.3f\n", blocks, usr, cells / usr / 1e3, cells * 4 / usr / 1e6);
      const double usw = timeit([&] {
        hipLaunchKernelGGL(stream_write, dim3(blocks), dim3(256), 0, s, (f4 *)ld.next_data(0), nv);
      });
      std::printf("write_only,%d,0,0,%.2f,%.1f,%.3f\n", blocks, usw, cells / usw / 1e3, cells * 4 / usw / 1e6);
    }
  }
  struct Cfg {
    int variant, ty, zc, nw = 8;
  };
  std::vector<Cfg> cfgs;
  if (only.empty() || only == "lds")
    for (int ty : {2, 4, 8})
      for (int zc : {0, 8, 16, 32, 64}) cfgs.push_back({0, ty, zc});
  if (only.empty() || only == "deep" || only == "lds")
    for (int pf : {2, 3})
      for (int nw : {4, 8, 16})
        for (int zc : {0, 32, 64}) cfgs.push_back({pf, 2, zc, nw});
  if (only.empty() || only == "reg")
    for (int ty : {4, 8})
      for (int zc : {0, 16, 32}) cfgs.push_back({1, ty, zc});
  for (int rep = 0; rep < reps; ++rep)
  if (only.empty() || only == "xchg") {
    // the Kernel-transport exchange of a single self-wrapping sub-domain (one copy-plan launch), all faces and per axis
    const char *names[] = {"xchg_all", "xchg_x", "xchg_y", "xchg_z"};
    for (int mode = 0; mode < 4; ++mode) {
      std::vector<CopySeg> segs;
      for (int ax = 0; ax < 3; ++ax) {
        if (mode != 0 && mode != ax + 1) continue;
        for (int sgn = -1; sgn <= 1; sgn += 2) {
          Dim3 d(0, 0, 0);
          (ax == 0 ? d.x : ax == 1 ? d.y : d.z) = sgn;
          build_translate_segs(ld, ld, d, true, segs);
        }
      }
      finalize_segs(segs);
      CopyPlan cp = make_copy_plan(segs, 0);
      const double us = timeit([&] { copy_plan_device(cp, s); });
      std::printf("%s,0,0,0,%.2f,%.1f,%.3f\n", names[mode], us, double(cp.bytes) / us / 1e3, 2.0 * cp.bytes / us / 1e6);
      free_copy_plan(cp);
    }
  }
  for (int rep = 0; rep < reps; ++rep)
  if (only.empty() || only == "fwd") {
    // halo forwarding onto itself (periodic self-wrap of a single sub-domain): all faces, then each axis alone
    // fwd_xself: x messages stored onto the sender's own output cells (same lines as the main store): separates
    // the instruction cost of the x path from the cost of its scattered halo lines
    const char *names[] = {"fwd_all", "fwd_x", "fwd_y", "fwd_z", "fwd_xself"};
    for (int mode = 0; mode < 5; ++mode)
    for (int zc : {0, 16, 32, 64}) {
      std::vector<ForwardTarget> tg;
      for (int ax = 0; ax < 3; ++ax) {
        if (mode != 0 && mode != ax + 1 && !(mode == 4 && ax == 0)) continue;
        for (int sgn = -1; sgn <= 1; sgn += 2) {
          Dim3 d(0, 0, 0), off(0, 0, 0);
          (ax == 0 ? d.x : ax == 1 ? d.y : d.z) = sgn;
          (ax == 0 ? off.x : ax == 1 ? off.y : off.z) = mode == 4 ? 0 : -sgn * n;
          tg.push_back(ForwardTarget{d, &ld, off});
        }
      }
      HaloForwarder hf(ld, 0, tg);
      StencilTune t;
      t.zchunk = zc;
      const double us = timeit([&] { stencil7_apply(ld, 0, reg, StencilKind::Jacobi, sph, s, t, &hf); });
      std::printf("%s,0,2,%d,%.2f,%.1f,%.3f\n", names[mode], zc, us, cells / us / 1e3, cells * 8 / us / 1e6);
    }
  }
  for (int rep = 0; rep < reps; ++rep)
  if (only.empty() || only == "mfma") {
    // the matrix-core line update (x pair on MFMA) against the VALU single step on the same domain
    for (int zc : {0, 16, 64}) {
      StencilTune t;
      t.variant = StencilTune::kMfma;
      t.zchunk = zc;
      const double us = timeit([&] { stencil7_apply(ld, 0, reg, StencilKind::Jacobi, sph, s, t); });
      std::printf("stencil7_mfma,%d,0,%d,%.2f,%.1f,%.3f\n", StencilTune::kMfma, zc, us, cells / us / 1e3,
                  cells * 8 / us / 1e6);
    }
  }
  if (only == "one") {
    // one launch of each default kernel (single step v2, fused pair, MFMA variant) for counter collection
    StencilTune t;
    timeit([&] { stencil7_apply(ld, 0, reg, StencilKind::Jacobi, sph, s, t); });
    StencilTune tm;
    tm.variant = StencilTune::kMfma;
    timeit([&] { stencil7_apply(ld, 0, reg, StencilKind::Jacobi, sph, s, tm); });
    LocalDomain l2(Dim3(n, n, n), Dim3(0, 0, 0), 0, Backend::Device);
    l2.set_radius(Radius::face_edge_corner(2, 1, 0));
    l2.add_data<float>("d");
    l2.realize();
    jacobi_init(l2, 0, l2.get_full_region(), s);
    timeit([&] { stencil7x2_apply(l2, 0, l2.get_compute_region(), StencilKind::Jacobi, sph, s, t); });
    return 0;
  }
  for (int rep = 0; rep < reps; ++rep)
  if (only == "ext") {
    // overlapped fused pair pieces on a depth-2 domain: whole sweep, interior sweep, exterior (thin-slab kernels)
    LocalDomain l2(Dim3(n, n, n), Dim3(0, 0, 0), 0, Backend::Device);
    l2.set_radius(Radius::face_edge_corner(2, 1, 0));
    l2.add_data<float>("d");
    l2.realize();
    jacobi_init(l2, 0, l2.get_full_region(), s);
    s.sync();
    const Rect3 c = l2.get_compute_region();
    for (int sx : {2, 4}) {
    const Rect3 in(c.lo + Dim3(sx, 2, 2), c.hi - Dim3(sx, 2, 2));
    std::printf("# interior shrink x=%d\n", sx);
    StencilTune t;
    const double whole = timeit([&] { stencil7x2_apply(l2, 0, c, StencilKind::Jacobi, sph, s, t); });
    const double inner = timeit([&] { stencil7x2_apply(l2, 0, in, StencilKind::Jacobi, sph, s, t); });
    const double outer = timeit([&] { stencil7x2_apply_exterior(l2, 0, in, StencilKind::Jacobi, sph, s, t); });
    Stream s2(0, Priority::HIGH);
    Event e(0);
    const double both = timeit([&] {
      e.record(s);
      e.wait_on(s2);
      stencil7x2_apply_exterior(l2, 0, in, StencilKind::Jacobi, sph, s2, t);
      stencil7x2_apply(l2, 0, in, StencilKind::Jacobi, sph, s, t);
      e.record(s2);
      e.wait_on(s);
    });
    std::printf("x2_whole,0,0,0,%.2f,0,0\nx2_interior,0,0,0,%.2f,0,0\nx2_exterior,0,0,0,%.2f,0,0\nx2_int+ext_concurrent,0,0,0,%.2f,0,0\n",
                whole, inner, outer, both);
    }
  }
  for (int rep = 0; rep < reps; ++rep)
  if (only == "ovl") {
    // Remote-halo overlap of a fused pair on ONE GPU, the off-GPU link emulated by host-pinned memory (PCIe, about
    // as slow as one xGMI link): the z faces are "packed" into a pinned buffer, "unpacked" from a device buffer,
    // then the z slabs are computed. seq = pack + unpack + whole sweep on one stream (no overlap); ovl = pack ->
    // unpack -> z slabs on a high-priority stream while the z-shrunk interior sweep runs (reserve r CUs).
    // (CU-masked streams were tried as well: no faster, and one masked configuration hung the run.)
    LocalDomain l2(Dim3(n, n, n), Dim3(0, 0, 0), 0, Backend::Device);
    l2.set_radius(Radius::face_edge_corner(2, 1, 0));
    l2.add_data<float>("d");
    l2.realize();
    jacobi_init(l2, 0, l2.get_full_region(), s);
    s.sync();
    const Rect3 c = l2.get_compute_region();
    const Rect3 in(c.lo + Dim3(0, 0, 2), c.hi - Dim3(0, 0, 2));
    const Dim3 pch = l2.pitch(0);
    const int64_t faceBytes = 2 * pch.x * pch.y * 4; // two planes
    char *hostBuf = nullptr, *devBuf = nullptr;
    HIP_CHECK(hipHostMalloc((void **)&hostBuf, 2 * faceBytes, hipHostMallocDefault));
    HIP_CHECK(hipMalloc((void **)&devBuf, 2 * faceBytes));
    std::vector<CopySeg> packSegs, unpackSegs;
    char *cur = static_cast<char *>(l2.curr_data(0));
    const int64_t zlo = l2.radius().z(-1), nz = l2.size().z;
    for (int k = 0; k < 2; ++k) {
      const int64_t zs = k == 0 ? zlo : zlo + nz - 2;  // interior planes sent
      const int64_t zh = k == 0 ? zlo + nz : zlo - 2;  // halo planes received (periodic self)
      const Dim3 ext(faceBytes / 4, 1, 1);
      packSegs.push_back(make_copy_seg(StridedBox{cur + zs * pch.x * pch.y * 4, 0, 0},
                                       StridedBox{hostBuf + k * faceBytes, 0, 0}, ext, 4));
      unpackSegs.push_back(make_copy_seg(StridedBox{devBuf + k * faceBytes, 0, 0},
                                         StridedBox{cur + zh * pch.x * pch.y * 4, 0, 0}, ext, 4));
    }
    finalize_segs(packSegs);
    finalize_segs(unpackSegs);
    CopyPlan pk = make_copy_plan(packSegs, 0), up = make_copy_plan(unpackSegs, 0);
    StencilTune t;
    Stream hi(0, Priority::HIGH);
    Event e(0), e2(0);
    const double sweep = timeit([&] { stencil7x2_apply(l2, 0, c, StencilKind::Jacobi, sph, s, t); });
    const double packOnly = timeit([&] { copy_plan_device(pk, s); });
    const double seq = timeit([&] {
      copy_plan_device(pk, s);
      copy_plan_device(up, s);
      stencil7x2_apply(l2, 0, c, StencilKind::Jacobi, sph, s, t);
    });
    std::printf("ovl_sweep,0,0,0,%.2f,0,0\novl_pack_pinned,0,0,0,%.2f,0,0\novl_seq,0,0,0,%.2f,0,0\n", sweep, packOnly, seq);
    const double ext = timeit([&] { stencil7x2_apply_exterior(l2, 0, in, StencilKind::Jacobi, sph, s, t); });
    std::printf("ovl_zslabs_alone,0,0,0,%.2f,0,0\n", ext);
    // extAfter: the slabs run on the compute stream after the interior sweep (whole GPU) instead of on the comm
    // stream behind the unpack (few CUs while the sweep holds the rest)
    auto overlapped = [&](hipStream_t cs, hipStream_t ms, int reserve, bool extAfter = false, int lim = 0) {
      StencilTune ti = t;
      ti.reserveCUs = reserve;
      return timeit([&] {
        e.record(s);
        e.wait_on(ms);
        e.wait_on(cs);
        copy_plan_device(pk, ms, lim);
        copy_plan_device(up, ms, lim);
        if (!extAfter) stencil7x2_apply_exterior(l2, 0, in, StencilKind::Jacobi, sph, ms, t);
        stencil7x2_apply(l2, 0, in, StencilKind::Jacobi, sph, cs, ti);
        e2.record(ms);
        e2.wait_on(extAfter ? cs : s);
        if (extAfter) stencil7x2_apply_exterior(l2, 0, in, StencilKind::Jacobi, sph, cs, t);
        e.record(cs);
        e.wait_on(s);
      });
    };
    for (int r : {0, 8, 16})
      std::printf("ovl_reserve%d,0,0,0,%.2f,0,0\n", r, overlapped(s, hi, r));
    for (int r : {0, 4, 8, 16})
      std::printf("ovl_extafter_reserve%d,0,0,0,%.2f,0,0\n", r, overlapped(s, hi, r, true));
    // comm kernels confined to `lim` CUs (copy_plan_device maxBlocks) beside a sweep that leaves `r` CUs free
    for (int lim : {4, 8, 16})
      for (int r : {4, 8, 16}) {
        if (r < lim) continue;
        std::printf("ovl_lim%d_reserve%d,0,0,0,%.2f,0,0\n", lim, r, overlapped(s, hi, r, true, lim));
        std::printf("ovl_lim%d_reserve%d_extcomm,0,0,0,%.2f,0,0\n", lim, r, overlapped(s, hi, r, false, lim));
      }
    {
      const double p8 = timeit([&] { copy_plan_device(pk, s, 8); });
      std::printf("ovl_pack_pinned_lim8,0,0,0,%.2f,0,0\n", p8);
    }
    {
      StencilTune tc = t;
      tc.x2sched = 0; // fixed z-chunks (several rounds of blocks) instead of balanced segments
      const double ch = timeit([&] {
        e.record(s);
        e.wait_on(hi);
        copy_plan_device(pk, hi);
        copy_plan_device(up, hi);
        stencil7x2_apply(l2, 0, in, StencilKind::Jacobi, sph, s, tc);
        e2.record(hi);
        e2.wait_on(s);
        stencil7x2_apply_exterior(l2, 0, in, StencilKind::Jacobi, sph, s, t);
      });
      std::printf("ovl_extafter_chunks,0,0,0,%.2f,0,0\n", ch);
    }
    free_copy_plan(pk);
    free_copy_plan(up);
    HIP_CHECK(hipHostFree(hostBuf));
    HIP_CHECK(hipFree(devBuf));
  }
  if (only == "star" || only == "starzc") {
    // weighted stars of radius 1, 2, 3 (fp32) on a depth-3 domain, interleaved per repetition with the default
    // 7-point single step (variant 2) on the radius-1 domain: both read the field once and write it once
    LocalDomain l3(Dim3(n, n, n), Dim3(0, 0, 0), 0, Backend::Device);
    l3.set_radius(Radius::face_edge_corner(3, 0, 0));
    l3.add_data<float>("d");
    l3.realize();
    jacobi_init(l3, 0, l3.get_full_region(), s);
    s.sync();
    const Rect3 reg3 = l3.get_compute_region();
    for (int rep = 0; rep < reps && only == "starzc"; ++rep)
      for (int r = 1; r <= 3; ++r) // the z-chunk length (blocks per launch) around the automatic choice
        for (int zc : {0, 32, 43, 52, 64, 86, 128}) {
          StencilTune t;
          t.zchunk = zc;
          StarWeights w;
          w.radius = r;
          w.center = 0.25;
          for (int ax = 0; ax < 3; ++ax)
            for (int sd = 0; sd < 2; ++sd)
              for (int k = 0; k < r; ++k) w.w[ax][sd][k] = 0.125 / r;
          const StarLaunchInfo li = stencil_star_launch_info(l3, 0, reg3, w, t);
          const double us = timeit([&] { stencil_star_apply(l3, 0, reg3, w, s, t); });
          std::printf("stencil_star,%d,2,%d,%.2f,%.1f,%.3f,blocks%lld\n", r, li.zchunk, us, cells / us / 1e3,
                      cells * 8 / us / 1e6, (long long)li.blocks);
        }
    for (int rep = 0; rep < reps && only == "star"; ++rep) {
      StencilTune t;
      const double us7 = timeit([&] { stencil7_apply(ld, 0, reg, StencilKind::Jacobi, sph, s, t); });
      std::printf("stencil7,%d,%d,%d,%.2f,%.1f,%.3f,nw%d\n", t.variant, t.ty, t.zchunk, us7, cells / us7 / 1e3,
                  cells * 8 / us7 / 1e6, t.nw);
      for (int r = 1; r <= 3; ++r) {
        StarWeights w; // identity + a sixth of the 2nd-order Laplacian spread over the radius (values do not matter)
        w.radius = r;
        w.center = 0.25;
        for (int ax = 0; ax < 3; ++ax)
          for (int sd = 0; sd < 2; ++sd)
            for (int k = 0; k < r; ++k) w.w[ax][sd][k] = 0.125 / r;
        const StarLaunchInfo li = stencil_star_launch_info(l3, 0, reg3, w, t);
        const double us = timeit([&] { stencil_star_apply(l3, 0, reg3, w, s, t); });
        std::printf("stencil_star,%d,2,%d,%.2f,%.1f,%.3f,path%d\n", r, li.zchunk, us, cells / us / 1e3,
                    cells * 8 / us / 1e6, li.path);
      }
    }
  }
  if (only == "box" || only == "boxzc") {
    // weighted 27-point boxes (fp32 and fp64) on radius-(1, 1, 1) domains, interleaved per repetition with the default
    // 7-point single step (variant 2) on the radius-1 domain and the radius-1 star on the box's domain: all read the
    // field once and write it once. The one-thread-per-cell box kernel runs on an unpadded twin of each domain.
    auto box_domain = [&](bool f64, bool pad) {
      auto l = std::make_unique<LocalDomain>(Dim3(n, n, n), Dim3(0, 0, 0), 0, Backend::Device);
      l->set_radius(Radius::face_edge_corner(1, 1, 1));
      l->set_padding(pad);
      if (f64)
        l->add_data<double>("d");
      else
        l->add_data<float>("d");
      l->realize();
      fill_value(*l, 0, 0.5, true, s);
      s.sync();
      return l;
    };
    BoxWeights bw; // the binomial filter (values do not matter)
    for (int k = 0; k < 3; ++k)
      for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) bw.w[k][j][i] = double(1 << ((k == 1) + (j == 1) + (i == 1))) / 64.0;
    StarWeights sw;
    sw.radius = 1;
    sw.center = 0.25;
    for (int ax = 0; ax < 3; ++ax)
      for (int sd = 0; sd < 2; ++sd) sw.w[ax][sd][0] = 0.125;
    for (int f64 = 0; f64 < 2; ++f64) {
      const double bytes = f64 ? 16 : 8;
      const char *ty = f64 ? "fp64" : "fp32";
      {
        auto lb = box_domain(f64 != 0, true);
        const Rect3 regb = lb->get_compute_region();
        for (int rep = 0; rep < reps && only == "boxzc"; ++rep)
          for (int zc : {0, 32, 43, 52, 64, 86, 128}) { // the z-chunk length (blocks per launch) around the automatic choice
            StencilTune t;
            t.zchunk = zc;
            const BoxLaunchInfo li = stencil_box_launch_info(*lb, 0, regb, bw, t);
            const double us = timeit([&] { stencil_box_apply(*lb, 0, regb, bw, s, t); });
            std::printf("stencil_box,%s,2,%d,%.2f,%.1f,%.3f,blocks%lld\n", ty, li.zchunk, us, cells / us / 1e3,
                        cells * bytes / us / 1e6, (long long)li.blocks);
          }
        for (int rep = 0; rep < reps && only == "box"; ++rep) {
          StencilTune t;
          if (!f64) {
            const double us7 = timeit([&] { stencil7_apply(ld, 0, reg, StencilKind::Jacobi, sph, s, t); });
            std::printf("stencil7,%d,%d,%d,%.2f,%.1f,%.3f,nw%d\n", t.variant, t.ty, t.zchunk, us7, cells / us7 / 1e3,
                        cells * 8 / us7 / 1e6, t.nw);
          }
          const StarLaunchInfo si = stencil_star_launch_info(*lb, 0, regb, sw, t);
          const double uss = timeit([&] { stencil_star_apply(*lb, 0, regb, sw, s, t); });
          std::printf("stencil_star,%s,2,%d,%.2f,%.1f,%.3f,path%d\n", ty, si.zchunk, uss, cells / uss / 1e3,
                      cells * bytes / uss / 1e6, si.path);
          const BoxLaunchInfo li = stencil_box_launch_info(*lb, 0, regb, bw, t);
          const double us = timeit([&] { stencil_box_apply(*lb, 0, regb, bw, s, t); });
          std::printf("stencil_box,%s,2,%d,%.2f,%.1f,%.3f,path%d\n", ty, li.zchunk, us, cells / us / 1e3,
                      cells * bytes / us / 1e6, li.path);
        }
      }
      if (only == "box") {
        auto lg = box_domain(f64 != 0, false);
        const Rect3 regg = lg->get_compute_region();
        for (int rep = 0; rep < reps; ++rep) {
          StencilTune t;
          const BoxLaunchInfo li = stencil_box_launch_info(*lg, 0, regg, bw, t);
          const double us = timeit([&] { stencil_box_apply(*lg, 0, regg, bw, s, t); });
          std::printf("stencil_box_unpadded,%s,2,%d,%.2f,%.1f,%.3f,path%d\n", ty, li.zchunk, us, cells / us / 1e3,
                      cells * bytes / us / 1e6, li.path);
        }
      }
    }
  }
  if (only == "varcoef") {
    // the variable-coefficient stencil (u and kappa read, next(u) written: three fields) beside the radius-1 star (two
    // fields) on the same domain, interleaved per repetition, at n^3 and (n / 2)^3, fp32 and fp64. The variant column
    // holds the element type and the cube edge; eff_TBps counts three fields for varcoef, two for the star.
    StarWeights sw;
    sw.radius = 1;
    sw.center = 0.25;
    for (int ax = 0; ax < 3; ++ax)
      for (int sd = 0; sd < 2; ++sd) sw.w[ax][sd][0] = 0.125;
    VarCoefWeights vw; // an explicit diffusion step (values do not matter)
    vw.shift = 1.0;
    vw.h[0] = 0.02;
    vw.h[1] = 0.03;
    vw.h[2] = 0.025;
    for (int64_t m : {n, n / 2})
      for (int f64 = 0; f64 < 2; ++f64) {
        const double es = f64 ? 8 : 4, mcells = double(m) * m * m;
        LocalDomain lv(Dim3(m, m, m), Dim3(0, 0, 0), 0, Backend::Device);
        lv.set_radius(Radius::face_edge_corner(1, 0, 0));
        if (f64) {
          lv.add_data<double>("u");
          lv.add_data<double>("kappa");
        } else {
          lv.add_data<float>("u");
          lv.add_data<float>("kappa");
        }
        lv.realize();
        fill_value(lv, 0, 0.5, true, s);
        fill_value(lv, 1, 1.5, true, s);
        s.sync();
        const Rect3 regv = lv.get_compute_region();
        char tag[32];
        std::snprintf(tag, sizeof tag, "%s_%lld", f64 ? "fp64" : "fp32", (long long)m);
        for (int rep = 0; rep < reps; ++rep) {
          StencilTune t;
          const StarLaunchInfo si = stencil_star_launch_info(lv, 0, regv, sw, t);
          const double uss = timeit([&] { stencil_star_apply(lv, 0, regv, sw, s, t); });
          std::printf("stencil_star,%s,2,%d,%.2f,%.1f,%.3f,path%d\n", tag, si.zchunk, uss, mcells / uss / 1e3,
                      mcells * 2 * es / uss / 1e6, si.path);
          const VarCoefLaunchInfo vi = stencil_varcoef_launch_info(lv, 0, 1, regv, vw, t);
          const double usv = timeit([&] { stencil_varcoef_apply(lv, 0, 1, regv, vw, s, t); });
          std::printf("stencil_varcoef,%s,2,%d,%.2f,%.1f,%.3f,path%d\n", tag, vi.zchunk, usv, mcells / usv / 1e3,
                      mcells * 3 * es / usv / 1e6, vi.path);
        }
      }
  }
  if (only == "relax") {
    // The fused residual / Jacobi sweep of the variable-coefficient operator beside what it replaces, on one domain
    // with the quantities u, kappa, f, r, interleaved per repetition, fp32 and fp64 at n^3: (a) stencil_varcoef_apply
    // (three fields), (b) stencil_varcoef_apply then field_axpby r = f - next(u), the unfused residual (six fields), (c)
    // relax in Residual mode into r and (d) in Jacobi mode into next(u) (four fields each). eff_TBps counts those fields.
    VarCoefWeights vw; // 1 - div(kappa grad), kappa = 1.5: the diagonal is 10
    vw.shift = 1.0;
    vw.h[0] = vw.h[1] = vw.h[2] = -0.5;
    for (int f64 = 0; f64 < 2; ++f64) {
      const double es = f64 ? 8 : 4;
      LocalDomain lv(Dim3(n, n, n), Dim3(0, 0, 0), 0, Backend::Device);
      lv.set_radius(Radius::face_edge_corner(1, 0, 0));
      for (const char *name : {"u", "kappa", "f", "r"}) {
        if (f64)
          lv.add_data<double>(name);
        else
          lv.add_data<float>(name);
      }
      lv.realize();
      fill_value(lv, 0, 0.5, true, s);
      fill_value(lv, 1, 1.5, true, s);
      fill_value(lv, 2, 0.25, true, s);
      s.sync();
      const Rect3 regv = lv.get_compute_region();
      char tag[32];
      std::snprintf(tag, sizeof tag, "%s_%lld", f64 ? "fp64" : "fp32", (long long)n);
      for (int rep = 0; rep < reps; ++rep) {
        StencilTune t;
        const VarCoefLaunchInfo vi = stencil_varcoef_launch_info(lv, 0, 1, regv, vw, t);
        const VarCoefRelaxLaunchInfo ri =
            stencil_varcoef_relax_launch_info(lv, 0, 1, 2, 3, true, regv, vw, VarCoefRelaxMode::Residual, t);
        const double usa = timeit([&] { stencil_varcoef_apply(lv, 0, 1, regv, vw, s, t); });
        const double usp = timeit([&] {
          stencil_varcoef_apply(lv, 0, 1, regv, vw, s, t);
          field_axpby_enqueue(lv, FieldRef(3, true), 1.0, FieldRef(2, true), -1.0, FieldRef(0, false), regv, s);
        });
        const double usr = timeit(
            [&] { stencil_varcoef_relax(lv, 0, 1, 2, 3, true, regv, vw, VarCoefRelaxMode::Residual, 1.0, s, t); });
        const double usj = timeit([&] {
          stencil_varcoef_relax(lv, 0, 1, 2, 0, false, regv, vw, VarCoefRelaxMode::Jacobi, 6.0 / 7.0, s, t);
        });
        std::printf("stencil_varcoef,%s,2,%d,%.2f,%.1f,%.3f,path%d\n", tag, vi.zchunk, usa, cells / usa / 1e3,
                    cells * 3 * es / usa / 1e6, vi.path);
        std::printf("varcoef_then_axpby,%s,2,%d,%.2f,%.1f,%.3f,path%d\n", tag, vi.zchunk, usp, cells / usp / 1e3,
                    cells * 6 * es / usp / 1e6, vi.path);
        std::printf("varcoef_relax_residual,%s,2,%d,%.2f,%.1f,%.3f,path%d\n", tag, ri.zchunk, usr, cells / usr / 1e3,
                    cells * 4 * es / usr / 1e6, ri.path);
        std::printf("varcoef_relax_jacobi,%s,2,%d,%.2f,%.1f,%.3f,path%d\n", tag, ri.zchunk, usj, cells / usj / 1e3,
                    cells * 4 * es / usj / 1e6, ri.path);
        std::printf("relax_ratios,%s,residual_over_pair,%.3f,jacobi_over_apply,%.3f\n", tag, usr / usp, usj / usa);
      }
    }
  }
  if (only == "bc") {
    // Boundary fill beside the periodic exchange of the same domain (fp32, face radius 3, one GPU): (a) the exchange
    // with every axis a same-GPU self copy (Kernel method), (b) apply_boundary with all six faces Mirror, (c) with
    // AntiMirror; both move the face cells (a) moves. Interleaved per round in one process, each call timed on its own,
    // blocking; medians over reps x iters calls, and `stream_us`, the mean of iters back-to-back launches between two
    // events. Then (b) with non-temporal row stores, and a star step (exchange, fill, star_apply, swap) periodic
    // against all-Mirror at radius 1 and 3.
    auto make_dd = [&](int r, const FaceCondition *fc) {
      auto dd = std::make_unique<DistributedDomain>(n, n, n);
      dd->set_radius(Radius::face_edge_corner(r, 0, 0));
      dd->set_methods(MethodFlags::Kernel);
      dd->set_gpus({0});
      dd->add_data<float>("u");
      if (fc) {
        BoundaryConditions bc;
        for (int a = 0; a < 3; ++a) bc.set_axis(a, *fc, *fc);
        dd->set_boundary_conditions(bc);
      }
      dd->realize();
      jacobi_init(dd->domains()[0], 0, dd->domains()[0].get_full_region(), s);
      s.sync();
      return dd;
    };
    const FaceCondition mir = FaceCondition::mirror(), anti = FaceCondition::antimirror(0.5);
    auto ddP = make_dd(3, nullptr), ddM = make_dd(3, &mir), ddA = make_dd(3, &anti);
    auto blocking_us = [&](auto &&fn, std::vector<double> &out) {
      const auto t0 = std::chrono::steady_clock::now();
      fn();
      HIP_CHECK(hipStreamSynchronize(s));
      out.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    };
    auto median = [](std::vector<double> v) {
      std::sort(v.begin(), v.end());
      return v.empty() ? 0.0 : (v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]));
    };
    auto xchg = [&] { ddP->exchange_async(s); };
    auto fillM = [&] { ddM->apply_boundary(s); };
    auto fillA = [&] { ddA->apply_boundary(s); };
    for (int i = 0; i < 3; ++i) { // warm-up: first launches, table upload
      xchg();
      fillM();
      fillA();
    }
    s.sync();
    std::vector<double> ux, um, ua, unt;
    for (int rep = 0; rep < std::max(reps, 1); ++rep)
      for (int i = 0; i < iters; ++i) {
        blocking_us(xchg, ux);
        blocking_us(fillM, um);
        blocking_us(fillA, ua);
        set_boundary_fill_nontemporal(true);
        blocking_us(fillM, unt);
        set_boundary_fill_nontemporal(false);
      }
    const double mx = median(ux), mm = median(um), ma = median(ua), mnt = median(unt);
    const double sx = timeit(xchg), sm = timeit(fillM), sa = timeit(fillA);
    set_boundary_fill_nontemporal(true);
    const double snt = timeit(fillM);
    set_boundary_fill_nontemporal(false);
    std::vector<FillRequest> rq(1);
    rq[0].bc = ddM->boundary_conditions(0);
    const FillLaunchInfo li = boundary_fill_launch_info(ddM->domains()[0], ddM->size(), rq);
    const double ghostBytes = 4.0 * (double(n + 6) * (n + 6) * (n + 6) - double(n) * n * n);
    std::printf("kernel,n,path,blocks,median_us,stream_us,ghost_MB\n");
    std::printf("exchange_periodic,%lld,-,-,%.2f,%.2f,%.2f\n", (long long)n, mx, sx,
                double(ddP->exchange_bytes_for_method(MethodFlags::All)) / 1e6);
    std::printf("fill_mirror,%lld,%d,%lld,%.2f,%.2f,%.2f\n", (long long)n, li.path, (long long)li.blocks, mm, sm, ghostBytes / 1e6);
    std::printf("fill_antimirror,%lld,%d,%lld,%.2f,%.2f,%.2f\n", (long long)n, li.path, (long long)li.blocks, ma, sa, ghostBytes / 1e6);
    std::printf("fill_mirror_nontemporal,%lld,%d,%lld,%.2f,%.2f,%.2f\n", (long long)n, li.path, (long long)li.blocks, mnt, snt,
                ghostBytes / 1e6);
    const bool met = mm <= 1.5 * mx && ma <= 1.5 * mx && sm <= 1.5 * sx && sa <= 1.5 * sx;
    std::printf("bc_condition,fill_le_1.5x_exchange,median %.2f %.2f vs %.2f,stream %.2f %.2f vs %.2f,%s\n", mm, ma, 1.5 * mx, sm,
                sa, 1.5 * sx, met ? "met" : "MISSED");
    ddA.reset();
    // a star step, periodic against all-Mirror
    std::printf("kernel,radius,boundary,step_us\n");
    for (int r : {1, 3}) {
      StarWeights w;
      w.radius = r;
      w.center = 0.25;
      for (int ax = 0; ax < 3; ++ax)
        for (int sd = 0; sd < 2; ++sd)
          for (int k = 0; k < r; ++k) w.w[ax][sd][k] = 0.125 / r;
      auto dp = r == 3 ? std::move(ddP) : make_dd(r, nullptr);
      auto dm = r == 3 ? std::move(ddM) : make_dd(r, &mir);
      StencilTune t;
      for (int which = 0; which < 2; ++which) {
        DistributedDomain &dd = which ? *dm : *dp;
        const double us = timeit([&] {
          dd.exchange_async(s);
          if (which) dd.apply_boundary(s);
          stencil_star_apply(dd.domains()[0], 0, dd.domains()[0].get_compute_region(), w, s, t);
          dd.swap();
        });
        std::printf("star_step,%d,%s,%.2f\n", r, which ? "mirror" : "periodic", us);
      }
    }
  }
  if (only == "reduce") {
    // Field reductions beside the default single-step sweep (stencil7_apply, default tune), all on the same field in
    // one invocation. Every call is timed on its own, blocking (launch, then wait for the stream: a reduction's
    // result is only of use on the host), interleaved sweep / one operand / two operands per round; the medians over
    // reps x iters calls are compared: the one-operand reduction reads half the bytes the sweep moves and must not
    // take longer than it. `stream_us` is the mean of iters back-to-back launches between two events.
    ReduceScratch scratch;
    StencilTune t;
    auto blocking_us = [&](auto &&fn, std::vector<double> &out) {
      const auto t0 = std::chrono::steady_clock::now();
      fn();
      HIP_CHECK(hipStreamSynchronize(s));
      out.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    };
    auto median = [](std::vector<double> v) {
      std::sort(v.begin(), v.end());
      return v.empty() ? 0.0 : (v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]));
    };
    auto sweep = [&] { stencil7_apply(ld, 0, reg, StencilKind::Jacobi, sph, s, t); };
    auto red1 = [&] { field_reduce_enqueue(ld, 0, true, -1, false, reg, scratch, s); };
    auto red2 = [&] { field_reduce_enqueue(ld, 0, true, 0, false, reg, scratch, s); };
    const ReduceLaunchInfo li = field_reduce_launch_info(ld, 0, true, 0, false, reg);
    for (int i = 0; i < 3; ++i) { // warm-up: first launches, scratch allocation
      sweep();
      red1();
      red2();
    }
    s.sync();
    std::vector<double> us7, us1, us2;
    for (int rep = 0; rep < std::max(reps, 1); ++rep)
      for (int i = 0; i < iters; ++i) {
        blocking_us(sweep, us7);
        blocking_us(red1, us1);
        blocking_us(red2, us2);
      }
    const double m7 = median(us7), m1 = median(us1), m2 = median(us2);
    const double s7 = timeit(sweep), s1 = timeit(red1), s2 = timeit(red2);
    std::printf("kernel,operands,path,blocks,median_us,gcells,read_TBps,stream_us\n");
    std::printf("stencil7,%d,%d,0,%.2f,%.1f,%.3f,%.2f\n", t.variant, t.ty, m7, cells / m7 / 1e3, cells * 4 / m7 / 1e6, s7);
    std::printf("field_reduce,1,%d,%lld,%.2f,%.1f,%.3f,%.2f\n", li.path, (long long)li.blocks, m1, cells / m1 / 1e3,
                cells * 4 / m1 / 1e6, s1);
    std::printf("field_reduce,2,%d,%lld,%.2f,%.1f,%.3f,%.2f\n", li.path, (long long)li.blocks, m2, cells / m2 / 1e3,
                cells * 8 / m2 / 1e6, s2);
    const FieldStats r = scratch.result();
    std::printf("reduce_check,count,%lld,nonfinite,%lld,sum_sq,%.17g\n", (long long)r.count, (long long)r.nonfinite, r.sum_sq);
    std::printf("reduce_condition,one_operand_median_us,%.2f,sweep_median_us,%.2f,%s\n", m1, m7, m1 <= m7 ? "met" : "MISSED");
  }
  if (only == "axpby") {
    // Field algebra beside the field reductions, on a domain of its own with three quantities r, p, w, all in one
    // invocation, every call timed as under 'reduce' (blocking medians, interleaved per round, and back-to-back stream
    // time). The CG residual update r <- r - alpha next(p) with stats reads 8 B and writes 4 B per cell; the
    // one-operand and the two-operand reduction (unchanged code) together move the same 12 B per cell, so the fused
    // update must take at most 1.25 x the sum of their medians.
    LocalDomain ad(Dim3(n, n, n), Dim3(0, 0, 0), 0, Backend::Device);
    ad.set_radius(1);
    for (const char *name : {"r", "p", "w"}) ad.add_data<float>(name);
    ad.realize();
    const Rect3 areg = ad.get_compute_region();
    for (int q = 0; q < 3; ++q) {
      jacobi_init(ad, q, ad.get_full_region(), s);
      field_axpby_enqueue(ad, FieldRef(q, false), 1.0, FieldRef(q, true), 0.0, FieldRef(), areg, s);
    }
    s.sync();
    ReduceScratch scratch;
    auto blocking_us = [&](auto &&fn, std::vector<double> &out) {
      const auto t0 = std::chrono::steady_clock::now();
      fn();
      HIP_CHECK(hipStreamSynchronize(s));
      out.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    };
    auto median = [](std::vector<double> v) {
      std::sort(v.begin(), v.end());
      return v.empty() ? 0.0 : (v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]));
    };
    const FieldRef r(0, true), ap(1, false), w(2, true), none;
    const double alpha = 1e-4;
    std::vector<std::function<void()>> fns = {
        [&] { field_reduce_enqueue(ad, 0, true, -1, false, areg, scratch, s); },
        [&] { field_reduce_enqueue(ad, 0, true, 1, false, areg, scratch, s); },
        [&] { field_axpby_enqueue(ad, w, 0.5, r, 0.0, none, areg, s); },                          // w <- 0.5 r
        [&] { field_axpby_enqueue(ad, w, 1.0, r, 0.5, w, areg, s); },                             // w <- r + 0.5 w
        [&] { field_axpby_enqueue(ad, r, 1.0, r, -alpha, ap, areg, s, &scratch); },               // r <- r - alpha Ap, ||r||
        [&] { field_axpby_enqueue(ad, r, 1.0, r, -alpha, ap, areg, s, &scratch, 0, true); },      // the same, nt stores
    };
    const char *names[] = {"field_reduce,1", "field_reduce,2", "field_axpby,1", "field_axpby,2", "field_axpby_stats,2",
                           "field_axpby_stats_nt,2"};
    const double bytes[] = {4, 8, 8, 12, 12, 12};
    const ReduceLaunchInfo rli = field_reduce_launch_info(ad, 0, true, 1, false, areg);
    const AxpbyLaunchInfo ali[] = {field_axpby_launch_info(ad, w, 0.5, r, 0.0, none, areg),
                                   field_axpby_launch_info(ad, w, 1.0, r, 0.5, w, areg),
                                   field_axpby_launch_info(ad, r, 1.0, r, -alpha, ap, areg, true),
                                   field_axpby_launch_info(ad, r, 1.0, r, -alpha, ap, areg, true, 0, true)};
    for (int i = 0; i < 3; ++i) // warm-up: first launches, scratch allocation
      for (auto &f : fns) f();
    s.sync();
    std::vector<std::vector<double>> us(fns.size());
    for (int rep = 0; rep < std::max(reps, 1); ++rep)
      for (int i = 0; i < iters; ++i)
        for (size_t k = 0; k < fns.size(); ++k) blocking_us(fns[k], us[k]);
    std::printf("kernel,operands,path,blocks,median_us,gcells,moved_TBps,stream_us\n");
    std::vector<double> med(fns.size());
    for (size_t k = 0; k < fns.size(); ++k) {
      med[k] = median(us[k]);
      const double st = timeit(fns[k]);
      const int path = k < 2 ? rli.path : ali[k - 2].path;
      const long long blocks = (long long)(k < 2 ? rli.blocks : ali[k - 2].blocks);
      std::printf("%s,%d,%lld,%.2f,%.1f,%.3f,%.2f\n", names[k], path, blocks, med[k], cells / med[k] / 1e3,
                  cells * bytes[k] / med[k] / 1e6, st);
    }
    const FieldStats fs = scratch.result();
    std::printf("axpby_check,count,%lld,nonfinite,%lld,sum_sq,%.17g\n", (long long)fs.count, (long long)fs.nonfinite, fs.sum_sq);
    const double bound = 1.25 * (med[0] + med[1]);
    std::printf("axpby_condition,fused_update_median_us,%.2f,reduce1_plus_reduce2_median_us,%.2f,ratio,%.3f,bound,1.25,%s\n",
                med[4], med[0] + med[1], med[4] / (med[0] + med[1]), med[4] <= bound ? "met" : "MISSED");
    std::printf("axpby_stores,plain_median_us,%.2f,nontemporal_median_us,%.2f\n", med[4], med[5]);
  }
  if (only == "transfer") {
    // Grid transfer between n^3 and (n/2)^3 in fp32 and fp64 beside two unchanged yardsticks on the fine grid, all
    // in one invocation and timed as under 'axpby' (blocking medians, interleaved per round, and back-to-back stream
    // time). Restriction reads every fine cell once and writes 1/8 as many coarse cells (9/8 of the bytes the
    // one-operand reduction reads); the correction u <- u + P e reads and writes every fine cell once and reads the
    // coarse grid (17/16 of the bytes of the one-source axpby). Each must take at most 1.25 x its yardstick's median
    // scaled by those bytes.
    auto blocking_us = [&](auto &&fn, std::vector<double> &out) {
      const auto t0 = std::chrono::steady_clock::now();
      fn();
      HIP_CHECK(hipStreamSynchronize(s));
      out.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    };
    auto median = [](std::vector<double> v) {
      std::sort(v.begin(), v.end());
      return v.empty() ? 0.0 : (v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]));
    };
    std::printf("kernel,dtype,path,blocks,median_us,fine_gcells,moved_TBps,stream_us\n");
    auto run = [&](auto tag, const char *tname) {
      using T = decltype(tag);
      const double es = sizeof(T);
      LocalDomain fd(Dim3(n, n, n), Dim3(0, 0, 0), 0, Backend::Device), cd(Dim3(n / 2, n / 2, n / 2), Dim3(0, 0, 0), 0, Backend::Device);
      fd.set_radius(Radius::face_edge_corner(1, 1, 1));
      cd.set_radius(Radius::face_edge_corner(1, 1, 1));
      for (const char *name : {"u", "r", "w"}) fd.add_data<T>(name);
      for (const char *name : {"u", "f"}) cd.add_data<T>(name);
      fd.realize();
      cd.realize();
      const Rect3 freg = fd.get_compute_region(), creg = cd.get_compute_region();
      for (int q = 0; q < 3; ++q) fill_value(fd, q, 0.25 + q, true, s);
      for (int q = 0; q < 2; ++q) fill_value(cd, q, 1e-3 * (q + 1), true, s);
      s.sync();
      ReduceScratch scratch;
      const FieldRef u(0, true), r(1, true), w(2, true), cu(0, true), cf(1, true), none;
      std::vector<std::function<void()>> fns = {
          [&] { field_reduce_enqueue(fd, 1, true, -1, false, freg, scratch, s); },   // the yardstick of restriction
          [&] { grid_restrict_enqueue(fd, r, cd, cf, creg, s); },                    // f_c <- R r
          [&] { field_axpby_enqueue(fd, w, 0.5, r, 0.0, none, freg, s); },           // the yardstick of the correction
          [&] { grid_prolong_enqueue(cd, cu, fd, u, u, freg, s); },                  // u <- u + P e
          [&] { grid_prolong_enqueue(cd, cu, fd, w, none, freg, s); },               // w <- P e
          [&] { grid_prolong_enqueue(cd, cu, fd, u, u, freg, s, 4); },               // u <- u + P e, shorter marches
          [&] { grid_prolong_enqueue(cd, cu, fd, u, u, freg, s, 16); },              // ... and longer ones
      };
      const char *names[] = {"field_reduce_1", "grid_restrict", "field_axpby_1", "grid_prolong_add", "grid_prolong",
                             "grid_prolong_add_zc4", "grid_prolong_add_zc16"};
      const double bytes[] = {es, es * 9 / 8, 2 * es, es * 17 / 8, es * 9 / 8, es * 17 / 8, es * 17 / 8};
      const ReduceLaunchInfo rli = field_reduce_launch_info(fd, 1, true, -1, false, freg);
      const AxpbyLaunchInfo ali = field_axpby_launch_info(fd, w, 0.5, r, 0.0, none, freg);
      const TransferLaunchInfo tli[] = {grid_restrict_launch_info(fd, r, cd, cf, creg),
                                        grid_prolong_launch_info(cd, cu, fd, u, u, freg),
                                        grid_prolong_launch_info(cd, cu, fd, w, none, freg),
                                        grid_prolong_launch_info(cd, cu, fd, u, u, freg, 4),
                                        grid_prolong_launch_info(cd, cu, fd, u, u, freg, 16)};
      const int paths[] = {rli.path, tli[0].path, ali.path, tli[1].path, tli[2].path, tli[3].path, tli[4].path};
      const long long blocks[] = {(long long)rli.blocks,    (long long)tli[0].blocks, (long long)ali.blocks, (long long)tli[1].blocks,
                                  (long long)tli[2].blocks, (long long)tli[3].blocks, (long long)tli[4].blocks};
      for (int i = 0; i < 3; ++i) // warm-up: first launches, scratch allocation
        for (auto &f : fns) f();
      s.sync();
      std::vector<std::vector<double>> us(fns.size());
      for (int rep = 0; rep < std::max(reps, 1); ++rep)
        for (int i = 0; i < iters; ++i)
          for (size_t k = 0; k < fns.size(); ++k) blocking_us(fns[k], us[k]);
      std::vector<double> med(fns.size());
      for (size_t k = 0; k < fns.size(); ++k) {
        med[k] = median(us[k]);
        const double st = timeit(fns[k]);
        std::printf("%s,%s,%d,%lld,%.2f,%.1f,%.3f,%.2f\n", names[k], tname, paths[k], blocks[k], med[k],
                    cells / med[k] / 1e3, cells * bytes[k] / med[k] / 1e6, st);
      }
      const double rb = 1.25 * 9 / 8 * med[0], pb = 1.25 * 17 / 16 * med[2];
      std::printf("transfer_condition,%s,restrict_median_us,%.2f,reduce1_median_us,%.2f,ratio,%.3f,bound,%.4f,%s\n", tname,
                  med[1], med[0], med[1] / med[0], 1.25 * 9 / 8, med[1] <= rb ? "met" : "MISSED");
      std::printf("transfer_condition,%s,prolong_add_median_us,%.2f,axpby1_median_us,%.2f,ratio,%.3f,bound,%.4f,%s\n", tname,
                  med[3], med[2], med[3] / med[2], 1.25 * 17 / 16, med[3] <= pb ? "met" : "MISSED");
    };
    run(float(), "fp32");
    run(double(), "fp64");
  }
  for (int rep = 0; rep < reps; ++rep)
  if (only == "x2pp") {
    // the fused pair as the model runs it: ping-pong (swap after every launch), so every launch reads what the
    // previous one wrote; non-temporal stores and the alternating z-march on/off
    LocalDomain l2(Dim3(n, n, n), Dim3(0, 0, 0), 0, Backend::Device);
    l2.set_radius(Radius::face_edge_corner(2, 1, 0));
    l2.add_data<float>("d");
    l2.realize();
    const Rect3 reg2 = l2.get_compute_region();
    jacobi_init(l2, 0, l2.get_full_region(), s);
    fill_value(l2, 0, 0.5, false, s);
    s.sync();
    for (int zc : {-1, 0, 64, 128}) { // -1: fixed auto z-chunks (x2sched 0); 0: balanced segments
      const int nt = 1, alt = 1;
      StencilTune t;
      t.nontemporal = nt;
      t.alternateZ = alt;
      t.zchunk = zc < 0 ? 0 : zc;
      t.x2sched = zc < 0 ? 0 : 1;
      const double us = timeit([&] {
        stencil7x2_apply(l2, 0, reg2, StencilKind::Jacobi, sph, s, t);
        l2.swap();
      }) / 2;
      std::printf("x2pp_nt%d_alt%d,1,1,%d,%.2f,%.1f,%.3f,nw12\n", nt, alt, zc, us, cells / us / 1e3,
                  cells * 8 / us / 1e6);
    }
  }
  for (int rep = 0; rep < reps; ++rep)
  if (only.empty() || only == "x2") {
    // two fused steps per sweep (temporal blocking) on a depth-2 domain; reported per STEP (two steps per launch)
    LocalDomain l2(Dim3(n, n, n), Dim3(0, 0, 0), 0, Backend::Device);
    l2.set_radius(Radius::face_edge_corner(2, 1, 0));
    l2.add_data<float>("d");
    l2.realize();
    const Rect3 reg2 = l2.get_compute_region();
    jacobi_init(l2, 0, l2.get_full_region(), s);
    s.sync();
    for (int zc : {0, 43, 64, 128}) {
      StencilTune t;
      t.zchunk = zc;
      const double us = timeit([&] { stencil7x2_apply(l2, 0, reg2, StencilKind::Jacobi, sph, s, t); }) / 2;
      std::printf("stencil7x2,1,1,%d,%.2f,%.1f,%.3f,nw12\n", zc, us, cells / us / 1e3, cells * 8 / us / 1e6);
    }
  }
  for (int rep = 0; rep < reps; ++rep)
  for (const Cfg &c : cfgs) {
    StencilTune t;
    t.variant = c.variant;
    t.ty = c.ty;
    t.zchunk = c.zc;
    t.nw = c.nw;
    const double us = timeit([&] { stencil7_apply(ld, 0, reg, StencilKind::Jacobi, sph, s, t); });
    std::printf("stencil7,%d,%d,%d,%.2f,%.1f,%.3f,nw%d\n", c.variant, c.ty, c.zc, us, cells / us / 1e3,
                cells * 8 / us / 1e6, c.nw);
  }
  return 0;
}
