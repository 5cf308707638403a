// Residual and damped-Jacobi sweep of the variable-coefficient operator for gfx950, one pass over u, kappa and f. See
// stencil/kernels/stencil_ops.hpp (stencil_varcoef_relax).
//   acc as stencil_varcoef_apply; dg = shift; for axis x, y, z, low face then high face:
//     ks = k(c) + k(n) (the sum acc uses); g = h[axis] * ks; dg = dg - g
//   r = f(c) - acc
//   Residual: dst(c) = r          Jacobi: q = r / dg; s = omega * q; dst(c) = u(c) + s
// Every sum, difference, product and quotient is its own rounding, in exactly that order, in the fast kernel, the
// generic kernel and the host loop alike, so all three are bitwise equal to stencil2_amd.ops.varcoef_relax_reference.
#include <hip/hip_runtime.h>

#include "stencil_varcoef_march.hpp"
#include "stencil/rt/hip_check.hpp"

// no FMA contraction anywhere below, device or host (hipcc contracts by default)
#pragma clang fp contract(off)

namespace stencil {

// one thread per cell: every layout the fast path refuses
template <typename T, int MODE> __global__ __launch_bounds__(256) void stencil_varcoef_relax_generic_kernel(VarCoefRelaxArgs<T> a) {
  const int64_t nx = a.hix - a.lox, ny = a.hiy - a.loy, nz = a.hiz - a.loz;
  const int64_t total = nx * ny * nz;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int x = a.lox + int(i % nx), y = a.loy + int((i / nx) % ny), z = a.loz + int(i / (nx * ny));
    const int64_t o = int64_t(z) * a.pxy + int64_t(y) * a.px + x;
    a.dst[o] = varcoef_relax_cell<T, MODE>(a.vw, a.omega, a.src + o, a.coef + o, a.rhs + o, a.px, a.pxy);
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
template <typename T, int MODE> static void varcoef_relax_host(const VarCoefRelaxArgs<T> &a) {
  for (int z = a.loz; z < a.hiz; ++z)
    for (int y = a.loy; y < a.hiy; ++y)
      for (int x = a.lox; x < a.hix; ++x) {
        const int64_t o = int64_t(z) * a.pxy + int64_t(y) * a.px + x;
        a.dst[o] = varcoef_relax_cell<T, MODE>(a.vw, a.omega, a.src + o, a.coef + o, a.rhs + o, a.px, a.pxy);
      }
}

// the quantities and the mode of one call
struct RelaxCall {
  int64_t qu, qk, qf, qdst;
  bool dstCurr;
  VarCoefRelaxMode mode;
  double omega;
};

// The z-march of stencil_varcoef_march.hpp bounded for two waves per SIMD, i.e. one block per CU: the right-hand
// side's rows and the carried diagonal need about 20 registers more than the 128 the operator fills, and without
// spills (144 to 166 VGPRs) one block per CU ran faster than two with scratch traffic.
template <typename T, int MODE> static const void *relax_kernel(bool nt) {
  return nt ? (const void *)stencil_varcoef_kernel<T, kVarTY, kVarNW, true, MODE, 2>
            : (const void *)stencil_varcoef_kernel<T, kVarTY, kVarNW, false, MODE, 2>;
}

template <typename T>
static VarCoefRelaxArgs<T> varcoef_relax_plan(const LocalDomain &dom, const RelaxCall &c, const Rect3 &region,
                                              const VarCoefWeights &wts, const StencilTune &tune,
                                              VarCoefRelaxLaunchInfo *info) {
  const void *kern = c.mode == VarCoefRelaxMode::Jacobi ? relax_kernel<T, kVarJacobi>(tune.nontemporal)
                                                        : relax_kernel<T, kVarResidual>(tune.nontemporal);
  T *dst = static_cast<T *>(c.dstCurr ? dom.curr_data(c.qdst) : dom.next_data(c.qdst));
  VarCoefRelaxArgs<T> a{};
  static_cast<VarCoefArgs<T> &>(a) =
      varcoef_plan<T>(dom, c.qu, c.qk, dst, {c.qf, c.qdst}, region, wts, tune, kern, info);
  a.rhs = static_cast<const T *>(dom.curr_data(c.qf));
  a.omega = T(c.omega);
  return a;
}

template <typename T, int MODE>
static void varcoef_relax_launch(const VarCoefRelaxArgs<T> &a, const VarCoefRelaxLaunchInfo &info, hipStream_t stream,
                                 bool nt) {
  if (info.path == 2) {
    void *params[] = {const_cast<VarCoefRelaxArgs<T> *>(&a)};
    HIP_CHECK(hipLaunchKernel(relax_kernel<T, MODE>(nt), dim3(uint32_t(info.blocks)), dim3(64, kVarNW),
                              params, 0, stream));
  } else {
    const int64_t total = int64_t(a.hix - a.lox) * (a.hiy - a.loy) * (a.hiz - a.loz);
    const int blocks = int(std::min<int64_t>((total + 255) / 256, 4096));
    hipLaunchKernelGGL((stencil_varcoef_relax_generic_kernel<T, MODE>), dim3(blocks), dim3(256), 0, stream, a);
  }
  HIP_CHECK(hipGetLastError());
}

template <typename T>
static void varcoef_relax_t(const LocalDomain &dom, const RelaxCall &c, const Rect3 &region, const VarCoefWeights &wts,
                            hipStream_t stream, const StencilTune &tune) {
  VarCoefRelaxLaunchInfo info;
  const VarCoefRelaxArgs<T> a = varcoef_relax_plan<T>(dom, c, region, wts, tune, &info);
  const bool jacobi = c.mode == VarCoefRelaxMode::Jacobi;
  if (info.path == 0) {
    if (jacobi)
      varcoef_relax_host<T, kVarJacobi>(a);
    else
      varcoef_relax_host<T, kVarResidual>(a);
    return;
  }
  dom.set_device();
  if (jacobi)
    varcoef_relax_launch<T, kVarJacobi>(a, info, stream, tune.nontemporal);
  else
    varcoef_relax_launch<T, kVarResidual>(a, info, stream, tune.nontemporal);
}

bool stencil_varcoef_relax_supported(const LocalDomain &dom, int64_t qu, int64_t qk, int64_t qf, int64_t qdst) {
  bool f64[4] = {false, false, false, false};
  const int64_t q[4] = {qu, qk, qf, qdst};
  if (!dom.realized()) return false;
  for (int i = 0; i < 4; ++i)
    if (!varcoef_fp(dom, q[i], &f64[i]) || !varcoef_same_layout(dom, qu, q[i])) return false;
  return varcoef_radii_ok(dom);
}

// the refusals shared by relax and launch_info; false: nothing to do (empty region)
static bool varcoef_relax_check(const LocalDomain &dom, const RelaxCall &c, const Rect3 &region, const StencilTune &tune,
                                bool *f64) {
  STENCIL_REQUIRE(dom.realized(), "variable-coefficient stencils need a realized domain");
  const int64_t q[4] = {c.qu, c.qk, c.qf, c.qdst};
  const char *names[4] = {"u", "kappa", "f", "dst"};
  for (int i = 0; i < 4; ++i) {
    bool f = false;
    STENCIL_REQUIRE(varcoef_fp(dom, q[i], i == 0 ? f64 : &f),
                    "variable-coefficient relax takes fp32 / fp64 quantities (" << names[i] << " " << q[i] << ")");
    STENCIL_REQUIRE(varcoef_same_layout(dom, c.qu, q[i]),
                    "variable-coefficient relax: u and " << names[i] << " differ in element size or row pitch ("
                        << dom.elem_size(c.qu) << " B, pitch " << dom.pitch(c.qu) << " vs " << dom.elem_size(q[i])
                        << " B, pitch " << dom.pitch(q[i]) << ")");
  }
  // the neighbours of u and kappa are read by other lanes than the one that stores a cell
  STENCIL_REQUIRE(!(c.dstCurr && (c.qdst == c.qu || c.qdst == c.qk)),
                  "variable-coefficient relax cannot write curr(u) or curr(kappa) in place (dst " << c.qdst << ")");
  STENCIL_REQUIRE(varcoef_radii_ok(dom), "variable-coefficient stencil needs face radii >= 1");
  STENCIL_REQUIRE(tune.wrap == 0, "variable-coefficient stencils read halos (no in-kernel wrap)");
  require_region_in_compute(dom, region);
  return !region.empty();
}

void stencil_varcoef_relax(const LocalDomain &dom, int64_t qu, int64_t qk, int64_t qf, int64_t qdst, bool dstCurr,
                           const Rect3 &region, const VarCoefWeights &w, VarCoefRelaxMode mode, double omega,
                           hipStream_t stream, const StencilTune &tune) {
  const RelaxCall c{qu, qk, qf, qdst, dstCurr, mode, omega};
  bool f64 = false;
  if (!varcoef_relax_check(dom, c, region, tune, &f64)) return;
  if (!f64)
    varcoef_relax_t<float>(dom, c, region, w, stream, tune);
  else
    varcoef_relax_t<double>(dom, c, region, w, stream, tune);
}

VarCoefRelaxLaunchInfo stencil_varcoef_relax_launch_info(const LocalDomain &dom, int64_t qu, int64_t qk, int64_t qf,
                                                         int64_t qdst, bool dstCurr, const Rect3 &region,
                                                         const VarCoefWeights &w, VarCoefRelaxMode mode,
                                                         const StencilTune &tune) {
  const RelaxCall c{qu, qk, qf, qdst, dstCurr, mode, 1.0};
  VarCoefRelaxLaunchInfo info;
  bool f64 = false;
  if (!varcoef_relax_check(dom, c, region, tune, &f64)) {
    info.path = -1;
    return info;
  }
  if (!f64)
    varcoef_relax_plan<float>(dom, c, region, w, tune, &info);
  else
    varcoef_relax_plan<double>(dom, c, region, w, tune, &info);
  return info;
}

} // namespace stencil
