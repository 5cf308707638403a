// Variable-coefficient diffusion stencil for gfx950. See stencil/kernels/stencil_ops.hpp (VarCoefWeights).
//   acc = shift * u(c); for axis a in x, y, z:
//     km = k(c) + k(c - e_a); dm = u(c - e_a) - u(c); fm = km * dm; tm = h[a] * fm; acc = acc + tm
//     kp = k(c) + k(c + e_a); dp = u(c + e_a) - u(c); fp = kp * dp; tp = h[a] * fp; acc = acc + tp
//   next(u)(c) = acc
// Every sum, difference and product is its own rounding, in exactly that order, in the fast kernel, the generic kernel
// and the host loop alike, so all three are bitwise equal to stencil2_amd.ops.varcoef_step_reference.
#include <hip/hip_runtime.h>

#include "stencil_varcoef_march.hpp"
#include "stencil/rt/hip_check.hpp"

// no FMA contraction anywhere below, device or host (hipcc contracts by default)
#pragma clang fp contract(off)

namespace stencil {

// The operator alone is the z-march of stencil_varcoef_march.hpp in its default mode: four waves per SIMD (two blocks
// per CU, as the LDS allows) mean 128 VGPRs, with fp32 free of scratch and fp64 at two spilled registers.

// one thread per cell: every layout the fast path refuses
template <typename T> __global__ __launch_bounds__(256) void stencil_varcoef_generic_kernel(VarCoefArgs<T> a) {
  const int64_t nx = a.hix - a.lox, ny = a.hiy - a.loy, nz = a.hiz - a.loz;
  const int64_t total = nx * ny * nz;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int x = a.lox + int(i % nx), y = a.loy + int((i / nx) % ny), z = a.loz + int(i / (nx * ny));
    const int64_t o = int64_t(z) * a.pxy + int64_t(y) * a.px + x;
    a.dst[o] = varcoef_cell<T>(a.vw, a.src + o, a.coef + o, a.px, a.pxy);
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
template <typename T> static void varcoef_host(const VarCoefArgs<T> &a) {
  for (int z = a.loz; z < a.hiz; ++z)
    for (int y = a.loy; y < a.hiy; ++y)
      for (int x = a.lox; x < a.hix; ++x) {
        const int64_t o = int64_t(z) * a.pxy + int64_t(y) * a.px + x;
        a.dst[o] = varcoef_cell<T>(a.vw, a.src + o, a.coef + o, a.px, a.pxy);
      }
}

// kernel arguments and the path apply takes for them
template <typename T>
static VarCoefArgs<T> varcoef_apply_plan(const LocalDomain &dom, int64_t qu, int64_t qk, const Rect3 &region,
                                   const VarCoefWeights &wts, const StencilTune &tune, VarCoefLaunchInfo *info) {
  const void *kern = tune.nontemporal ? (const void *)stencil_varcoef_kernel<T, kVarTY, kVarNW, true>
                                      : (const void *)stencil_varcoef_kernel<T, kVarTY, kVarNW, false>;
  return varcoef_plan<T>(dom, qu, qk, static_cast<T *>(dom.next_data(qu)), {}, region, wts, tune, kern, info);
}

template <typename T>
static void varcoef_apply_t(const LocalDomain &dom, int64_t qu, int64_t qk, const Rect3 &region,
                            const VarCoefWeights &wts, hipStream_t stream, const StencilTune &tune) {
  VarCoefLaunchInfo info;
  const VarCoefArgs<T> a = varcoef_apply_plan<T>(dom, qu, qk, region, wts, tune, &info);
  if (info.path == 0) {
    varcoef_host<T>(a);
    return;
  }
  dom.set_device();
  if (info.path == 2) {
    const dim3 block(64, kVarNW);
    if (tune.nontemporal)
      hipLaunchKernelGGL((stencil_varcoef_kernel<T, kVarTY, kVarNW, true>), dim3(uint32_t(info.blocks)), block, 0, stream, a);
    else
      hipLaunchKernelGGL((stencil_varcoef_kernel<T, kVarTY, kVarNW, false>), dim3(uint32_t(info.blocks)), block, 0, stream, a);
  } else {
    const int64_t total = int64_t(a.hix - a.lox) * (a.hiy - a.loy) * (a.hiz - a.loz);
    const int blocks = int(std::min<int64_t>((total + 255) / 256, 4096));
    hipLaunchKernelGGL((stencil_varcoef_generic_kernel<T>), dim3(blocks), dim3(256), 0, stream, a);
  }
  HIP_CHECK(hipGetLastError());
}

bool stencil_varcoef_supported(const LocalDomain &dom, int64_t qu, int64_t qk) {
  bool fu = false, fk = false;
  if (!dom.realized() || !varcoef_fp(dom, qu, &fu) || !varcoef_fp(dom, qk, &fk)) return false;
  return varcoef_same_layout(dom, qu, qk) && varcoef_radii_ok(dom);
}

// the refusals shared by apply and launch_info; false: nothing to do (empty region)
static bool varcoef_check(const LocalDomain &dom, int64_t qu, int64_t qk, const Rect3 &region, const StencilTune &tune,
                          bool *f64) {
  bool fk = false;
  STENCIL_REQUIRE(dom.realized(), "variable-coefficient stencils need a realized domain");
  STENCIL_REQUIRE(varcoef_fp(dom, qu, f64) && varcoef_fp(dom, qk, &fk),
                  "variable-coefficient stencils take fp32 / fp64 quantities (u " << qu << ", kappa " << qk << ")");
  STENCIL_REQUIRE(varcoef_same_layout(dom, qu, qk),
                  "variable-coefficient stencil: u and kappa differ in element size or row pitch (" << dom.elem_size(qu)
                      << " B, pitch " << dom.pitch(qu) << " vs " << dom.elem_size(qk) << " B, pitch " << dom.pitch(qk) << ")");
  STENCIL_REQUIRE(varcoef_radii_ok(dom), "variable-coefficient stencil needs face radii >= 1");
  STENCIL_REQUIRE(tune.wrap == 0, "variable-coefficient stencils read halos (no in-kernel wrap)");
  require_region_in_compute(dom, region);
  return !region.empty();
}

void stencil_varcoef_apply(const LocalDomain &dom, int64_t qu, int64_t qk, const Rect3 &region, const VarCoefWeights &w,
                           hipStream_t stream, const StencilTune &tune) {
  bool f64 = false;
  if (!varcoef_check(dom, qu, qk, region, tune, &f64)) return;
  if (!f64)
    varcoef_apply_t<float>(dom, qu, qk, region, w, stream, tune);
  else
    varcoef_apply_t<double>(dom, qu, qk, region, w, stream, tune);
}

VarCoefLaunchInfo stencil_varcoef_launch_info(const LocalDomain &dom, int64_t qu, int64_t qk, const Rect3 &region,
                                              const VarCoefWeights &w, const StencilTune &tune) {
  VarCoefLaunchInfo info;
  bool f64 = false;
  if (!varcoef_check(dom, qu, qk, region, tune, &f64)) {
    info.path = -1;
    return info;
  }
  if (!f64)
    varcoef_apply_plan<float>(dom, qu, qk, region, w, tune, &info);
  else
    varcoef_apply_plan<double>(dom, qu, qk, region, w, tune, &info);
  return info;
}

} // namespace stencil
