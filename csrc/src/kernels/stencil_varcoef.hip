// Variable-coefficient diffusion stencil for gfx950. See stencil/kernels/stencil_ops.hpp (VarCoefWeights).
//   acc = shift * u(c); for axis a in x, y, z:
//     km = k(c) + k(c - e_a); dm = u(c - e_a) - u(c); fm = km * dm; tm = h[a] * fm; acc = acc + tm
//     kp = k(c) + k(c + e_a); dp = u(c + e_a) - u(c); fp = kp * dp; tp = h[a] * fp; acc = acc + tp
//   next(u)(c) = acc
// Every sum, difference and product is its own rounding, in exactly that order, in the fast kernel, the generic kernel
// and the host loop alike, so all three are bitwise equal to stencil2_amd.ops.varcoef_step_reference.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "stencil_common.hpp"
#include "stencil/kernels/stencil_ops.hpp"
#include "stencil/rt/hip_check.hpp"

// no FMA contraction anywhere below, device or host (hipcc contracts by default)
#pragma clang fp contract(off)

namespace stencil {

// the weights in the element type (converted once on the host), passed by value in the kernel arguments
template <typename T> struct VarCoefW {
  T shift;
  T h[3];
};

template <typename T> struct VarCoefArgs {
  const T *src;  // raw [0,0,0] of curr(u)
  const T *coef; // raw [0,0,0] of curr(kappa): the pitches of u
  T *dst;        // raw [0,0,0] of next(u)
  int64_t px, pxy;
  int lox, loy, loz, hix, hiy, hiz; // region, raw coordinates
  int x0;                           // raw x of chunk 0 (16-B aligned in memory)
  int nchunks;                      // chunks covering [x0, hix)
  int rawYm1, rawZm1;               // clamps of the row / plane prefetches
  int zc;                           // planes per block
  int gx, gy, gz;                   // logical grid
  int remap;                        // XCD-aware block remap
  int flip;                         // reverse every block's z-march direction
  VarCoefW<T> vw;
};

// one face: h * ((k(c) + k(n)) * (u(n) - u(c))), three roundings after the two of the operands
template <typename T> __host__ __device__ __forceinline__ T varcoef_face(T h, T kc, T kn, T uc, T un) {
  const T ks = kc + kn;
  const T d = un - uc;
  const T f = ks * d;
  return h * f;
}

// one cell from memory: the generic kernel and the host loop
template <typename T>
__host__ __device__ inline T varcoef_cell(const VarCoefW<T> &vw, const T *u, const T *k, int64_t px, int64_t pxy) {
  const int64_t st[3] = {1, px, pxy};
  const T uc = u[0], kc = k[0];
  T acc = vw.shift * uc;
  for (int ax = 0; ax < 3; ++ax) {
    const T tm = varcoef_face<T>(vw.h[ax], kc, k[-st[ax]], uc, u[-st[ax]]);
    acc = acc + tm;
    const T tp = varcoef_face<T>(vw.h[ax], kc, k[st[ax]], uc, u[st[ax]]);
    acc = acc + tp;
  }
  return acc;
}

// 2.5D z-march for the aligned vector layout, stencil_star_kernel at radius 1 carrying two fields. Lane = one 16-B x
// chunk of TY rows; block = NW waves stacked in y over one column of 64 chunks. Per field the lane holds the centre
// plane and the plane ahead of it in march direction of its rows, with the plane entering next loaded one step ahead.
// The plane behind is not kept: its face term h * ((k(c) + k(behind)) * (u(behind) - u(c))) is computed one step early,
// while the cell that is then behind is still the centre, from the same operands by the same three operations (the sum
// k(c) + k(n) is shared with the face ahead: it is commutative bit for bit) and carried in registers. It is not taken
// as the negation of the face ahead, which differs in the sign of a zero when the two cells are equal. The z terms are
// added low face first whatever the march direction. The block's rows of the centre plane plus one halo row above and
// below (loaded by waves 0 and 1 during the step before) are shared through LDS, double-buffered by step parity with
// one barrier per step. x neighbours come from the adjacent lanes; only the wave-edge lanes load the cell beyond the
// wave from memory, one step ahead. Four waves per SIMD (two blocks per CU, as the LDS allows) mean 128 VGPRs: the
// rows read from LDS are loaded where the row loop uses them, not ahead of it, which keeps fp32 free of scratch and
// fp64 at two spilled registers (with them hoisted, 15 and 12 were spilled and the sweep ran 12 % slower).
template <typename T, int TY, int NW, bool NT>
__global__ __launch_bounds__(64 * NW, 4) void stencil_varcoef_kernel(VarCoefArgs<T> a) {
  using VT = typename Vec16<T>::type;
  constexpr int V = Vec16<T>::N;
  constexpr int ROWS = NW * TY + 2; // LDS row r holds raw y = yblk - 1 + r
  static_assert(NW >= 2, "one wave per halo row");
  __shared__ VT lds[2][2][ROWS][64]; // [field: 0 u, 1 kappa][step parity]
  const uint32_t nb = uint32_t(a.gx) * a.gy * a.gz;
  const uint32_t lb = a.remap ? xcd_remap(blockIdx.x, nb) : blockIdx.x;
  // logical order: z-chunk fastest, then y group, then x wave-column
  const int bz = int(lb % uint32_t(a.gz));
  const int by = int((lb / uint32_t(a.gz)) % uint32_t(a.gy));
  const int bx = int(lb / (uint32_t(a.gz) * a.gy));
  const int lane = threadIdx.x;
  const int w = int(threadIdx.y);
  const int c = bx * 64 + lane;
  const bool cvalid = c < a.nchunks;
  const int cl = cvalid ? c : a.nchunks - 1;
  const int xb = a.x0 + cl * V;
  const int yblk = a.loy + NW * TY * by;
  const int ybase = yblk + TY * w;
  const int zs = a.loz + bz * a.zc;
  const int ze = min(zs + a.zc, a.hiz);
  if (yblk >= a.hiy || zs >= ze) return; // block-uniform
  // odd z-chunks march downwards, so a chunk boundary is read by both neighbouring chunks at the same time
  const bool down = ((bz & 1) != 0) != (a.flip != 0);
  const int dz = down ? -1 : 1;
  const int z0 = down ? ze - 1 : zs;
  const int nzs = ze - zs;

  // The cell left of the wave's first chunk is loaded by lane 0. The cell right of its last chunk is loaded by lane 63
  // when that holds a chunk, else by the first lane without one (its clamped chunk is the last one), which hands it to
  // the last chunk's lane in place of its own first cell. No lane has two of these roles, so one register holds either.
  const bool edgeL = lane == 0;
  const bool edgeR = lane == 63 && cvalid;
  const bool edgeS = c == a.nchunks;
  const bool edge = edgeL || edgeR || edgeS;
  const int eoff = edgeL ? -1 : V;
  const bool fullX = xb >= a.lox && xb + V <= a.hix;
  // halo row of the block this wave loads (waves 0 and 1): the row above, the row below
  const bool hwave = w < 2;
  const int hy = w == 0 ? yblk - 1 : yblk + NW * TY;
  const int hrow = w == 0 ? 0 : NW * TY + 1;

  // element offset of the lane's chunk in row y of plane z, the same for both fields; rows past the allocation's last
  // row and planes outside it are clamped: those values are never used
  auto off = [&](int y, int z) -> int64_t {
    y = min(y, a.rawYm1);
    z = z < 0 ? 0 : (z > a.rawZm1 ? a.rawZm1 : z);
    return int64_t(z) * a.pxy + int64_t(y) * a.px + xb;
  };
  auto ld = [&](const T *p) -> VT { return *reinterpret_cast<const VT *>(p); };

  VT uc[TY], kc[TY], ua[TY], ka[TY], uinc[TY], kinc[TY]; // centre plane z, plane z + dz ahead, plane z + 2 dz entering
  T tb[TY][V];                                            // the face term towards the plane behind, z - dz
  T uce[TY], kce[TY], une[TY], kne[TY]; // edge lanes: their cell beyond the wave in the centre / next plane
  VT uh = VT(), kh = VT(); // waves 0 and 1: the block's halo row of the next centre plane
#pragma unroll
  for (int i = 0; i < TY; ++i) {
    const int64_t o = off(ybase + i, z0), ob = off(ybase + i, z0 - dz), oa = off(ybase + i, z0 + dz);
    uc[i] = ld(a.src + o);
    kc[i] = ld(a.coef + o);
    ua[i] = ld(a.src + oa);
    ka[i] = ld(a.coef + oa);
    const VT ub = ld(a.src + ob), kb = ld(a.coef + ob);
#pragma unroll
    for (int e = 0; e < V; ++e)
      tb[i][e] = varcoef_face<T>(a.vw.h[2], vget<T>(kc[i], e), vget<T>(kb, e), vget<T>(uc[i], e), vget<T>(ub, e));
    uce[i] = edge ? a.src[o + eoff] : T(0);
    kce[i] = edge ? a.coef[o + eoff] : T(0);
  }
  if (hwave) {
    const int64_t o0 = off(hy, z0);
    lds[0][0][hrow][lane] = ld(a.src + o0);
    lds[1][0][hrow][lane] = ld(a.coef + o0);
  }
#pragma unroll
  for (int i = 0; i < TY; ++i) {
    lds[0][0][1 + w * TY + i][lane] = uc[i];
    lds[1][0][1 + w * TY + i][lane] = kc[i];
  }
  __syncthreads();

  int buf = 0;
  int z = z0;
  for (int step = 0; step < nzs; ++step, z += dz) {
    // one step ahead: the next centre plane's halo row and edge cells, then the planes entering (loads return in
    // order: the halo row is published at the end of this step, the entering planes are not used before the next)
    if (hwave) {
      const int64_t o = off(hy, z + dz);
      uh = ld(a.src + o);
      kh = ld(a.coef + o);
    }
#pragma unroll
    for (int i = 0; i < TY; ++i) {
      const int64_t o = off(ybase + i, z + dz);
      une[i] = edge ? a.src[o + eoff] : T(0);
      kne[i] = edge ? a.coef[o + eoff] : T(0);
    }
#pragma unroll
    for (int i = 0; i < TY; ++i) {
      const int64_t o = off(ybase + i, z + 2 * dz);
      uinc[i] = ld(a.src + o);
      kinc[i] = ld(a.coef + o);
    }

#pragma unroll
    for (int i = 0; i < TY; ++i) {
      const int y = ybase + i;
      const VT ucv = uc[i], kcv = kc[i];
      // the rows above and below: the wave's own from registers, rows ybase - 1 and ybase + TY from LDS
      VT ulo, klo, uhi, khi;
      if (i > 0) {
        ulo = uc[i > 0 ? i - 1 : 0];
        klo = kc[i > 0 ? i - 1 : 0];
      } else {
        ulo = lds[0][buf][w * TY][lane];
        klo = lds[1][buf][w * TY][lane];
      }
      if (i + 1 < TY) {
        uhi = uc[i + 1 < TY ? i + 1 : 0];
        khi = kc[i + 1 < TY ? i + 1 : 0];
      } else {
        uhi = lds[0][buf][w * TY + TY + 1][lane];
        khi = lds[1][buf][w * TY + TY + 1][lane];
      }
      const T usl = shfl_up1<T>(vget<T>(ucv, V - 1)), usr = shfl_down1<T>(edgeS ? uce[i] : vget<T>(ucv, 0));
      const T ksl = shfl_up1<T>(vget<T>(kcv, V - 1)), ksr = shfl_down1<T>(edgeS ? kce[i] : vget<T>(kcv, 0));
      const T ulx = edgeL ? uce[i] : usl, urx = edgeR ? uce[i] : usr;
      const T klx = edgeL ? kce[i] : ksl, krx = edgeR ? kce[i] : ksr;
      T out[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const T u0 = vget<T>(ucv, e), k0 = vget<T>(kcv, e);
        T acc = a.vw.shift * u0;
        const T txm = varcoef_face<T>(a.vw.h[0], k0, e > 0 ? vget<T>(kcv, e - 1) : klx, u0, e > 0 ? vget<T>(ucv, e - 1) : ulx);
        acc = acc + txm;
        const T txp =
            varcoef_face<T>(a.vw.h[0], k0, e + 1 < V ? vget<T>(kcv, e + 1) : krx, u0, e + 1 < V ? vget<T>(ucv, e + 1) : urx);
        acc = acc + txp;
        const T tym = varcoef_face<T>(a.vw.h[1], k0, vget<T>(klo, e), u0, vget<T>(ulo, e));
        acc = acc + tym;
        const T typ = varcoef_face<T>(a.vw.h[1], k0, vget<T>(khi, e), u0, vget<T>(uhi, e));
        acc = acc + typ;
        // the face ahead, and the same face seen from the cell ahead (the next step's face behind): one sum of k
        const T u1 = vget<T>(ua[i], e);
        const T ks = k0 + vget<T>(ka[i], e);
        const T da = u1 - u0;
        const T fa = ks * da;
        const T ta = a.vw.h[2] * fa;
        const T db = u0 - u1;
        const T fb = ks * db;
        const T tbn = a.vw.h[2] * fb;
        const T tzm = down ? ta : tb[i][e], tzp = down ? tb[i][e] : ta;
        acc = acc + tzm;
        acc = acc + tzp;
        tb[i][e] = tbn;
        out[e] = acc;
      }
      if (cvalid && y < a.hiy) {
        T *dp = a.dst + int64_t(z) * a.pxy + int64_t(y) * a.px + xb;
        if (fullX) {
          using NV = typename Vec16<T>::native;
          NV v;
#pragma unroll
          for (int e = 0; e < V; ++e) v[e] = out[e];
          if (NT)
            __builtin_nontemporal_store(v, reinterpret_cast<NV *>(dp));
          else
            *reinterpret_cast<NV *>(dp) = v;
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e)
            if (xb + e >= a.lox && xb + e < a.hix) dp[e] = out[e];
        }
      }
    }

    // the plane ahead becomes the centre: publish its rows and the halo row loaded above, then take in the entering plane
    buf ^= 1;
#pragma unroll
    for (int i = 0; i < TY; ++i) {
      uc[i] = ua[i];
      kc[i] = ka[i];
      lds[0][buf][1 + w * TY + i][lane] = uc[i];
      lds[1][buf][1 + w * TY + i][lane] = kc[i];
    }
    if (hwave) {
      lds[0][buf][hrow][lane] = uh;
      lds[1][buf][hrow][lane] = kh;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TY; ++i) {
      ua[i] = uinc[i];
      ka[i] = kinc[i];
      uce[i] = une[i];
      kce[i] = kne[i];
    }
  }
}

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
// the star kernel's block shape, z-chunk floor and cap of blocks per CU (two blocks' LDS, 2 x 73 728 B, fit a CU)
constexpr int kVarTY = 2, kVarNW = 8, kVarMinZc = 16, kVarMaxBlocksPerCU = 2;

template <typename T> static void varcoef_host(const VarCoefArgs<T> &a) {
  for (int z = a.loz; z < a.hiz; ++z)
    for (int y = a.loy; y < a.hiy; ++y)
      for (int x = a.lox; x < a.hix; ++x) {
        const int64_t o = int64_t(z) * a.pxy + int64_t(y) * a.px + x;
        a.dst[o] = varcoef_cell<T>(a.vw, a.src + o, a.coef + o, a.px, a.pxy);
      }
}

// kernel arguments and the path apply takes for them; the fast path's grid is filled in (device sub-domains)
template <typename T>
static VarCoefArgs<T> varcoef_plan(const LocalDomain &dom, int64_t qu, int64_t qk, const Rect3 &region,
                                   const VarCoefWeights &wts, const StencilTune &tune, VarCoefLaunchInfo *info) {
  VarCoefArgs<T> a{};
  const Dim3 org = dom.accessor_origin();
  const Dim3 p = dom.pitch(qu);
  a.src = static_cast<const T *>(dom.curr_data(qu));
  a.coef = static_cast<const T *>(dom.curr_data(qk));
  a.dst = static_cast<T *>(dom.next_data(qu));
  a.px = p.x;
  a.pxy = p.x * p.y;
  a.lox = int(region.lo.x - org.x);
  a.loy = int(region.lo.y - org.y);
  a.loz = int(region.lo.z - org.z);
  a.hix = int(region.hi.x - org.x);
  a.hiy = int(region.hi.y - org.y);
  a.hiz = int(region.hi.z - org.z);
  a.rawYm1 = int(dom.raw_size().y - 1);
  a.rawZm1 = int(dom.raw_size().z - 1);
  a.remap = tune.xcdRemap ? 1 : 0;
  a.flip = tune.alternateZ ? (dom.parity() & 1) : 0;
  a.vw.shift = T(wts.shift);
  for (int ax = 0; ax < 3; ++ax) a.vw.h[ax] = T(wts.h[ax]);
  *info = VarCoefLaunchInfo();
  if (dom.backend() == Backend::Host) return a;
  info->path = 1;
  constexpr int V = Vec16<T>::N;
  const int rxm = int(dom.radius().x(-1));
  // chunk grid anchored at the 16-B aligned interior start
  const int off = ((a.lox - rxm) % V + V) % V;
  a.x0 = a.lox - off;
  a.nchunks = (a.hix - a.x0 + V - 1) / V;
  const bool alignedLayout = aligned_vector_layout(dom, qu, a.x0) && aligned_vector_layout(dom, qk, a.x0);
  // the last chunk's vector load and the cell right of it stay below both rows' read limits; the cell left of chunk 0
  // is a raw cell of the row (x0 >= the -x radius >= 1)
  const int64_t last = a.x0 + int64_t(a.nchunks) * V + 1;
  const bool fits = last <= dom.row_limit(qu) && last <= dom.row_limit(qk) && a.x0 >= 1;
  if (!(alignedLayout && fits)) return a;
  info->path = 2;
  const int ny = a.hiy - a.loy, nz = a.hiz - a.loz;
  a.gx = (a.nchunks + 63) / 64;
  a.gy = (ny + kVarNW * kVarTY - 1) / (kVarNW * kVarTY);
  int zc = tune.zchunk;
  if (zc <= 0) {
    // one round of resident blocks (occupancy, at most two per CU, x CUs), z chunks of at least kVarMinZc planes
    // (each re-reads 2)
    dom.set_device();
    const void *kern = tune.nontemporal ? (const void *)stencil_varcoef_kernel<T, kVarTY, kVarNW, true>
                                        : (const void *)stencil_varcoef_kernel<T, kVarTY, kVarNW, false>;
    const int64_t cols = int64_t(a.gx) * a.gy;
    const int64_t resident = std::min(resident_blocks(kern, 64 * kVarNW, 2),
                                      int64_t(kVarMaxBlocksPerCU) * device_cus(dom.gpu()));
    const int64_t nzc = std::max<int64_t>(1, resident / cols);
    zc = int(std::max<int64_t>(kVarMinZc, (nz + nzc - 1) / nzc));
  }
  a.zc = zc;
  a.gz = (nz + zc - 1) / zc;
  info->zchunk = zc;
  info->zchunks = a.gz;
  info->blocks = int64_t(a.gx) * a.gy * a.gz;
  return a;
}

template <typename T>
static void varcoef_apply_t(const LocalDomain &dom, int64_t qu, int64_t qk, const Rect3 &region,
                            const VarCoefWeights &wts, hipStream_t stream, const StencilTune &tune) {
  VarCoefLaunchInfo info;
  const VarCoefArgs<T> a = varcoef_plan<T>(dom, qu, qk, region, wts, tune, &info);
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

static bool varcoef_fp(const LocalDomain &dom, int64_t qi, bool *f64) {
  if (qi < 0 || qi >= dom.num_data()) return false;
  const DType dt = dom.dtype(qi);
  const int64_t es = dom.elem_size(qi);
  *f64 = dt == DType::F64 || (dt == DType::Bytes && es == 8);
  return *f64 || dt == DType::F32 || (dt == DType::Bytes && es == 4);
}

static bool varcoef_radii_ok(const LocalDomain &dom) {
  const Radius &rd = dom.radius();
  return rd.x(-1) >= 1 && rd.x(1) >= 1 && rd.y(-1) >= 1 && rd.y(1) >= 1 && rd.z(-1) >= 1 && rd.z(1) >= 1;
}

static bool varcoef_same_layout(const LocalDomain &dom, int64_t qu, int64_t qk) {
  return dom.elem_size(qu) == dom.elem_size(qk) && dom.pitch(qu) == dom.pitch(qk);
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
    varcoef_plan<float>(dom, qu, qk, region, w, tune, &info);
  else
    varcoef_plan<double>(dom, qu, qk, region, w, tune, &info);
  return info;
}

} // namespace stencil
