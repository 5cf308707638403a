#pragma once
// Shared by stencil_varcoef.hip (the operator) and stencil_varcoef_relax.hip (residual / damped Jacobi): the kernel
// arguments, the face term, the 2.5D z-march and the host plan of the variable-coefficient stencils.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <initializer_list>
#include <type_traits>

#include "stencil_common.hpp"
#include "stencil/kernels/stencil_ops.hpp"

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
  T *dst;        // raw [0,0,0] of the destination (the operator: next(u))
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

// the relax kernels' arguments: the operator's, the right-hand side and omega in the element type
template <typename T> struct VarCoefRelaxArgs : VarCoefArgs<T> {
  const T *rhs; // raw [0,0,0] of curr(f): the pitches of u
  T omega;
};

// what the march computes per cell: the operator, f - A u, or u + omega (f - A u) / diag(A)
enum VarCoefMode { kVarApply = 0, kVarResidual = 1, kVarJacobi = 2 };

// one face: h * ((k(c) + k(n)) * (u(n) - u(c))), three roundings after the two of the operands
template <typename T> __host__ __device__ __forceinline__ T varcoef_face(T h, T kc, T kn, T uc, T un) {
  const T ks = kc + kn;
  const T d = un - uc;
  const T f = ks * d;
  return h * f;
}

// the same face, and its share g = h * (k(c) + k(n)) of the diagonal, from the same sum of k
template <typename T> __host__ __device__ __forceinline__ T varcoef_face_diag(T h, T kc, T kn, T uc, T un, T *g) {
  const T ks = kc + kn;
  const T d = un - uc;
  const T f = ks * d;
  *g = h * ks;
  return h * f;
}

// what is stored for a cell with operator value acc and diagonal dg: r = f - acc, or u + omega * (r / dg) (IEEE
// division, three roundings)
template <typename T, int MODE> __host__ __device__ __forceinline__ T varcoef_relax_value(T acc, T dg, T u0, T f0, T omega) {
  const T r = f0 - acc;
  if (MODE == kVarResidual) return r;
  const T q = r / dg;
  const T s = omega * q;
  return u0 + s;
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

// one cell of the residual / Jacobi update from memory
template <typename T, int MODE>
__host__ __device__ inline T varcoef_relax_cell(const VarCoefW<T> &vw, T omega, const T *u, const T *k, const T *f,
                                                int64_t px, int64_t pxy) {
  const int64_t st[3] = {1, px, pxy};
  const T uc = u[0], kc = k[0];
  T acc = vw.shift * uc;
  T dg = vw.shift;
  for (int ax = 0; ax < 3; ++ax) {
    T g;
    const T tm = varcoef_face_diag<T>(vw.h[ax], kc, k[-st[ax]], uc, u[-st[ax]], &g);
    acc = acc + tm;
    dg = dg - g;
    const T tp = varcoef_face_diag<T>(vw.h[ax], kc, k[st[ax]], uc, u[st[ax]], &g);
    acc = acc + tp;
    dg = dg - g;
  }
  return varcoef_relax_value<T, MODE>(acc, dg, uc, f[0], omega);
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
// wave from memory, one step ahead. The rows read from LDS are loaded where the row loop uses them, not ahead of it.
//
// MODE != kVarApply (stencil_varcoef_relax.hip) adds the diagonal dg = shift - sum of h * (k(c) + k(n)) over the six
// faces, low face first per axis as the operator's sum: the share of the face behind is that of the face ahead one
// step earlier (the same sum of k, the same product), so it is carried beside the face term. The right-hand side is
// read at the centre only, its rows loaded one step ahead with the edge cells, and the value stored is
// varcoef_relax_value. WPS, the waves per SIMD the registers are bounded for, is 2 there (one block per CU): bounded
// to 4 like the operator the Jacobi kernels spilled 26 to 57 registers and ran 1.4 to 2.2 times longer.
template <typename T, int TY, int NW, bool NT, int MODE = kVarApply, int WPS = 4>
__global__ __launch_bounds__(64 * NW, WPS) void stencil_varcoef_kernel(
    std::conditional_t<MODE == kVarApply, VarCoefArgs<T>, VarCoefRelaxArgs<T>> a) {
  using VT = typename Vec16<T>::type;
  constexpr int V = Vec16<T>::N;
  constexpr int ROWS = NW * TY + 2; // LDS row r holds raw y = yblk - 1 + r
  constexpr bool RELAX = MODE != kVarApply;
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

  // element offset of the lane's chunk in row y of plane z, the same for every field; rows past the allocation's last
  // row and planes outside it are clamped: those values are never used
  auto off = [&](int y, int z) -> int64_t {
    y = min(y, a.rawYm1);
    z = z < 0 ? 0 : (z > a.rawZm1 ? a.rawZm1 : z);
    return int64_t(z) * a.pxy + int64_t(y) * a.px + xb;
  };
  auto ld = [&](const T *p) -> VT { return *reinterpret_cast<const VT *>(p); };

  VT uc[TY], kc[TY], ua[TY], ka[TY], uinc[TY], kinc[TY]; // centre plane z, plane z + dz ahead, plane z + 2 dz entering
  T tb[TY][V];                                            // the face term towards the plane behind, z - dz
  T gb[RELAX ? TY : 1][V];                                // its share of the diagonal
  VT fc[RELAX ? TY : 1], finc[RELAX ? TY : 1];            // the right-hand side's centre plane, and its next
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
    for (int e = 0; e < V; ++e) {
      if (RELAX)
        tb[i][e] = varcoef_face_diag<T>(a.vw.h[2], vget<T>(kc[i], e), vget<T>(kb, e), vget<T>(uc[i], e), vget<T>(ub, e),
                                        &gb[i][e]);
      else
        tb[i][e] = varcoef_face<T>(a.vw.h[2], vget<T>(kc[i], e), vget<T>(kb, e), vget<T>(uc[i], e), vget<T>(ub, e));
    }
    uce[i] = edge ? a.src[o + eoff] : T(0);
    kce[i] = edge ? a.coef[o + eoff] : T(0);
    if constexpr (RELAX) fc[i] = ld(a.rhs + o);
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
      if constexpr (RELAX) finc[i] = ld(a.rhs + o);
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
      const VT fv = fc[RELAX ? i : 0];
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
        if (!RELAX) {
          const T txm = varcoef_face<T>(a.vw.h[0], k0, e > 0 ? vget<T>(kcv, e - 1) : klx, u0, e > 0 ? vget<T>(ucv, e - 1) : ulx);
          acc = acc + txm;
          const T txp =
              varcoef_face<T>(a.vw.h[0], k0, e + 1 < V ? vget<T>(kcv, e + 1) : krx, u0, e + 1 < V ? vget<T>(ucv, e + 1) : urx);
          acc = acc + txp;
          const T tym = varcoef_face<T>(a.vw.h[1], k0, vget<T>(klo, e), u0, vget<T>(ulo, e));
          acc = acc + tym;
          const T typ = varcoef_face<T>(a.vw.h[1], k0, vget<T>(khi, e), u0, vget<T>(uhi, e));
          acc = acc + typ;
        }
        T dg = a.vw.shift;
        if (RELAX) {
          T g;
          const T txm = varcoef_face_diag<T>(a.vw.h[0], k0, e > 0 ? vget<T>(kcv, e - 1) : klx, u0,
                                             e > 0 ? vget<T>(ucv, e - 1) : ulx, &g);
          acc = acc + txm;
          dg = dg - g;
          const T txp = varcoef_face_diag<T>(a.vw.h[0], k0, e + 1 < V ? vget<T>(kcv, e + 1) : krx, u0,
                                             e + 1 < V ? vget<T>(ucv, e + 1) : urx, &g);
          acc = acc + txp;
          dg = dg - g;
          const T tym = varcoef_face_diag<T>(a.vw.h[1], k0, vget<T>(klo, e), u0, vget<T>(ulo, e), &g);
          acc = acc + tym;
          dg = dg - g;
          const T typ = varcoef_face_diag<T>(a.vw.h[1], k0, vget<T>(khi, e), u0, vget<T>(uhi, e), &g);
          acc = acc + typ;
          dg = dg - g;
        }
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
        if constexpr (RELAX) {
          // h * ks is the diagonal share of the face ahead here and of the face behind at the next step
          const T ga = a.vw.h[2] * ks;
          const T gzm = down ? ga : gb[i][e], gzp = down ? gb[i][e] : ga;
          dg = dg - gzm;
          dg = dg - gzp;
          gb[i][e] = ga;
          out[e] = varcoef_relax_value<T, MODE>(acc, dg, u0, vget<T>(fv, e), a.omega);
        } else {
          out[e] = acc;
        }
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
      if (RELAX) fc[i] = finc[i];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
// the star kernel's block shape, z-chunk floor and cap of blocks per CU (two blocks' LDS, 2 x 73 728 B, fit a CU)
constexpr int kVarTY = 2, kVarNW = 8, kVarMinZc = 16, kVarMaxBlocksPerCU = 2;

// Kernel arguments and the path a launch takes for them; the fast path's grid is filled in (device sub-domains).
// `dst`: the buffer written; `others`: further quantities whose curr buffers the fast kernel reads or writes in 16-B
// chunks (the right-hand side and the destination of the relax kernels); `kern`: the kernel whose occupancy sizes the
// automatic z chunk.
template <typename T>
inline VarCoefArgs<T> varcoef_plan(const LocalDomain &dom, int64_t qu, int64_t qk, T *dst,
                                   std::initializer_list<int64_t> others, const Rect3 &region, const VarCoefWeights &wts,
                                   const StencilTune &tune, const void *kern, VarCoefLaunchInfo *info) {
  VarCoefArgs<T> a{};
  const Dim3 org = dom.accessor_origin();
  const Dim3 p = dom.pitch(qu);
  a.src = static_cast<const T *>(dom.curr_data(qu));
  a.coef = static_cast<const T *>(dom.curr_data(qk));
  a.dst = dst;
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
  bool alignedLayout = aligned_vector_layout(dom, qu, a.x0) && aligned_vector_layout(dom, qk, a.x0);
  // the last chunk's vector load and the cell right of it stay below every row's read limit; the cell left of chunk 0
  // is a raw cell of the row (x0 >= the -x radius >= 1)
  const int64_t last = a.x0 + int64_t(a.nchunks) * V + 1;
  bool fits = last <= dom.row_limit(qu) && last <= dom.row_limit(qk) && a.x0 >= 1;
  for (int64_t q : others) {
    alignedLayout = alignedLayout && aligned_vector_layout(dom, q, a.x0);
    fits = fits && last <= dom.row_limit(q);
  }
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

inline bool varcoef_fp(const LocalDomain &dom, int64_t qi, bool *f64) {
  if (qi < 0 || qi >= dom.num_data()) return false;
  const DType dt = dom.dtype(qi);
  const int64_t es = dom.elem_size(qi);
  *f64 = dt == DType::F64 || (dt == DType::Bytes && es == 8);
  return *f64 || dt == DType::F32 || (dt == DType::Bytes && es == 4);
}

inline bool varcoef_radii_ok(const LocalDomain &dom) {
  const Radius &rd = dom.radius();
  return rd.x(-1) >= 1 && rd.x(1) >= 1 && rd.y(-1) >= 1 && rd.y(1) >= 1 && rd.z(-1) >= 1 && rd.z(1) >= 1;
}

inline bool varcoef_same_layout(const LocalDomain &dom, int64_t qu, int64_t qk) {
  return dom.elem_size(qu) == dom.elem_size(qk) && dom.pitch(qu) == dom.pitch(qk);
}

} // namespace stencil
