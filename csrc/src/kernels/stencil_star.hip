// Weighted star stencils of radius 1-3 for gfx950. See stencil/kernels/stencil_ops.hpp (StarWeights).
//   next(c) = center * u(c) + sum over axis x, y, z and k = 1..R of w[axis][-][k] * u(c - k e) + w[axis][+][k] * u(c + k e)
// Every product and every sum is its own rounding, in exactly that order, in the fast kernel, the generic kernel and
// the host loop alike, so all three are bitwise equal to stencil2_amd.ops.star_step_reference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>

#include "stencil_common.hpp"
#include "stencil/kernels/stencil_ops.hpp"
#include "stencil/rt/hip_check.hpp"

// no FMA contraction anywhere below, device or host (hipcc contracts by default)
#pragma clang fp contract(off)

namespace stencil {

// the weights in the element type (converted once on the host), passed by value in the kernel arguments
template <typename T, int R> struct StarW {
  T c;
  T w[3][2][R]; // [axis][0: -, 1: +][k - 1]
};

template <typename T, int R> struct StarArgs {
  const T *src; // raw [0,0,0] of curr
  T *dst;       // raw [0,0,0] of next
  int64_t px, pxy;
  int lox, loy, loz, hix, hiy, hiz; // region, raw coordinates
  int x0;                           // raw x of chunk 0 (16-B aligned in memory)
  int nchunks;                      // chunks covering [x0, hix)
  int rawYm1, rawZm1;               // clamps of the row / plane prefetches
  int zc;                           // planes per block
  int gx, gy, gz;                   // logical grid
  int remap;                        // XCD-aware block remap
  int flip;                         // reverse every block's z-march direction
  StarW<T, R> sw;
};

// one cell from memory: the generic kernel and the host loop
template <typename T, int R>
__host__ __device__ inline T star_cell(const StarW<T, R> &sw, const T *p, int64_t px, int64_t pxy) {
  const int64_t st[3] = {1, px, pxy};
  T acc = sw.c * p[0];
  for (int ax = 0; ax < 3; ++ax)
    for (int k = 1; k <= R; ++k) {
      const T m = sw.w[ax][0][k - 1] * p[-k * st[ax]];
      acc = acc + m;
      const T q = sw.w[ax][1][k - 1] * p[k * st[ax]];
      acc = acc + q;
    }
  return acc;
}

// 2.5D z-march for the aligned vector layout. Lane = one 16-B x chunk of TY rows; block = NW waves stacked in y over
// one column of 64 chunks. A register ring holds the 2R+1 planes z-R .. z+R of the lane's rows (in z order whatever the
// march direction; the plane entering next is loaded one step ahead). The block's rows of the centre plane plus R halo
// rows above and below (loaded by the first 2R waves, one step ahead) are shared through LDS, double-buffered by step
// parity with one barrier per step. x neighbours up to R cells away come from the adjacent lanes (the third cell of an
// fp64 chunk's neighbour through the adjacent lane's own neighbour cell); only the wave-edge lanes load the R cells
// beyond the wave from memory, one step ahead.
template <typename T, int R, int TY, int NW, bool NT>
__global__ __launch_bounds__(64 * NW) void stencil_star_kernel(StarArgs<T, R> a) {
  using VT = typename Vec16<T>::type;
  constexpr int V = Vec16<T>::N;
  constexpr int ROWS = NW * TY + 2 * R; // LDS row r holds raw y = yblk - R + r
  constexpr int NP = 2 * R + 1;
  static_assert(NW >= 2 * R, "one wave per halo row");
  static_assert(R >= 1 && R <= 3 && R <= 2 * V, "x neighbours reach at most two lanes");
  __shared__ VT lds[2][ROWS][64];
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

  const bool edgeL = lane == 0;
  const bool edgeR = lane == 63 || c + 1 >= a.nchunks;
  const bool fullX = xb >= a.lox && xb + V <= a.hix;
  // halo row of the block this wave loads (waves 0 .. 2R-1): R rows above, R rows below
  const bool hwave = w < 2 * R;
  const int hy = w < R ? yblk - R + w : yblk + NW * TY + (w - R);
  const int hrow = w < R ? w : NW * TY + w;

  // rows past the allocation's last row and planes outside it are clamped: those values are never used
  auto rowp = [&](int y, int z) -> const T * {
    y = min(y, a.rawYm1);
    z = z < 0 ? 0 : (z > a.rawZm1 ? a.rawZm1 : z);
    return a.src + int64_t(z) * a.pxy + int64_t(y) * a.px + xb;
  };
  auto ld = [&](const T *p) -> VT { return *reinterpret_cast<const VT *>(p); };

  VT ring[NP][TY], inc[TY]; // ring[j] = plane z + j - R
  T cL[TY][R], cR[TY][R], nL[TY][R], nR[TY][R]; // edge lanes: u(xb - 1 - k) / u(xb + V + k) of the centre / next plane
  VT haloC = VT(), haloN = VT();
#pragma unroll
  for (int j = 0; j < NP; ++j)
#pragma unroll
    for (int i = 0; i < TY; ++i) ring[j][i] = ld(rowp(ybase + i, z0 + j - R));
#pragma unroll
  for (int i = 0; i < TY; ++i) {
    const T *p = rowp(ybase + i, z0);
#pragma unroll
    for (int k = 0; k < R; ++k) {
      cL[i][k] = edgeL ? p[-1 - k] : T(0);
      cR[i][k] = edgeR ? p[V + k] : T(0);
    }
  }
  if (hwave) {
    lds[0][hrow][lane] = ld(rowp(hy, z0));
    haloC = ld(rowp(hy, z0 + dz));
  }
#pragma unroll
  for (int i = 0; i < TY; ++i) lds[0][R + w * TY + i][lane] = ring[R][i];
  __syncthreads();

  int buf = 0;
  int z = z0;
  for (int step = 0; step < nzs; ++step, z += dz) {
    // one step ahead: the plane entering the ring, the next centre plane's edge cells and halo row
#pragma unroll
    for (int i = 0; i < TY; ++i) inc[i] = ld(rowp(ybase + i, z + (R + 1) * dz));
#pragma unroll
    for (int i = 0; i < TY; ++i) {
      const T *p = rowp(ybase + i, z + dz);
#pragma unroll
      for (int k = 0; k < R; ++k) {
        nL[i][k] = edgeL ? p[-1 - k] : T(0);
        nR[i][k] = edgeR ? p[V + k] : T(0);
      }
    }
    if (hwave) haloN = ld(rowp(hy, z + 2 * dz));

    // rows ybase - R .. ybase + TY - 1 + R of the centre plane: the wave's own from registers, the rest from LDS
    VT yv[TY + 2 * R];
#pragma unroll
    for (int j = 0; j < TY + 2 * R; ++j) {
      if (j >= R && j < R + TY)
        yv[j] = ring[R][j - R];
      else
        yv[j] = lds[buf][w * TY + j][lane];
    }

#pragma unroll
    for (int i = 0; i < TY; ++i) {
      const int y = ybase + i;
      const VT cc = ring[R][i];
      // lx[m - 1] = u(xb - m), rx[m - 1] = u(xb + V - 1 + m); beyond the adjacent chunk: that lane's own neighbour
      T lx[R] = {}, rx[R] = {};
#pragma unroll
      for (int m = 1; m <= R; ++m) {
        const int far = m > V ? m - V - 1 : 0; // m > V only
        const T sl = shfl_up1<T>(m <= V ? vget<T>(cc, V - m) : lx[far]);
        const T sr = shfl_down1<T>(m <= V ? vget<T>(cc, m - 1) : rx[far]);
        lx[m - 1] = edgeL ? cL[i][m - 1] : sl;
        rx[m - 1] = edgeR ? cR[i][m - 1] : sr;
      }
      T out[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        T acc = a.sw.c * vget<T>(cc, e);
#pragma unroll
        for (int k = 1; k <= R; ++k) {
          const T um = e - k >= 0 ? vget<T>(cc, e - k) : lx[k - e - 1 > 0 ? k - e - 1 : 0];
          const T up = e + k < V ? vget<T>(cc, e + k) : rx[e + k - V > 0 ? e + k - V : 0];
          const T pm = a.sw.w[0][0][k - 1] * um;
          acc = acc + pm;
          const T pp = a.sw.w[0][1][k - 1] * up;
          acc = acc + pp;
        }
#pragma unroll
        for (int k = 1; k <= R; ++k) {
          const T pm = a.sw.w[1][0][k - 1] * vget<T>(yv[R + i - k], e);
          acc = acc + pm;
          const T pp = a.sw.w[1][1][k - 1] * vget<T>(yv[R + i + k], e);
          acc = acc + pp;
        }
#pragma unroll
        for (int k = 1; k <= R; ++k) {
          const T pm = a.sw.w[2][0][k - 1] * vget<T>(ring[R - k][i], e);
          acc = acc + pm;
          const T pp = a.sw.w[2][1][k - 1] * vget<T>(ring[R + k][i], e);
          acc = acc + pp;
        }
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

    // advance the ring (kept in z order), publish the next centre plane's rows, then take in the plane loaded above
    if (!down) {
#pragma unroll
      for (int j = 0; j + 1 < NP; ++j)
#pragma unroll
        for (int i = 0; i < TY; ++i) ring[j][i] = ring[j + 1][i];
    } else {
#pragma unroll
      for (int j = NP - 1; j > 0; --j)
#pragma unroll
        for (int i = 0; i < TY; ++i) ring[j][i] = ring[j - 1][i];
    }
    buf ^= 1;
#pragma unroll
    for (int i = 0; i < TY; ++i) lds[buf][R + w * TY + i][lane] = ring[R][i];
    if (hwave) {
      lds[buf][hrow][lane] = haloC;
      haloC = haloN;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < TY; ++i) {
      if (!down)
        ring[NP - 1][i] = inc[i];
      else
        ring[0][i] = inc[i];
#pragma unroll
      for (int k = 0; k < R; ++k) {
        cL[i][k] = nL[i][k];
        cR[i][k] = nR[i][k];
      }
    }
  }
}

// one thread per cell: every layout or region the fast path refuses
template <typename T, int R> __global__ __launch_bounds__(256) void stencil_star_generic_kernel(StarArgs<T, R> a) {
  const int64_t nx = a.hix - a.lox, ny = a.hiy - a.loy, nz = a.hiz - a.loz;
  const int64_t total = nx * ny * nz;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int x = a.lox + int(i % nx), y = a.loy + int((i / nx) % ny), z = a.loz + int(i / (nx * ny));
    const int64_t o = int64_t(z) * a.pxy + int64_t(y) * a.px + x;
    a.dst[o] = star_cell<T, R>(a.sw, a.src + o, a.px, a.pxy);
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
constexpr int kStarTY = 2, kStarNW = 8, kStarMinZc = 16, kStarMaxBlocksPerCU = 2;

template <typename T, int R> static void star_host(const StarArgs<T, R> &a) {
  for (int z = a.loz; z < a.hiz; ++z)
    for (int y = a.loy; y < a.hiy; ++y)
      for (int x = a.lox; x < a.hix; ++x) {
        const int64_t o = int64_t(z) * a.pxy + int64_t(y) * a.px + x;
        a.dst[o] = star_cell<T, R>(a.sw, a.src + o, a.px, a.pxy);
      }
}

// kernel arguments and the path apply takes for them; the fast path's grid is filled in (device sub-domains)
template <typename T, int R>
static StarArgs<T, R> star_plan(const LocalDomain &dom, int64_t qi, const Rect3 &region, const StarWeights &wts,
                                const StencilTune &tune, StarLaunchInfo *info) {
  StarArgs<T, R> a{};
  const Dim3 org = dom.accessor_origin();
  const Dim3 p = dom.pitch(qi);
  a.src = static_cast<const T *>(dom.curr_data(qi));
  a.dst = static_cast<T *>(dom.next_data(qi));
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
  a.sw.c = T(wts.center);
  for (int ax = 0; ax < 3; ++ax)
    for (int s = 0; s < 2; ++s)
      for (int k = 0; k < R; ++k) a.sw.w[ax][s][k] = T(wts.w[ax][s][k]);
  *info = StarLaunchInfo();
  if (dom.backend() == Backend::Host) return a;
  info->path = 1;
  constexpr int V = Vec16<T>::N;
  const int rxm = int(dom.radius().x(-1));
  // chunk grid anchored at the 16-B aligned interior start
  const int off = ((a.lox - rxm) % V + V) % V;
  a.x0 = a.lox - off;
  a.nchunks = (a.hix - a.x0 + V - 1) / V;
  const bool alignedLayout = aligned_vector_layout(dom, qi, a.x0);
  // the last chunk's vector load and the R cells right of it stay below the row's read limit; the R cells left of
  // chunk 0 are raw cells of the row (x0 >= the -x radius >= R)
  const bool fits = a.x0 + int64_t(a.nchunks) * V + R <= dom.row_limit(qi) && a.x0 >= R;
  if (!(alignedLayout && fits)) return a;
  info->path = 2;
  const int ny = a.hiy - a.loy, nz = a.hiz - a.loz;
  a.gx = (a.nchunks + 63) / 64;
  a.gy = (ny + kStarNW * kStarTY - 1) / (kStarNW * kStarTY);
  int zc = tune.zchunk;
  if (zc <= 0) {
    // one round of resident blocks (occupancy, at most two per CU, x CUs), z chunks of at least kStarMinZc planes
    // (each re-reads 2R)
    dom.set_device();
    const void *kern = tune.nontemporal ? (const void *)stencil_star_kernel<T, R, kStarTY, kStarNW, true>
                                        : (const void *)stencil_star_kernel<T, R, kStarTY, kStarNW, false>;
    const int64_t cols = int64_t(a.gx) * a.gy;
    // at most two blocks per CU: the radius-1 fp32 kernel fits three, but 512^3 in 768 blocks ran 221 us against 212 us
    // in 512 or 256 blocks (profiles/star/bench_stencil_starzc.csv); the other instances fit one or two anyway
    const int64_t resident = std::min(resident_blocks(kern, 64 * kStarNW, 2),
                                      int64_t(kStarMaxBlocksPerCU) * device_cus(dom.gpu()));
    const int64_t nzc = std::max<int64_t>(1, resident / cols);
    zc = int(std::max<int64_t>(kStarMinZc, (nz + nzc - 1) / nzc));
  }
  a.zc = zc;
  a.gz = (nz + zc - 1) / zc;
  info->zchunk = zc;
  info->zchunks = a.gz;
  info->blocks = int64_t(a.gx) * a.gy * a.gz;
  return a;
}

template <typename T, int R>
static void star_apply_t(const LocalDomain &dom, int64_t qi, const Rect3 &region, const StarWeights &wts,
                         hipStream_t stream, const StencilTune &tune) {
  StarLaunchInfo info;
  const StarArgs<T, R> a = star_plan<T, R>(dom, qi, region, wts, tune, &info);
  if (info.path == 0) {
    star_host<T, R>(a);
    return;
  }
  dom.set_device();
  if (info.path == 2) {
    const dim3 block(64, kStarNW);
    if (tune.nontemporal)
      hipLaunchKernelGGL((stencil_star_kernel<T, R, kStarTY, kStarNW, true>), dim3(uint32_t(info.blocks)), block, 0, stream, a);
    else
      hipLaunchKernelGGL((stencil_star_kernel<T, R, kStarTY, kStarNW, false>), dim3(uint32_t(info.blocks)), block, 0, stream, a);
  } else {
    const int64_t total = int64_t(a.hix - a.lox) * (a.hiy - a.loy) * (a.hiz - a.loz);
    const int blocks = int(std::min<int64_t>((total + 255) / 256, 4096));
    hipLaunchKernelGGL((stencil_star_generic_kernel<T, R>), dim3(blocks), dim3(256), 0, stream, a);
  }
  HIP_CHECK(hipGetLastError());
}

static bool star_fp(const LocalDomain &dom, int64_t qi, bool *f64) {
  const DType dt = dom.dtype(qi);
  const int64_t es = dom.elem_size(qi);
  *f64 = dt == DType::F64 || (dt == DType::Bytes && es == 8);
  return *f64 || dt == DType::F32 || (dt == DType::Bytes && es == 4);
}

static bool star_radii_ok(const LocalDomain &dom, int r) {
  const Radius &rd = dom.radius();
  return rd.x(-1) >= r && rd.x(1) >= r && rd.y(-1) >= r && rd.y(1) >= r && rd.z(-1) >= r && rd.z(1) >= r;
}

bool stencil_star_supported(const LocalDomain &dom, int64_t qi, const StarWeights &w) {
  bool f64 = false;
  if (qi < 0 || qi >= dom.num_data() || !star_fp(dom, qi, &f64)) return false;
  return w.radius >= 1 && w.radius <= 3 && star_radii_ok(dom, w.radius);
}

// the refusals shared by apply and launch_info; false: nothing to do (empty region)
static bool star_check(const LocalDomain &dom, int64_t qi, const Rect3 &region, const StarWeights &w,
                       const StencilTune &tune, bool *f64) {
  STENCIL_REQUIRE(w.radius >= 1 && w.radius <= 3, "star stencil radius " << w.radius << " is not 1, 2 or 3");
  STENCIL_REQUIRE(qi >= 0 && qi < dom.num_data() && star_fp(dom, qi, f64), "star stencils take fp32 / fp64 quantities");
  STENCIL_REQUIRE(star_radii_ok(dom, w.radius), "star stencil of radius " << w.radius << " needs face radii >= " << w.radius);
  STENCIL_REQUIRE(tune.wrap == 0, "star stencils read halos (no in-kernel wrap)");
  require_region_in_compute(dom, region);
  return !region.empty();
}

void stencil_star_apply(const LocalDomain &dom, int64_t qi, const Rect3 &region, const StarWeights &w, hipStream_t stream,
                        const StencilTune &tune) {
  bool f64 = false;
  if (!star_check(dom, qi, region, w, tune, &f64)) return;
  if (!f64) {
    if (w.radius == 1)
      star_apply_t<float, 1>(dom, qi, region, w, stream, tune);
    else if (w.radius == 2)
      star_apply_t<float, 2>(dom, qi, region, w, stream, tune);
    else
      star_apply_t<float, 3>(dom, qi, region, w, stream, tune);
  } else {
    if (w.radius == 1)
      star_apply_t<double, 1>(dom, qi, region, w, stream, tune);
    else if (w.radius == 2)
      star_apply_t<double, 2>(dom, qi, region, w, stream, tune);
    else
      star_apply_t<double, 3>(dom, qi, region, w, stream, tune);
  }
}

StarLaunchInfo stencil_star_launch_info(const LocalDomain &dom, int64_t qi, const Rect3 &region, const StarWeights &w,
                                        const StencilTune &tune) {
  StarLaunchInfo info;
  bool f64 = false;
  if (!star_check(dom, qi, region, w, tune, &f64)) {
    info.path = -1;
    return info;
  }
  if (!f64) {
    if (w.radius == 1)
      star_plan<float, 1>(dom, qi, region, w, tune, &info);
    else if (w.radius == 2)
      star_plan<float, 2>(dom, qi, region, w, tune, &info);
    else
      star_plan<float, 3>(dom, qi, region, w, tune, &info);
  } else {
    if (w.radius == 1)
      star_plan<double, 1>(dom, qi, region, w, tune, &info);
    else if (w.radius == 2)
      star_plan<double, 2>(dom, qi, region, w, tune, &info);
    else
      star_plan<double, 3>(dom, qi, region, w, tune, &info);
  }
  return info;
}

} // namespace stencil
