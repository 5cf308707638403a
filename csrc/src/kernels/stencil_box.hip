// Weighted 27-point box stencils for gfx950. See stencil/kernels/stencil_ops.hpp (BoxWeights).
//   next(c) = sum over (dz, dy, dx) in {-1, 0, 1}^3, lexicographic with dz slowest and dx fastest, of
//             w[dz][dy][dx] * u(c + (dx, dy, dz))
// The first term is a product alone; every later product and every sum is its own rounding, in exactly that order, in
// the fast kernel, the generic kernel and the host loop alike, so all three are bitwise
// equal to stencil2_amd.ops.box_step_reference.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>

#include "stencil_common.hpp"
#include "stencil_wave.hpp"
#include "stencil/kernels/stencil_ops.hpp"
#include "stencil/rt/hip_check.hpp"

// no FMA contraction anywhere below, device or host (hipcc contracts by default)
#pragma clang fp contract(off)

namespace stencil {

// the weights in the element type (converted once on the host), passed by value in the kernel arguments
template <typename T> struct BoxW {
  T w[3][3][3]; // [dz + 1][dy + 1][dx + 1]
};

template <typename T> struct BoxArgs {
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
  BoxW<T> bw;
};

// one cell from memory: the generic kernel and the host loop
template <typename T> __host__ __device__ inline T box_cell(const BoxW<T> &bw, const T *p, int64_t px, int64_t pxy) {
  T acc = T(0);
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const T t = bw.w[dz + 1][dy + 1][dx + 1] * p[dz * pxy + dy * px + dx];
        acc = (dz == -1 && dy == -1 && dx == -1) ? t : acc + t;
      }
  return acc;
}

// the operand pairs of one row for the two output pairs of a chunk: fp32 pairs output cells (0, 2) and (1, 3), so the
// six operands of dx = -1, 0, +1 are the four pairs (l, y), (x, z), (y, w), (z, r), each held once in an aligned register
// pair (no per-term copies); fp64 has one output pair (0, 1) and no packed form
template <typename T> struct BoxRowOps;
template <> struct BoxRowOps<float> {
  typedef Pk<float>::t P2;
  static constexpr int NP = 2;
  P2 o[3][NP];
  __device__ __forceinline__ void set(const float4 &v, float l, float r) {
    const P2 d = {l, v.y}, a = {v.x, v.z}, b = {v.y, v.w}, c = {v.z, r};
    o[0][0] = d, o[0][1] = a;
    o[1][0] = a, o[1][1] = b;
    o[2][0] = b, o[2][1] = c;
  }
  static __device__ __forceinline__ float out(const P2 (&acc)[NP], int e) { return acc[e % 2][e / 2]; }
};
template <> struct BoxRowOps<double> {
  typedef Pk<double>::t P2;
  static constexpr int NP = 1;
  P2 o[3][NP];
  __device__ __forceinline__ void set(const double2 &v, double l, double r) {
    o[0][0] = P2{l, v.x};
    o[1][0] = P2{v.x, v.y};
    o[2][0] = P2{v.y, r};
  }
  static __device__ __forceinline__ double out(const P2 (&acc)[NP], int e) { return acc[0][e]; }
};

// 2.5D z-march for the aligned vector layout with carried accumulators. Lane = one 16-B x chunk of TY rows; block = NW
// waves stacked in y over one column of 64 chunks. Every block marches upwards in z (the sum takes dz = -1 first, so
// StencilTune::alternateZ is ignored) over the planes zs - 1 .. ze of its chunk [zs, ze). Each plane is held for one
// step only: its nine terms per output cell finish out(z - 1) (dz = +1), continue out(z) (dz = 0) and start out(z + 1)
// (dz = -1, the first of them a product alone), so three partial sums per output cell stay in flight and every sum
// still runs dz slowest, dy, dx fastest. The lane's own rows of a plane are loaded from memory one step ahead; the
// plane is published to LDS once (the block's rows plus one halo row above and below, loaded by the first two waves
// one step ahead), double-buffered by step parity with one barrier per step, and the lane reads the row above and
// below its own from there. x neighbours come from the adjacent lanes (DPP wave shifts); only the wave-edge lanes load
// the one cell beyond the wave from memory, one step ahead. fp32 sums are packed pairs (BoxRowOps).
// Not taken: a register ring of the three planes x (TY + 2) rows with their x neighbour cells. It marches both ways,
// but the fp32 instance needed 178 VGPRs (one block per CU), a ring shift and per-term operand copies every step:
// 400 us per 512^3 fp32 sweep, 857 us fp64 (profiles/box/bench_stencil_box_ring.csv).
template <typename T, int TY, int NW, bool NT>
__global__ __launch_bounds__(64 * NW) void stencil_box_kernel(BoxArgs<T> a) {
  using VT = typename Vec16<T>::type;
  using RO = BoxRowOps<T>;
  using P2 = typename RO::P2;
  constexpr int V = Vec16<T>::N;
  constexpr int NP = RO::NP;
  constexpr int ROWS = NW * TY + 2; // LDS row r holds raw y = yblk - 1 + r
  constexpr int NR = TY + 2;        // row j of a lane holds raw y = ybase - 1 + j
  static_assert(NW >= 2, "one wave per halo row");
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

  const bool edgeL = lane == 0;
  const bool edgeR = lane == 63 || c + 1 >= a.nchunks;
  const bool fullX = xb >= a.lox && xb + V <= a.hix;
  // halo row of the block this wave loads (waves 0 and 1): the row above, the row below
  const bool hwave = w < 2;
  const int hy = w == 0 ? yblk - 1 : yblk + NW * TY;
  const int hrow = w == 0 ? 0 : NW * TY + 1;

  // rows past the allocation's last row and planes past its last plane are clamped: those values are never used
  auto rowp = [&](int y, int z) -> const T * {
    y = min(y, a.rawYm1);
    z = min(z, a.rawZm1);
    return a.src + int64_t(z) * a.pxy + int64_t(y) * a.px + xb;
  };
  auto ld = [&](const T *p) -> VT { return *reinterpret_cast<const VT *>(p); };

  VT inc[TY], ninc[TY];             // own rows of this step's / the next step's plane
  T eL[NR], eR[NR], nL[NR], nR[NR]; // edge lanes: the cells beyond the wave of that plane's rows
  VT haloC = VT(), haloN = VT();
  P2 accA[TY][NP], accB[TY][NP];    // out(z - 1) with dz = -1, 0 summed; out(z) with dz = -1 summed
#pragma unroll
  for (int i = 0; i < TY; ++i)
#pragma unroll
    for (int q = 0; q < NP; ++q) accA[i][q] = accB[i][q] = P2{T(0), T(0)};

#pragma unroll
  for (int i = 0; i < TY; ++i) inc[i] = ld(rowp(ybase + i, zs - 1));
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const T *p = rowp(ybase - 1 + j, zs - 1);
    eL[j] = edgeL ? p[-1] : T(0);
    eR[j] = edgeR ? p[V] : T(0);
  }
  if (hwave) haloC = ld(rowp(hy, zs - 1));

  int buf = 0;
  for (int z = zs - 1; z <= ze; ++z) {
    // one step ahead: the own rows, edge cells and halo row of the next plane
#pragma unroll
    for (int i = 0; i < TY; ++i) ninc[i] = ld(rowp(ybase + i, z + 1));
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const T *p = rowp(ybase - 1 + j, z + 1);
      nL[j] = edgeL ? p[-1] : T(0);
      nR[j] = edgeR ? p[V] : T(0);
    }
    if (hwave) haloN = ld(rowp(hy, z + 1));

    // publish this plane, then take the row above and the row below the lane's own back
#pragma unroll
    for (int i = 0; i < TY; ++i) lds[buf][1 + w * TY + i][lane] = inc[i];
    if (hwave) lds[buf][hrow][lane] = haloC;
    __syncthreads();
    RO row[NR];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      const VT v = (j >= 1 && j <= TY) ? inc[j >= 1 && j <= TY ? j - 1 : 0] : lds[buf][w * TY + j][lane];
      const T sl = from_prev_lane<T>(vget<T>(v, V - 1));
      const T sr = from_next_lane<T>(vget<T>(v, 0));
      row[j].set(v, edgeL ? eL[j] : sl, edgeR ? eR[j] : sr);
    }

    // the nine terms of one dz over the lane's TY x NP independent sums: the products of a (dy, dx) first, then the
    // sums. Below: kz = 2, the dz = +1 terms, finishes out(z - 1); kz = 1 continues out(z); kz = 0 starts out(z + 1)
    auto terms = [&](int kz, P2 (&acc)[TY][NP], bool start) {
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const T wt = a.bw.w[kz][ky][kx];
          const P2 w2 = {wt, wt};
          P2 t[TY][NP];
#pragma unroll
          for (int i = 0; i < TY; ++i)
#pragma unroll
            for (int q = 0; q < NP; ++q) t[i][q] = w2 * row[i + ky].o[kx][q];
#pragma unroll
          for (int i = 0; i < TY; ++i)
#pragma unroll
            for (int q = 0; q < NP; ++q) acc[i][q] = (start && ky == 0 && kx == 0) ? t[i][q] : acc[i][q] + t[i][q];
        }
    };
    if (z > zs) {
      terms(2, accA, false);
#pragma unroll
      for (int i = 0; i < TY; ++i) {
        const int y = ybase + i;
        if (cvalid && y < a.hiy) {
          T *dp = a.dst + int64_t(z - 1) * a.pxy + int64_t(y) * a.px + xb;
          if (fullX) {
            using NV = typename Vec16<T>::native;
            NV o;
#pragma unroll
            for (int e = 0; e < V; ++e) o[e] = RO::out(accA[i], e);
            if (NT)
              __builtin_nontemporal_store(o, reinterpret_cast<NV *>(dp));
            else
              *reinterpret_cast<NV *>(dp) = o;
          } else {
#pragma unroll
            for (int e = 0; e < V; ++e)
              if (xb + e >= a.lox && xb + e < a.hix) dp[e] = RO::out(accA[i], e);
          }
        }
      }
    }
    if (z >= zs && z < ze) {
#pragma unroll
      for (int i = 0; i < TY; ++i)
#pragma unroll
        for (int q = 0; q < NP; ++q) accA[i][q] = accB[i][q];
      terms(1, accA, false);
    }
    if (z + 1 < ze) terms(0, accB, true);

#pragma unroll
    for (int j = 0; j < NR; ++j) {
      eL[j] = nL[j];
      eR[j] = nR[j];
    }
#pragma unroll
    for (int i = 0; i < TY; ++i) inc[i] = ninc[i];
    haloC = haloN;
    buf ^= 1;
  }
}

// one thread per cell: every layout or region the fast path refuses
template <typename T> __global__ __launch_bounds__(256) void stencil_box_generic_kernel(BoxArgs<T> a) {
  const int64_t nx = a.hix - a.lox, ny = a.hiy - a.loy, nz = a.hiz - a.loz;
  const int64_t total = nx * ny * nz;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < total; i += int64_t(gridDim.x) * blockDim.x) {
    const int x = a.lox + int(i % nx), y = a.loy + int((i / nx) % ny), z = a.loz + int(i / (nx * ny));
    const int64_t o = int64_t(z) * a.pxy + int64_t(y) * a.px + x;
    a.dst[o] = box_cell<T>(a.bw, a.src + o, a.px, a.pxy);
  }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
constexpr int kBoxTY = 2, kBoxNW = 8, kBoxMinZc = 16, kBoxMaxBlocksPerCU = 2;

template <typename T> static void box_host(const BoxArgs<T> &a) {
  for (int z = a.loz; z < a.hiz; ++z)
    for (int y = a.loy; y < a.hiy; ++y)
      for (int x = a.lox; x < a.hix; ++x) {
        const int64_t o = int64_t(z) * a.pxy + int64_t(y) * a.px + x;
        a.dst[o] = box_cell<T>(a.bw, a.src + o, a.px, a.pxy);
      }
}

// kernel arguments and the path apply takes for them; the fast path's grid is filled in (device sub-domains)
template <typename T>
static BoxArgs<T> box_plan(const LocalDomain &dom, int64_t qi, const Rect3 &region, const BoxWeights &wts,
                           const StencilTune &tune, BoxLaunchInfo *info) {
  BoxArgs<T> a{};
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
  for (int k = 0; k < 3; ++k)
    for (int j = 0; j < 3; ++j)
      for (int i = 0; i < 3; ++i) a.bw.w[k][j][i] = T(wts.w[k][j][i]);
  *info = BoxLaunchInfo();
  if (dom.backend() == Backend::Host) return a;
  info->path = 1;
  constexpr int V = Vec16<T>::N;
  const int rxm = int(dom.radius().x(-1));
  // chunk grid anchored at the 16-B aligned interior start
  const int off = ((a.lox - rxm) % V + V) % V;
  a.x0 = a.lox - off;
  a.nchunks = (a.hix - a.x0 + V - 1) / V;
  const bool alignedLayout = aligned_vector_layout(dom, qi, a.x0);
  // the last chunk's vector load and the cell right of it stay below the row's read limit; the cell left of chunk 0
  // is a raw cell of the row (x0 >= the -x radius >= 1)
  const bool fits = a.x0 + int64_t(a.nchunks) * V + 1 <= dom.row_limit(qi) && a.x0 >= 1;
  if (!(alignedLayout && fits)) return a;
  info->path = 2;
  const int ny = a.hiy - a.loy, nz = a.hiz - a.loz;
  a.gx = (a.nchunks + 63) / 64;
  a.gy = (ny + kBoxNW * kBoxTY - 1) / (kBoxNW * kBoxTY);
  int zc = tune.zchunk;
  if (zc <= 0) {
    // one round of resident blocks (occupancy, at most two per CU, x CUs), z chunks of at least kBoxMinZc planes
    // (each re-reads 2 planes)
    dom.set_device();
    const void *kern = tune.nontemporal ? (const void *)stencil_box_kernel<T, kBoxTY, kBoxNW, true>
                                        : (const void *)stencil_box_kernel<T, kBoxTY, kBoxNW, false>;
    const int64_t cols = int64_t(a.gx) * a.gy;
    const int64_t resident = std::min(resident_blocks(kern, 64 * kBoxNW, 2),
                                      int64_t(kBoxMaxBlocksPerCU) * device_cus(dom.gpu()));
    const int64_t nzc = std::max<int64_t>(1, resident / cols);
    zc = int(std::max<int64_t>(kBoxMinZc, (nz + nzc - 1) / nzc));
  }
  a.zc = zc;
  a.gz = (nz + zc - 1) / zc;
  info->zchunk = zc;
  info->zchunks = a.gz;
  info->blocks = int64_t(a.gx) * a.gy * a.gz;
  return a;
}

template <typename T>
static void box_apply_t(const LocalDomain &dom, int64_t qi, const Rect3 &region, const BoxWeights &wts,
                        hipStream_t stream, const StencilTune &tune) {
  BoxLaunchInfo info;
  const BoxArgs<T> a = box_plan<T>(dom, qi, region, wts, tune, &info);
  if (info.path == 0) {
    box_host<T>(a);
    return;
  }
  dom.set_device();
  if (info.path == 2) {
    const dim3 block(64, kBoxNW);
    if (tune.nontemporal)
      hipLaunchKernelGGL((stencil_box_kernel<T, kBoxTY, kBoxNW, true>), dim3(uint32_t(info.blocks)), block, 0, stream, a);
    else
      hipLaunchKernelGGL((stencil_box_kernel<T, kBoxTY, kBoxNW, false>), dim3(uint32_t(info.blocks)), block, 0, stream, a);
  } else {
    const int64_t total = int64_t(a.hix - a.lox) * (a.hiy - a.loy) * (a.hiz - a.loz);
    const int blocks = int(std::min<int64_t>((total + 255) / 256, 4096));
    hipLaunchKernelGGL((stencil_box_generic_kernel<T>), dim3(blocks), dim3(256), 0, stream, a);
  }
  HIP_CHECK(hipGetLastError());
}

static bool box_fp(const LocalDomain &dom, int64_t qi, bool *f64) {
  const DType dt = dom.dtype(qi);
  const int64_t es = dom.elem_size(qi);
  *f64 = dt == DType::F64 || (dt == DType::Bytes && es == 8);
  return *f64 || dt == DType::F32 || (dt == DType::Bytes && es == 4);
}

// the smallest of the 26 direction radii
static int64_t box_min_radius(const LocalDomain &dom) {
  const Radius &rd = dom.radius();
  int64_t m = rd.x(-1);
  for (int z = -1; z <= 1; ++z)
    for (int y = -1; y <= 1; ++y)
      for (int x = -1; x <= 1; ++x)
        if (x != 0 || y != 0 || z != 0) m = std::min(m, rd.dir(x, y, z));
  return m;
}

bool stencil_box_supported(const LocalDomain &dom, int64_t qi) {
  bool f64 = false;
  if (qi < 0 || qi >= dom.num_data() || !box_fp(dom, qi, &f64)) return false;
  return box_min_radius(dom) >= 1;
}

// the refusals shared by apply and launch_info; false: nothing to do (empty region)
static bool box_check(const LocalDomain &dom, int64_t qi, const Rect3 &region, const StencilTune &tune, bool *f64) {
  STENCIL_REQUIRE(qi >= 0 && qi < dom.num_data() && box_fp(dom, qi, f64), "box stencils take fp32 / fp64 quantities");
  STENCIL_REQUIRE(box_min_radius(dom) >= 1, "box stencils need face, edge and corner radii >= 1 (smallest of the 26: "
                                                << box_min_radius(dom) << ")");
  STENCIL_REQUIRE(tune.wrap == 0, "box stencils read halos (no in-kernel wrap)");
  require_region_in_compute(dom, region);
  return !region.empty();
}

void stencil_box_apply(const LocalDomain &dom, int64_t qi, const Rect3 &region, const BoxWeights &w, hipStream_t stream,
                       const StencilTune &tune) {
  bool f64 = false;
  if (!box_check(dom, qi, region, tune, &f64)) return;
  if (!f64)
    box_apply_t<float>(dom, qi, region, w, stream, tune);
  else
    box_apply_t<double>(dom, qi, region, w, stream, tune);
}

BoxLaunchInfo stencil_box_launch_info(const LocalDomain &dom, int64_t qi, const Rect3 &region, const BoxWeights &w,
                                      const StencilTune &tune) {
  BoxLaunchInfo info;
  bool f64 = false;
  if (!box_check(dom, qi, region, tune, &f64)) {
    info.path = -1;
    return info;
  }
  if (!f64)
    box_plan<float>(dom, qi, region, w, tune, &info);
  else
    box_plan<double>(dom, qi, region, w, tune, &info);
  return info;
}

} // namespace stencil
