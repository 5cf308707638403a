// Grid transfer for gfx950: restriction (8-cell mean) and trilinear prolongation between a fine sub-domain and its
// factor-2 coarse image. See stencil/kernels/grid_transfer.hpp for the arithmetic; the chunk kernels, the
// one-thread-per-cell kernels and the host loops evaluate the same expressions in the same order, so all three are
// bitwise equal to stencil2_amd.ops.restrict_reference / prolong_reference.
//
// Coordinates below are local: cell 0 is the first cell of the sub-domain's compute region, so fine local i = 2 I + p
// for coarse local I (the fine origin is twice the coarse origin), and raw = local + the -side face radius.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "stencil_common.hpp"
#include "stencil/kernels/grid_transfer.hpp"
#include "stencil/rt/hip_check.hpp"

// no FMA contraction anywhere below, device or host (hipcc contracts by default)
#pragma clang fp contract(off)

namespace stencil {

constexpr int kXferThreads = 256, kXferWaves = kXferThreads / 64;
constexpr int kProlongZChunk = 8;    // coarse planes a wave marches on the host path's launch info (no march there)
constexpr int kProlongMinZChunk = 4; // the shortest march the launch chooses (2 more planes are loaded as warm-up)

template <typename T> struct XferArgs {
  T *dst;       // raw [0,0,0] of the destination buffer (coarse: restriction, fine: prolongation)
  const T *src; // ... of the source buffer (fine: restriction, coarse: prolongation)
  const T *add; // ... of the fine `add` buffer (prolongation; null: none)
  int64_t fpx, fpxy, cpx, cpxy; // fine and coarse pitches
  int rfx, rfy, rfz, rcx, rcy, rcz; // raw coordinates of local cell 0, fine and coarse
  int lox, loy, loz, hix, hiy, hiz; // region, local coordinates of the destination grid
  // chunk kernels. Restriction: coarse chunk c covers coarse local x [c V, c V + V), fine local x [2 c V, 2 c V + 2 V).
  // Prolongation: fine chunk c covers fine local x [c V, c V + V), coarse local x [c V / 2, c V / 2 + V / 2)
  int c0, nchunks; // first chunk and the chunks that cover the region
  int jlo, nj;     // coarse rows that cover the region
  int klo, nk;     // coarse planes that cover the region
  int zc;          // prolongation: coarse planes per wave item
  int npass;       // prolongation: wave items per row (64 chunks each)
  int climit;      // prolongation: coarse raw x (exclusive) a row may be read to
  int64_t nitems;  // wave items
  int64_t count;   // cells of the region
};

template <typename T> __host__ __device__ __forceinline__ T lerp31(T nearv, T farv) {
  const T p = T(0.75) * nearv;
  const T q = T(0.25) * farv;
  return p + q;
}

// f: the fine cell (2K, 2J, 2I)
template <typename T> __host__ __device__ __forceinline__ T restrict_cell(const T *f, int64_t px, int64_t pxy) {
  const T sx00 = f[0] + f[1];
  const T sx01 = f[px] + f[px + 1];
  const T sx10 = f[pxy] + f[pxy + 1];
  const T sx11 = f[pxy + px] + f[pxy + px + 1];
  const T sy0 = sx00 + sx01;
  const T sy1 = sx10 + sx11;
  return T(0.125) * (sy0 + sy1);
}

// the interpolated value at fine local (i, j, k)
template <typename T> __host__ __device__ __forceinline__ T prolong_cell(const XferArgs<T> &a, int i, int j, int k) {
  const int64_t dI = (i & 1) ? 1 : -1;
  const int64_t dJ = (j & 1) ? a.cpx : -a.cpx;
  const int64_t dK = (k & 1) ? a.cpxy : -a.cpxy;
  const T *c = a.src + int64_t((k >> 1) + a.rcz) * a.cpxy + int64_t((j >> 1) + a.rcy) * a.cpx + ((i >> 1) + a.rcx);
  const T t00 = lerp31(c[0], c[dI]);
  const T t01 = lerp31(c[dJ], c[dJ + dI]);
  const T t10 = lerp31(c[dK], c[dK + dI]);
  const T t11 = lerp31(c[dK + dJ], c[dK + dJ + dI]);
  const T ty0 = lerp31(t00, t01);
  const T ty1 = lerp31(t10, t11);
  return lerp31(ty0, ty1);
}

template <typename T> __device__ __forceinline__ typename Vec16<T>::type vmake(const T *s);
template <> __device__ __forceinline__ float4 vmake<float>(const float *s) { return make_float4(s[0], s[1], s[2], s[3]); }
template <> __device__ __forceinline__ double2 vmake<double>(const double *s) { return make_double2(s[0], s[1]); }

// ---------------------------------------------------------------------------------------------------------
// restriction
// ---------------------------------------------------------------------------------------------------------
// The aligned vector layout: wave gw of the grid takes coarse (row, plane) items gw, gw + GW, ..., its lanes the row's
// 16-B coarse chunks lane, lane + 64, ... A lane loads the two fine chunks under its coarse chunk from each of the 4
// fine rows (8 loads in flight), and stores one coarse chunk. Chunks that reach outside [lox, hix) are loaded whole
// (inside the fine rows' read limit) and stored cell by cell for the cells inside only.
template <typename T> __global__ __launch_bounds__(kXferThreads) void grid_restrict_chunks_kernel(XferArgs<T> a) {
  using VT = typename Vec16<T>::type;
  constexpr int V = Vec16<T>::N;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gw = int64_t(blockIdx.x) * kXferWaves + wave, GW = int64_t(gridDim.x) * kXferWaves;
  for (int64_t r = gw; r < a.nitems; r += GW) {
    const int J = a.jlo + int(r % a.nj), K = a.klo + int(r / a.nj);
    const T *f = a.src + int64_t(2 * K + a.rfz) * a.fpxy + int64_t(2 * J + a.rfy) * a.fpx + a.rfx;
    T *d = a.dst + int64_t(K + a.rcz) * a.cpxy + int64_t(J + a.rcy) * a.cpx + a.rcx;
    for (int c = a.c0 + lane; c < a.c0 + a.nchunks; c += 64) {
      VT v[2][2][2];
#pragma unroll
      for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            v[dz][dy][h] = *reinterpret_cast<const VT *>(f + dz * a.fpxy + dy * a.fpx + int64_t(2 * c + h) * V);
      T o[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const int h = (2 * e) / V, i = (2 * e) % V;
        const T sx00 = vget<T>(v[0][0][h], i) + vget<T>(v[0][0][h], i + 1);
        const T sx01 = vget<T>(v[0][1][h], i) + vget<T>(v[0][1][h], i + 1);
        const T sx10 = vget<T>(v[1][0][h], i) + vget<T>(v[1][0][h], i + 1);
        const T sx11 = vget<T>(v[1][1][h], i) + vget<T>(v[1][1][h], i + 1);
        const T sy0 = sx00 + sx01;
        const T sy1 = sx10 + sx11;
        o[e] = T(0.125) * (sy0 + sy1);
      }
      const int xb = c * V;
      if (xb >= a.lox && xb + V <= a.hix) {
        *reinterpret_cast<VT *>(d + xb) = vmake<T>(o);
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e)
          if (xb + e >= a.lox && xb + e < a.hix) d[xb + e] = o[e];
      }
    }
  }
}

// one thread per coarse cell, grid-strided in cell order: every layout the chunk kernel refuses
template <typename T> __global__ __launch_bounds__(kXferThreads) void grid_restrict_generic_kernel(XferArgs<T> a) {
  const int64_t nx = a.hix - a.lox, ny = a.hiy - a.loy;
  for (int64_t n = int64_t(blockIdx.x) * kXferThreads + threadIdx.x; n < a.count; n += int64_t(gridDim.x) * kXferThreads) {
    const int I = a.lox + int(n % nx), J = a.loy + int((n / nx) % ny), K = a.loz + int(n / (nx * ny));
    const T *f = a.src + int64_t(2 * K + a.rfz) * a.fpxy + int64_t(2 * J + a.rfy) * a.fpx + (2 * I + a.rfx);
    a.dst[int64_t(K + a.rcz) * a.cpxy + int64_t(J + a.rcy) * a.cpx + (I + a.rcx)] = restrict_cell(f, a.fpx, a.fpxy);
  }
}

template <typename T> static void restrict_host(const XferArgs<T> &a) {
  for (int K = a.loz; K < a.hiz; ++K)
    for (int J = a.loy; J < a.hiy; ++J)
      for (int I = a.lox; I < a.hix; ++I) {
        const T *f = a.src + int64_t(2 * K + a.rfz) * a.fpxy + int64_t(2 * J + a.rfy) * a.fpx + (2 * I + a.rfx);
        a.dst[int64_t(K + a.rcz) * a.cpxy + int64_t(J + a.rcy) * a.cpx + (I + a.rcx)] = restrict_cell(f, a.fpx, a.fpxy);
      }
}

// ---------------------------------------------------------------------------------------------------------
// prolongation
// ---------------------------------------------------------------------------------------------------------
// A lane of the chunk kernel owns one 16-B fine chunk per fine row, i.e. the W = V / 2 coarse cells under it (8 B of
// the coarse row), so every fine access of a wave is one contiguous run of 64 x 16 B. (One 16-B coarse chunk per lane,
// the first form of this kernel, stores its two fine chunks at a 32-B lane stride, half of every 64-B block per
// instruction: 2.5 TB/s on 512^3 fp32 where this form was measured, BASELINE.md "Grid transfer".)
template <typename T> struct CoarseHalf;
template <> struct CoarseHalf<float> {
  static constexpr int W = 2;
  static __device__ __forceinline__ void load(const float *p, float *c) {
    const float2 v = *reinterpret_cast<const float2 *>(p);
    c[0] = v.x;
    c[1] = v.y;
  }
};
template <> struct CoarseHalf<double> {
  static constexpr int W = 1;
  static __device__ __forceinline__ void load(const double *p, double *c) { c[0] = p[0]; }
};

// The lane's loads of one coarse plane: c[r][1 .. W] its W cells of coarse rows J - 1, J, J + 1 (row: those of row J),
// c[r][0] the cell left of them and c[r][W + 1] the cell right of them where this lane loads them itself (lane 0;
// lane 63 and the lane of the row's last chunk, inside the row's read limit: beyond it no cell of the region needs
// it). Inactive lanes load nothing and hold zeros.
template <typename T>
__device__ __forceinline__ void prolong_load(const XferArgs<T> &a, const T *row, bool active, bool loadLeft,
                                             bool loadRight, T (&c)[3][CoarseHalf<T>::W + 2]) {
  constexpr int W = CoarseHalf<T>::W;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const T *p = row + int64_t(r - 1) * a.cpx;
#pragma unroll
    for (int e = 0; e < W + 2; ++e) c[r][e] = T(0);
    if (active) CoarseHalf<T>::load(p, &c[r][1]);
    if (active && loadLeft) c[r][0] = p[-1];
    if (active && loadRight) c[r][W + 1] = p[W];
  }
}

// The x- and y-interpolated rows of the loaded plane under the lane's fine chunk: ty[0] the fine row 2 J, ty[1] the
// fine row 2 J + 1, V fine cells each. The cell left of the lane's cells comes from the lane below and the cell right
// of them from the lane above, unless the lane loaded it. Every lane of the wave calls this (the shuffles).
template <typename T>
__device__ __forceinline__ void prolong_rows(const T (&c)[3][CoarseHalf<T>::W + 2], bool ownLeft, bool ownRight,
                                             T (&ty)[2][Vec16<T>::N]) {
  constexpr int V = Vec16<T>::N, W = CoarseHalf<T>::W;
  T tx[3][V];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    T v[W + 2];
    const T left = shfl_up1<T>(c[r][W]), right = shfl_down1<T>(c[r][1]);
    v[0] = ownLeft ? c[r][0] : left;
    v[W + 1] = ownRight ? c[r][W + 1] : right;
#pragma unroll
    for (int e = 0; e < W; ++e) v[e + 1] = c[r][e + 1];
#pragma unroll
    for (int e = 0; e < W; ++e) {
      tx[r][2 * e] = lerp31(v[e + 1], v[e]);
      tx[r][2 * e + 1] = lerp31(v[e + 1], v[e + 2]);
    }
  }
#pragma unroll
  for (int i = 0; i < V; ++i) {
    ty[0][i] = lerp31(tx[1][i], tx[0][i]);
    ty[1][i] = lerp31(tx[1][i], tx[2][i]);
  }
}

// The aligned vector layout: a wave item is (64 fine chunks of x, coarse row J, z chunk), x fastest; the wave's lanes
// own the item's fine chunks of the fine rows 2 J, 2 J + 1 and march the z chunk's coarse planes upwards with the interpolated
// rows of planes K - 1, K, K + 1 in registers (every lane loads rows J - 1, J and J + 1 itself: a coarse cell is
// requested three times, by the waves of three rows, and the repeats are left to the caches; the coarse traffic
// that reaches HBM has not been measured). Per coarse plane a lane writes fine planes 2 K, 2 K + 1 x fine rows
// 2 J, 2 J + 1, one 16-B chunk each; with ADD it loads those chunks of `add` first, all four loads before the first
// store, so add may be the buffer it stores to. The coarse loads run one plane ahead: a step issues the loads of plane
// K + 2 and of its `add` chunks together and interpolates plane K + 1, loaded a step earlier, while they are in
// flight (one memory round trip per step instead of two). Fine rows and planes outside the region are skipped
// (wave-uniform) and chunks that straddle [lox, hix) are stored cell by cell.
template <typename T, bool ADD> __global__ __launch_bounds__(kXferThreads) void grid_prolong_chunks_kernel(XferArgs<T> a) {
  using VT = typename Vec16<T>::type;
  constexpr int V = Vec16<T>::N, W = CoarseHalf<T>::W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t gw = int64_t(blockIdx.x) * kXferWaves + wave, GW = int64_t(gridDim.x) * kXferWaves;
  for (int64_t it = gw; it < a.nitems; it += GW) {
    const int cb = int(it % a.npass) * 64;
    const int J = a.jlo + int((it / a.npass) % a.nj);
    const int k0 = a.klo + int(it / (int64_t(a.npass) * a.nj)) * a.zc, k1 = min(k0 + a.zc, a.klo + a.nk);
    {
      const bool active = cb + lane < a.nchunks;
      const int c = a.c0 + (active ? cb + lane : 0); // fine chunk: fine local x [c V, c V + V), coarse [c W, c W + W)
      const bool loadLeft = lane == 0;
      const bool loadRight = (lane == 63 || cb + lane == a.nchunks - 1) && a.rcx + (c + 1) * W < a.climit;
      const bool ownLeft = active && loadLeft, ownRight = active && loadRight;
      // row: the lane's cells of coarse row J in plane k0 - 1
      const T *row = a.src + int64_t(k0 - 1 + a.rcz) * a.cpxy + int64_t(J + a.rcy) * a.cpx + (a.rcx + c * W);
      T lo[2][V], mid[2][V], hi[2][V];
      T cur[3][W + 2], nxt[3][W + 2];
      prolong_load<T>(a, row, active, loadLeft, loadRight, cur);
      prolong_load<T>(a, row + a.cpxy, active, loadLeft, loadRight, nxt);
      prolong_rows<T>(cur, ownLeft, ownRight, lo);
      prolong_load<T>(a, row + 2 * a.cpxy, active, loadLeft, loadRight, cur);
      prolong_rows<T>(nxt, ownLeft, ownRight, mid);
      for (int K = k0; K < k1; ++K) { // cur: plane K + 1
        if (K + 1 < k1) prolong_load<T>(a, row + int64_t(K + 3 - k0) * a.cpxy, active, loadLeft, loadRight, nxt);
        T *d = a.dst + int64_t(2 * K + a.rfz) * a.fpxy + int64_t(2 * J + a.rfy) * a.fpx + (a.rfx + c * V);
        const T *ad = ADD ? a.add + (d - a.dst) : nullptr;
        bool on[2][2]; // [plane][row] inside the region
        VT av[2][2];
#pragma unroll
        for (int pz = 0; pz < 2; ++pz)
#pragma unroll
          for (int py = 0; py < 2; ++py) {
            on[pz][py] = 2 * K + pz >= a.loz && 2 * K + pz < a.hiz && 2 * J + py >= a.loy && 2 * J + py < a.hiy;
            if (ADD && active && on[pz][py]) av[pz][py] = *reinterpret_cast<const VT *>(ad + pz * a.fpxy + py * a.fpx);
          }
        prolong_rows<T>(cur, ownLeft, ownRight, hi);
        if (active) {
          const int xb = c * V;
          const bool full = xb >= a.lox && xb + V <= a.hix;
#pragma unroll
          for (int pz = 0; pz < 2; ++pz)
#pragma unroll
            for (int py = 0; py < 2; ++py) {
              if (!on[pz][py]) continue;
              T o[V];
#pragma unroll
              for (int e = 0; e < V; ++e) {
                const T v = lerp31(mid[py][e], pz ? hi[py][e] : lo[py][e]);
                o[e] = ADD ? vget<T>(av[pz][py], e) + v : v;
              }
              T *dp = d + pz * a.fpxy + py * a.fpx;
              if (full) {
                *reinterpret_cast<VT *>(dp) = vmake<T>(o);
              } else {
#pragma unroll
                for (int e = 0; e < V; ++e)
                  if (xb + e >= a.lox && xb + e < a.hix) dp[e] = o[e];
              }
            }
        }
#pragma unroll
        for (int py = 0; py < 2; ++py)
#pragma unroll
          for (int i = 0; i < V; ++i) {
            lo[py][i] = mid[py][i];
            mid[py][i] = hi[py][i];
          }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int e = 0; e < W + 2; ++e) cur[r][e] = nxt[r][e];
      }
    }
  }
}

// one thread per fine cell, grid-strided in cell order: every layout the chunk kernel refuses
template <typename T, bool ADD> __global__ __launch_bounds__(kXferThreads) void grid_prolong_generic_kernel(XferArgs<T> a) {
  const int64_t nx = a.hix - a.lox, ny = a.hiy - a.loy;
  for (int64_t n = int64_t(blockIdx.x) * kXferThreads + threadIdx.x; n < a.count; n += int64_t(gridDim.x) * kXferThreads) {
    const int i = a.lox + int(n % nx), j = a.loy + int((n / nx) % ny), k = a.loz + int(n / (nx * ny));
    const int64_t o = int64_t(k + a.rfz) * a.fpxy + int64_t(j + a.rfy) * a.fpx + (i + a.rfx);
    const T v = prolong_cell(a, i, j, k);
    a.dst[o] = ADD ? a.add[o] + v : v;
  }
}

template <typename T> static void prolong_host(const XferArgs<T> &a) {
  for (int k = a.loz; k < a.hiz; ++k)
    for (int j = a.loy; j < a.hiy; ++j)
      for (int i = a.lox; i < a.hix; ++i) {
        const int64_t o = int64_t(k + a.rfz) * a.fpxy + int64_t(j + a.rfy) * a.fpx + (i + a.rfx);
        const T v = prolong_cell(a, i, j, k);
        a.dst[o] = a.add ? a.add[o] + v : v;
      }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
static bool xfer_fp(const LocalDomain &dom, int64_t q, int64_t *es) {
  return q >= 0 && q < dom.num_data() && fp_quantity(dom, q, es);
}
static bool even3(const Dim3 &d) { return d.x % 2 == 0 && d.y % 2 == 0 && d.z % 2 == 0; }
static bool factor2_pair(const LocalDomain &fine, const LocalDomain &coarse) {
  return even3(fine.origin()) && even3(fine.size()) && coarse.origin() * 2 == fine.origin() &&
         coarse.size() * 2 == fine.size();
}

bool grid_transfer_supported(const LocalDomain &fine, int64_t qf, const LocalDomain &coarse, int64_t qc) {
  int64_t ef = 0, ec = 0;
  if (!fine.realized() || !coarse.realized() || !xfer_fp(fine, qf, &ef) || !xfer_fp(coarse, qc, &ec)) return false;
  return ef == ec && factor2_pair(fine, coarse) && fine.backend() == coarse.backend() &&
         (fine.backend() == Backend::Host || fine.gpu() == coarse.gpu());
}

// the refusals shared by both transfers, enqueue and launch_info; returns the element size
static int64_t xfer_check(const LocalDomain &fine, FieldRef qf, const LocalDomain &coarse, FieldRef qc) {
  STENCIL_REQUIRE(fine.realized() && coarse.realized(), "grid transfer of an unrealized domain");
  int64_t ef = 0, ec = 0;
  STENCIL_REQUIRE(xfer_fp(fine, qf.q, &ef), "grid transfer takes fp32 / fp64 quantities (fine: quantity " << qf.q << ")");
  STENCIL_REQUIRE(xfer_fp(coarse, qc.q, &ec), "grid transfer takes fp32 / fp64 quantities (coarse: quantity " << qc.q << ")");
  STENCIL_REQUIRE(ef == ec, "grid transfer operands differ in type: " << ef << "- and " << ec << "-byte elements");
  STENCIL_REQUIRE(factor2_pair(fine, coarse), "grid transfer: coarse sub-domain " << coarse.get_compute_region()
                                                  << " is not the factor-2 image of fine sub-domain "
                                                  << fine.get_compute_region() << " (even origin and size, halved)");
  STENCIL_REQUIRE(fine.backend() == coarse.backend(), "grid transfer between different backends");
  STENCIL_REQUIRE(fine.backend() == Backend::Host || fine.gpu() == coarse.gpu(),
                  "grid transfer between different devices: " << fine.gpu() << " and " << coarse.gpu());
  return ef;
}

static const void *buf(const LocalDomain &dom, FieldRef f) { return f.curr ? dom.curr_data(f.q) : dom.next_data(f.q); }

template <typename T>
static XferArgs<T> xfer_args(const LocalDomain &fine, const LocalDomain &coarse, const LocalDomain &dstDom, int64_t qf,
                             int64_t qc, const Rect3 &region) {
  XferArgs<T> a{};
  const Dim3 pf = fine.pitch(qf), pc = coarse.pitch(qc);
  a.fpx = pf.x;
  a.fpxy = pf.x * pf.y;
  a.cpx = pc.x;
  a.cpxy = pc.x * pc.y;
  a.rfx = int(fine.radius().x(-1));
  a.rfy = int(fine.radius().y(-1));
  a.rfz = int(fine.radius().z(-1));
  a.rcx = int(coarse.radius().x(-1));
  a.rcy = int(coarse.radius().y(-1));
  a.rcz = int(coarse.radius().z(-1));
  const Dim3 o = dstDom.origin();
  a.lox = int(region.lo.x - o.x);
  a.loy = int(region.lo.y - o.y);
  a.loz = int(region.lo.z - o.z);
  a.hix = int(region.hi.x - o.x);
  a.hiy = int(region.hi.y - o.y);
  a.hiz = int(region.hi.z - o.z);
  a.count = int64_t(a.hix - a.lox) * (a.hiy - a.loy) * (a.hiz - a.loz);
  return a;
}

// blocks of a launch with one wave per item: every item its own wave up to 2^20 blocks, grid-strided beyond
static int64_t item_blocks(int64_t items) {
  return std::max<int64_t>(1, std::min<int64_t>((items + kXferWaves - 1) / kXferWaves, 1 << 20));
}
static int64_t cell_blocks(const LocalDomain &dom, const void *kernel, int64_t count) {
  dom.set_device();
  const int64_t resident = resident_blocks(kernel, kXferThreads, 4);
  return std::max<int64_t>(1, std::min<int64_t>((count + kXferThreads - 1) / kXferThreads, resident));
}

// ---- restriction ----
template <typename T>
static XferArgs<T> restrict_plan(const LocalDomain &fine, FieldRef src, const LocalDomain &coarse, FieldRef dst,
                                 const Rect3 &region, TransferLaunchInfo *info) {
  XferArgs<T> a = xfer_args<T>(fine, coarse, coarse, src.q, dst.q, region);
  a.src = static_cast<const T *>(buf(fine, src));
  a.dst = static_cast<T *>(const_cast<void *>(buf(coarse, dst)));
  constexpr int V = Vec16<T>::N;
  a.c0 = a.lox / V;
  a.nchunks = (a.hix + V - 1) / V - a.c0;
  a.jlo = a.loy;
  a.nj = a.hiy - a.loy;
  a.klo = a.loz;
  a.nk = a.hiz - a.loz;
  a.nitems = int64_t(a.nj) * a.nk;
  *info = TransferLaunchInfo();
  info->items = a.nitems;
  if (coarse.backend() == Backend::Host) return a;
  info->path = 1;
  // whole fine chunks are loaded: the last one may reach past the fine row's cells, up to its read limit
  const bool ok = !fine.x_halo_align() && !coarse.x_halo_align() && aligned_vector_layout(coarse, dst.q, a.rcx) &&
                  aligned_vector_layout(fine, src.q, a.rfx) &&
                  a.rfx + int64_t(2) * (a.c0 + a.nchunks) * V <= fine.row_limit(src.q);
  if (ok) {
    info->path = 2;
    info->blocks = item_blocks(a.nitems);
  } else {
    info->blocks = cell_blocks(coarse, (const void *)grid_restrict_generic_kernel<T>, a.count);
  }
  return a;
}

template <typename T>
static void restrict_enqueue_t(const LocalDomain &fine, FieldRef src, const LocalDomain &coarse, FieldRef dst,
                               const Rect3 &region, hipStream_t stream) {
  TransferLaunchInfo info;
  const XferArgs<T> a = restrict_plan<T>(fine, src, coarse, dst, region, &info);
  if (info.path == 0) {
    restrict_host<T>(a);
    return;
  }
  coarse.set_device();
  const dim3 grid(uint32_t(info.blocks)), block(kXferThreads);
  if (info.path == 2)
    hipLaunchKernelGGL(grid_restrict_chunks_kernel<T>, grid, block, 0, stream, a);
  else
    hipLaunchKernelGGL(grid_restrict_generic_kernel<T>, grid, block, 0, stream, a);
  HIP_CHECK(hipGetLastError());
}

static int64_t restrict_check(const LocalDomain &fine, FieldRef src, const LocalDomain &coarse, FieldRef dst,
                              const Rect3 &region) {
  const int64_t es = xfer_check(fine, src, coarse, dst);
  require_region_in_compute(coarse, region, "restriction region");
  return es;
}

void grid_restrict_enqueue(const LocalDomain &fine, FieldRef src, const LocalDomain &coarse, FieldRef dst,
                           const Rect3 &coarseRegion, hipStream_t stream) {
  const int64_t es = restrict_check(fine, src, coarse, dst, coarseRegion);
  if (coarseRegion.empty()) return;
  if (es == 4)
    restrict_enqueue_t<float>(fine, src, coarse, dst, coarseRegion, stream);
  else
    restrict_enqueue_t<double>(fine, src, coarse, dst, coarseRegion, stream);
}

TransferLaunchInfo grid_restrict_launch_info(const LocalDomain &fine, FieldRef src, const LocalDomain &coarse,
                                             FieldRef dst, const Rect3 &coarseRegion) {
  const int64_t es = restrict_check(fine, src, coarse, dst, coarseRegion);
  TransferLaunchInfo info;
  if (coarseRegion.empty()) {
    info.path = -1;
    return info;
  }
  if (es == 4)
    restrict_plan<float>(fine, src, coarse, dst, coarseRegion, &info);
  else
    restrict_plan<double>(fine, src, coarse, dst, coarseRegion, &info);
  return info;
}

// ---- prolongation ----
template <typename T>
static XferArgs<T> prolong_plan(const LocalDomain &coarse, FieldRef src, const LocalDomain &fine, FieldRef dst,
                                FieldRef add, const Rect3 &region, int zchunk, TransferLaunchInfo *info) {
  XferArgs<T> a = xfer_args<T>(fine, coarse, fine, dst.q, src.q, region);
  a.src = static_cast<const T *>(buf(coarse, src));
  a.dst = static_cast<T *>(const_cast<void *>(buf(fine, dst)));
  a.add = add.q >= 0 ? static_cast<const T *>(buf(fine, add)) : nullptr;
  constexpr int V = Vec16<T>::N;
  constexpr int W = V / 2;
  // the fine chunks that meet the region, and the coarse rows and planes whose fine cells do (local coordinates are
  // >= 0: the shifts are floors)
  a.c0 = a.lox / V;
  a.nchunks = (a.hix + V - 1) / V - a.c0;
  a.jlo = a.loy >> 1;
  a.nj = ((a.hiy - 1) >> 1) + 1 - a.jlo;
  a.klo = a.loz >> 1;
  a.nk = ((a.hiz - 1) >> 1) + 1 - a.klo;
  a.npass = (a.nchunks + 63) / 64;
  a.zc = std::min(zchunk > 0 ? zchunk : kProlongZChunk, a.nk);
  a.climit = int(coarse.row_limit(src.q));
  auto count_items = [&] { a.nitems = int64_t(a.npass) * a.nj * ((a.nk + a.zc - 1) / a.zc); };
  count_items();
  *info = TransferLaunchInfo();
  info->items = a.nitems;
  if (fine.backend() == Backend::Host) return a;
  info->path = 1;
  // a lane loads the W coarse cells under its fine chunk, and with `add` the whole fine chunk: the last ones may
  // reach past the rows' cells, up to their read limits
  bool ok = !fine.x_halo_align() && !coarse.x_halo_align() && aligned_vector_layout(coarse, src.q, a.rcx) &&
            aligned_vector_layout(fine, dst.q, a.rfx) && a.rcx + int64_t(a.c0 + a.nchunks) * W <= coarse.row_limit(src.q);
  if (add.q >= 0)
    ok = ok && aligned_vector_layout(fine, add.q, a.rfx) && a.rfx + int64_t(a.c0 + a.nchunks) * V <= fine.row_limit(add.q);
  if (ok && zchunk == 0) {
    // the z chunk that balances the two warm-up planes of every march against a partly empty last round of waves
    fine.set_device();
    const void *k = add.q >= 0 ? (const void *)grid_prolong_chunks_kernel<T, true> : (const void *)grid_prolong_chunks_kernel<T, false>;
    const int64_t waves = resident_blocks(k, kXferThreads, 4) * kXferWaves;
    a.zc = pick_zchunk(int64_t(a.npass) * a.nj, a.nk, waves, 2, kProlongMinZChunk);
    count_items();
    info->items = a.nitems;
  }
  if (ok) {
    info->path = 2;
    info->zchunk = a.zc;
    info->blocks = item_blocks(a.nitems);
  } else {
    info->blocks = cell_blocks(fine, add.q >= 0 ? (const void *)grid_prolong_generic_kernel<T, true>
                                                : (const void *)grid_prolong_generic_kernel<T, false>, a.count);
  }
  return a;
}

template <typename T>
static void prolong_enqueue_t(const LocalDomain &coarse, FieldRef src, const LocalDomain &fine, FieldRef dst,
                              FieldRef add, const Rect3 &region, hipStream_t stream, int zchunk) {
  TransferLaunchInfo info;
  const XferArgs<T> a = prolong_plan<T>(coarse, src, fine, dst, add, region, zchunk, &info);
  if (info.path == 0) {
    prolong_host<T>(a);
    return;
  }
  fine.set_device();
  const dim3 grid(uint32_t(info.blocks)), block(kXferThreads);
  if (info.path == 2) {
    if (a.add)
      hipLaunchKernelGGL((grid_prolong_chunks_kernel<T, true>), grid, block, 0, stream, a);
    else
      hipLaunchKernelGGL((grid_prolong_chunks_kernel<T, false>), grid, block, 0, stream, a);
  } else {
    if (a.add)
      hipLaunchKernelGGL((grid_prolong_generic_kernel<T, true>), grid, block, 0, stream, a);
    else
      hipLaunchKernelGGL((grid_prolong_generic_kernel<T, false>), grid, block, 0, stream, a);
  }
  HIP_CHECK(hipGetLastError());
}

static int64_t prolong_check(const LocalDomain &coarse, FieldRef src, const LocalDomain &fine, FieldRef dst, FieldRef add,
                             const Rect3 &region, int zchunk) {
  const int64_t es = xfer_check(fine, dst, coarse, src);
  if (add.q >= 0) {
    int64_t ea = 0;
    STENCIL_REQUIRE(xfer_fp(fine, add.q, &ea), "grid transfer takes fp32 / fp64 quantities (add: quantity " << add.q << ")");
    STENCIL_REQUIRE(ea == es, "grid transfer operands differ in type: " << es << "- and " << ea << "-byte elements");
    // add is addressed at dst's element offset (kernels and host loop alike): the two buffers must have one layout. The
    // y and z pitches are the sub-domain's; the row pitch and the front padding follow from the element size today
    STENCIL_REQUIRE(fine.pitch(add.q).x == fine.pitch(dst.q).x && fine.pad_x(add.q) == fine.pad_x(dst.q),
                    "grid transfer operands differ in row pitch");
  }
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx)
        STENCIL_REQUIRE((dx == 0 && dy == 0 && dz == 0) || coarse.radius().dir(dx, dy, dz) >= 1,
                        "prolongation reads one coarse halo cell in all 26 directions: the coarse radius of direction ("
                            << dx << ", " << dy << ", " << dz << ") is 0");
  STENCIL_REQUIRE(zchunk >= 0, "prolongation zchunk " << zchunk);
  require_region_in_compute(fine, region, "prolongation region");
  return es;
}

void grid_prolong_enqueue(const LocalDomain &coarse, FieldRef src, const LocalDomain &fine, FieldRef dst, FieldRef add,
                          const Rect3 &fineRegion, hipStream_t stream, int zchunk) {
  const int64_t es = prolong_check(coarse, src, fine, dst, add, fineRegion, zchunk);
  if (fineRegion.empty()) return;
  if (es == 4)
    prolong_enqueue_t<float>(coarse, src, fine, dst, add, fineRegion, stream, zchunk);
  else
    prolong_enqueue_t<double>(coarse, src, fine, dst, add, fineRegion, stream, zchunk);
}

TransferLaunchInfo grid_prolong_launch_info(const LocalDomain &coarse, FieldRef src, const LocalDomain &fine,
                                            FieldRef dst, FieldRef add, const Rect3 &fineRegion, int zchunk) {
  const int64_t es = prolong_check(coarse, src, fine, dst, add, fineRegion, zchunk);
  TransferLaunchInfo info;
  if (fineRegion.empty()) {
    info.path = -1;
    return info;
  }
  if (es == 4)
    prolong_plan<float>(coarse, src, fine, dst, add, fineRegion, zchunk, &info);
  else
    prolong_plan<double>(coarse, src, fine, dst, add, fineRegion, zchunk, &info);
  return info;
}

} // namespace stencil
