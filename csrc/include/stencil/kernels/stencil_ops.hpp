#pragma once
// Compute kernels of the reference apps, written for CDNA4.
// Reference kernels:
//   Jacobi3D  init_kernel / stencil_kernel (6-neighbour mean + hot/cold spheres)   bin/jacobi3d.cu:18-87
//   Astaroth  init_kernel (sin wave, halo -10) / stencil_kernel (6-neighbour mean)  bin/astaroth_sim.cu:14-83
// The device kernel is a 2.5D z-march: each lane owns one 16-B x-chunk (4 fp32 / 2 fp64) of TY consecutive rows and
// walks z keeping planes z-1, z, z+1 in registers, so every interior cell is read from HBM ~once per sweep
// (y-halo rows are shared through L1/L2 by the 4 waves of a block, x-neighbours come from adjacent lanes by
// ds_bpermute). Blocks are remapped XCD-aware so y/z-adjacent tiles share an XCD's L2. Summation order and the
// division by 6 are the reference's, so results are bitwise identical to a sequential fp32 evaluation.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "stencil/core/geometry.hpp"
#include "stencil/domain/local_domain.hpp"

namespace stencil {

enum class StencilKind : int {
  Jacobi = 0,   // sum order +x,-x,+y,-y,+z,-z then /6, hot/cold spheres
  Astaroth = 1, // sum order -x,-y,-z,+x,+y,+z then /6
};

struct Spheres {
  bool enabled = false;
  Dim3 hot, cold;     // global coordinates of the sphere centres
  int64_t radius = 0; // cell is inside iff floor(sqrt(|p-c|^2)) <= radius  <=>  |p-c|^2 < (radius+1)^2
  // reference placement (bin/jacobi3d.cu:45-50) for a global compute region
  static Spheres jacobi(const Rect3 &cReg) {
    Spheres s;
    s.enabled = true;
    s.hot = Dim3(cReg.lo.x + (cReg.hi.x - cReg.lo.x) / 3, (cReg.lo.y + cReg.hi.y) / 2, (cReg.lo.z + cReg.hi.z) / 2);
    s.cold = Dim3(cReg.lo.x + (cReg.hi.x - cReg.lo.x) * 2 / 3, (cReg.lo.y + cReg.hi.y) / 2, (cReg.lo.z + cReg.hi.z) / 2);
    s.radius = (cReg.hi.x - cReg.lo.x) / 10;
    return s;
  }
};

struct StencilTune {
  // 2 (default): LDS-shared y-halo kernel with 2 planes of z lookahead (every row load has a whole z step to land;
  //    3/4: 3/4 planes), 0: LDS kernel with 1 plane (the loads are consumed in the step that issues them),
  //    1: register-only kernel. 512^3 fp32 on one MI355X: 201 us (v2) vs 212 us (v0) per sweep.
  int variant = 2;
  // variant kMfma: the x line update on the matrix cores (stencil7_mfma.hip; fp32 Jacobi, for counter comparison)
  static constexpr int kMfma = 8;
  int ty = 2;     // rows per lane (variant 0: 2/4/8, variant 1: 4/8)
  int zchunk = 0; // planes per block (0 = auto: exactly one round of resident blocks)
  int nw = 8;     // waves per block stacked in y (deep-lookahead variants: 4/8/16)
  int x3sched = 1;        // fused triples: 0 = the pairs' lockstep schedule, 1 = lockstep over the most row groups
  int x3parts = 0;        // fused triples, x3sched 1: lockstep z parts per row group (0 = the cost model's choice)
  // fused triples (Jacobi): extra weight of a sphere-crossing row-plane when the lockstep z parts are cut per row group
  // and the leftover groups planned (0: equal parts). 0.3 was best with equal leftover slices, 0.6 with levelled
  // slices (x3left 1, profiles/r6/r6z), 0.45 with the second lockstep phase (x3left 2 / 3: steady-state 512^3 triple
  // 226.1 us vs 228.2 at 0.3 and 228.1 at 0.6, driver command 1613-1633 Gcells/s, profiles/r6/r6ad)
  float x3sphw = 0.45f;
  float x2sphw = 0.15f;   // fused pairs (Jacobi, row / col2 kernels): sphere weight of the z parts (r5/at, r5/au)
  bool x3sphchunk = true; // fused triples (Jacobi): test each sphere only on the lane chunks its x range reaches
  // fused triples, lockstep parts: the row groups beyond the parts' (leftover groups) as second segments. 0 = equal
  // slices; 1 = slices levelling each block against the blocks whose parts cost more (sphere-crossing groups);
  // 2 = a second lockstep phase (every leftover group in K parts of common z bounds, blocks binned by their parts'
  // cost); 3 = whichever of 1 / 2 the host's step estimate prefers, with the number of parts chosen the same way
  int x3left = 3;
  bool x2early = true;    // fused pairs (row / col2 kernels): publish the src and u1 rows right after the u1 update
                          // (row kernel 208.6 vs 216.6 us per pair, col2 226.9 vs 234.1)
  // fused pairs of fp32 sub-domains: one wave per whole 512-cell periodic row (x wrapped in-kernel and 512 cells
  // long; x-neighbours and the wrap by DPP lane rotates, stencil7x2_row_kernel), or 512-cell columns (x a whole
  // number of 512-cell columns: two 16-B chunks per lane, only the column ends from outside the wave,
  // stencil7x2_col2_kernel). 0 = always the 256-cell column kernel
  int x2row = 1;
  // fused-pair work split: 1 (default) = one block per resident slot, each taking an equal share of the
  // (column, plane) space (one or two z segments): no partly empty last round and the fewest warm-up planes;
  // 0 = fixed z-chunks per block column (zchunk / auto)
  int x2sched = 1;
  // fused-pair column order: 1 = x-major (x-adjacent columns of a y range on one XCD), 0 = y-major. One MI355X:
  // 512^3 equal within noise (944-965 Gcells/s either way); 645/813/1024-wide shapes 2-3 % faster y-major
  int x2xfast = 0;
  // CUs an overlapped fused-pair interior sweep leaves free for the exchange kernels of the comm stream (balanced
  // segment mode: the grid is that many blocks short of the resident slots); reserveCUs is what one launch uses
  int x2reserve = 8;
  int reserveCUs = 0;
  // whole-row fused pairs with fewer resident blocks than 4 per row group (CUs reserved for the transports): four
  // blocks per column march lockstep z quarters, so y-adjacent blocks share their halo rows in L2 (512^3 local
  // interior beside the slab kernels 276 -> 252 us); false = the balanced (column, plane) split
  bool x2lockstep = true;
  // overlapped fused pairs: the z slabs of periodic 512-cell rows go through the whole-row kernel with the slab as its
  // z chunk (true) or through the thin slab kernel (false); both time the same within 2 % (r2s3)
  bool zslabRow = true;
  bool xcdRemap = true;
  // nontemporal output stores. Fused triples: the whole-row kernel compiles an instance per setting (512^3: 1828-1849
  // Gcells/s with, 1783-1797 without, BASELINE.md "Deferred output stores"); in the XH form (columns with x halos)
  // and in the publishing instances the flag does nothing, their stores are plain
  bool nontemporal = true;
  // reverse the z-march of every block on odd buffer parities: each step then starts on the planes the previous
  // step wrote last, which are still in the MALL / L2
  // flip the z-march direction every pair (each sweep starts on the planes the previous one wrote last). r2s3, rows
  // 64-B aligned: -3 % (1164 vs 1202); r4, rows on whole 128-B lines: +2-6 % at 512^3 (interleaved bench.py
  // 1276-1290 vs 1256-1272, shape sweep 1321 / 1392 vs 1247 / 1311), +3-4 % at 645x645x323 and 1024x512x256, neutral
  // at 813-cell rows and fp64 (profiles/r4/q, profiles/r4/r): on
  bool alternateZ = true;
  // bitmask of axes (1 = x, 2 = y, 4 = z) along which the sub-domain is its own periodic
  // neighbour and the kernels read the periodic image in place of the halo (StencilModel sets it together with
  // DistributedDomain::exchange_async(.., skipWrapped), which then skips those same-GPU self copies). Needs the
  // region to span the whole compute region along wrapped axes, and for x an extent that is a multiple of the
  // 16-B chunk (fused pairs: >= 2 chunks). Fused pairs: stencil7x2_wrappable_axes; single steps (stencil7_apply):
  // stencil7_wrappable_axes. 0 = read halos.
  int wrap = 0;
  // pipelined pairs (StencilModel overlap mode 3; run-time state, not configuration): the whole-row kernel adds the
  // number of cells it has written in the first / last `publishDepth` z planes of the region to *publish (device
  // word, system-scope release after each such plane), so a gated exchange (DistributedDomain::set_send_gate) packs
  // the boundary planes while the rest of the sweep is still running. Other fused-pair kernels refuse it.
  uint64_t *publish = nullptr;
  // measurement: stencil7x3 writes every block's start / end wall clock (2 x uint64 per block) here when set
  uint64_t *blockClock = nullptr;
  int publishDepth = 0;
};
// the whole-row fused-pair kernel (the one that can publish its boundary planes) takes this region
bool stencil7x2_row_kernel_used(const LocalDomain &dom, int64_t qi, const Rect3 &region, const StencilTune &tune);
// axes (mask as StencilTune::wrap) the fused-pair kernels can wrap in-kernel for this quantity's layout; x2row as
// StencilTune::x2row (0: no whole-row kernel, so ragged x extents are not wrappable)
int stencil7x2_wrappable_axes(const LocalDomain &dom, int64_t qi, int x2row = 1);

// Halo forwarding: the producer writes its neighbours' halos. For every direction whose receiving halo lives in a
// sub-domain this process can store into directly (same GPU, or a P2P-mapped peer GPU over xGMI), the stencil
// kernel also stores each boundary output cell into the receiver's *next* buffer (the one that becomes curr after
// swap). A step is then one kernel per sub-domain (plus a small copy for receivers with a different layout): no
// pack, no separate exchange, and the halos of the new curr are valid when the step retires. Replaces the reference's separate exchange() for the Kernel/PeerCopy methods
// (reference tx_cuda.cuh:68-95 multi_translate, :141-162 peer copy).
struct ForwardTarget {
  Dim3 dir;                   // send direction
  const LocalDomain *dst;     // receiving sub-domain (same process)
  Dim3 offset;                // dst raw coordinate = src raw coordinate + offset
};

class HaloForwarder {
public:
  // per buffer parity (the receivers' next buffers alternate with swap()): an in-kernel store offset for every
  // receiver that shares this sub-domain's pitches, and a copy plan (run right after the kernel) for the others
  // (e.g. x neighbours of a different x size in an uneven partition). `targets` come from
  // DistributedDomain::forward_targets.
  HaloForwarder(const LocalDomain &src, int64_t qi, const std::vector<ForwardTarget> &targets);
  ~HaloForwarder();
  HaloForwarder(const HaloForwarder &) = delete;
  HaloForwarder &operator=(const HaloForwarder &) = delete;
  // cells within wm[a] of the low face send along -a, within wp[a] of the high face along +a
  const int *wm() const { return wm_; }
  const int *wp() const { return wp_; }
  int num_targets() const { return n_; }
  uint32_t mask(int parity) const { return mask_[parity]; }              // directions stored by the kernel
  int64_t delta(int parity, int k) const { return delta_[parity][k]; }   // element offset from the output cell
  bool has_rest() const { return hasRest_; }
  // copy the messages the kernel does not store (after the kernel, same stream)
  void forward_rest(int parity, hipStream_t stream) const;
  // can the forwarding kernel handle this sub-domain (aligned vector layout, fp32/fp64, sizes >= slab widths)?
  static bool supported(const LocalDomain &dom, int64_t qi);

private:
  int wm_[3] = {0, 0, 0}, wp_[3] = {0, 0, 0};
  int n_ = 0;
  int dev_ = -1;
  uint32_t mask_[2] = {0, 0};
  int64_t delta_[2][27] = {};
  CopyPlan rest_[2];
  bool hasRest_ = false;
};

// The host plan of a whole-row fused-triple sweep (stencil7x3's lockstep schedule, as apply runs it for a sub-domain
// of `size` cells with the reference's spheres for Jacobi, on `slots` resident blocks): for tests and tools, no GPU
struct X3PlanInfo {
  int parts = 0, blocks = 0, groups = 0, lockstepGroups = 0, rounds = 0;
  bool tabled = false;     // second segments from l0 / l1 / odd (leftover (column, plane) offsets), else equal slices
  double steps = 0;        // estimated steps of the longest block
  std::vector<int> zb;     // per lockstep group its parts - 1 z bounds (empty: equal parts)
  std::vector<int> l0, l1; // per block: its leftover slice
  std::vector<int> odd;    // per block: the slice's march direction bit
  // every march of the sweep in the order its block runs them, five ints each: block, row group, first plane, planes,
  // marching down (at sweep parity 0; StencilTune::alternateZ flips every direction on odd sweeps). A march of n
  // planes runs n + 4 z steps
  std::vector<int> marches;
};
X3PlanInfo stencil7x3_plan(const Dim3 &size, bool jacobi, const StencilTune &tune, int slots = 256);
// dst(region) = stencil(src) for one quantity of one LocalDomain. `region` is in global coordinates and must lie in
// the domain's compute region; face radii must be >= 1. `currIsSrc` selects curr->next (true) or next->curr.
// With `fwd`, region must be the whole compute region and the output is also forwarded into the receivers' halos.
void stencil7_apply(const LocalDomain &dom, int64_t qi, const Rect3 &region, StencilKind kind, const Spheres &sph,
                    hipStream_t stream, const StencilTune &tune = StencilTune(), const HaloForwarder *fwd = nullptr);
// Two fused steps (temporal blocking): dst(region) = S(S(src)), bitwise equal to two single steps. Needs halos of
// depth 2 on the faces and 1 on the edges (Radius::face_edge_corner(2, 1, 0) or more) valid in src, a device
// fp32/fp64 quantity and the aligned layout (stencil7x2_supported). Reads src once and writes dst once per two steps.
bool stencil7x2_supported(const LocalDomain &dom, int64_t qi);
void stencil7x2_apply(const LocalDomain &dom, int64_t qi, const Rect3 &region, StencilKind kind, const Spheres &sph,
                      hipStream_t stream, const StencilTune &tune = StencilTune());
// Three fused steps: dst = S(S(S(src))) on the whole compute region, bitwise equal to three single steps. x either
// wraps in-kernel (tune.wrap & 1: fp32 rows of exactly 512 cells) or is read from 3-deep halos (fp32 x a multiple of
// 512, fp64 of 256; faces, edges and corners exchanged); y / z wrap in-kernel or read 3-deep halos.
// Returns false (nothing launched) when this layout / region / tune is not supported.
bool stencil7x3_supported(const LocalDomain &dom, int64_t qi, const Rect3 &region, const StencilTune &tune);
// cells per column of the form that reads x from halos (XH): two 16-B chunks per lane, 512 fp32 / 256 fp64
int64_t stencil7x3_column_cells(int64_t elemSize);
bool stencil7x3_apply(const LocalDomain &dom, int64_t qi, const Rect3 &region, StencilKind kind, const Spheres &sph,
                      hipStream_t stream, const StencilTune &tune);
// S o S on several small regions (the exterior slabs of an overlapped fused pair), one thread per cell
void stencil7x2_apply_regions(const LocalDomain &dom, int64_t qi, const std::vector<Rect3> &regions, StencilKind kind,
                              const Spheres &sph, hipStream_t stream, int wrap = 0);
// S o S on the compute region minus `interior` (the exterior of an overlapped fused pair): z slabs and y slabs by
// the sweep kernel (6 waves per block for 2-row slabs), thin x slabs by a lanes-on-rows kernel
void stencil7x2_apply_exterior(const LocalDomain &dom, int64_t qi, const Rect3 &interior, StencilKind kind,
                               const Spheres &sph, hipStream_t stream, const StencilTune &tune = StencilTune());
// Lockstep block schedule of the whole-row / 512-cell-column fused pairs: `slots` resident blocks, `cols` row
// groups (8 output rows of one column strip each), `nz` planes. P blocks per row group march P z parts side by side (y-adjacent blocks on one XCD, so their
// shared y-halo rows meet in L2): quarters (P = 4) over the first slots / 4 row groups with the rest as short
// second segments, or P = slots / cols over every row group when the grid has fewer than slots / 4 row groups or
// the row groups divide the slots evenly; rounds of whole columns when there are more row groups than slots
// (813x407x407: 51 groups, 5 parts, 847 -> 910-917 Gcells/s; 645x323x645: 41 groups, 6 parts, 847 -> 1067-1072).
// Whole columns over fewer slots instead of quarters plus leftovers lose (645x645x323, 81 groups: 3 parts on 243
// blocks 930-946 vs 994-1001; profiles/r3/s3/ab_lockstep_parts.txt). parts == 0: no lockstep (parts under 16
// planes, or nz < 64): balanced split.
struct X2Schedule {
  int parts = 0;
  int64_t blocks = 0;
  int rounds = 1; // > 1: block b marches part b / cm of columns b % cm, b % cm + cm, ... (cm = blocks / parts) in
                  // step with the others; parts 1 = whole columns
};
// rounds = false: never rounds (a kernel without the round loop: quarters plus second segments, or no lockstep)
inline X2Schedule x2_lockstep_schedule(int64_t slots, int64_t cols, int64_t nz, bool rounds = true) {
  X2Schedule r;
  if (slots < 4 || cols < 1) return r;
  if (cols > slots && rounds) {
    // more row groups than blocks (fp64 1024^3 as 256-cell columns: 4 x 128 groups): rounds of whole columns, every
    // block on one column per round, y-adjacent columns side by side (quarters plus leftovers would run most
    // columns as balanced second segments)
    if (nz < 16) return r;
    r.rounds = int((cols + slots - 1) / slots);
    r.parts = 1;
    r.blocks = (cols + r.rounds - 1) / r.rounds;
    return r;
  }
  // whole columns when they divide the slots evenly (1024x512x256 on the 512-cell column kernel: 128 columns, P = 2)
  const int64_t P = (slots / 4 > cols || slots % cols == 0) ? slots / cols : 4;
  const int64_t cm = cols < slots / P ? cols : slots / P;
  if (cm < 1 || nz < 64 || nz / P < 16) return r;
  r.parts = int(P);
  r.blocks = P * cm;
  if (rounds && P == 4 && cm < cols && cols % 2 == 0) {
    // quarters over slots / 4 row groups leave the rest to balanced second segments; two rounds of P2 parts over
    // half the row groups each keep every segment in lockstep when they fill 15 / 16 of the slots in both rounds
    // (813x813x204: 102 groups = 2 rounds x 51 groups x 5 parts on 255 blocks, 928-931 -> 970-971 Gcells/s; an odd
    // count idles blocks in the second round: 645x645x323, 81 groups as 2 x 41 x 6, 1034 -> 1009-1018, not taken;
    // profiles/r3/s3/ab_rounds_parts.txt)
    const int64_t ch = cols / 2, P2 = slots / ch;
    if (P2 >= 2 && nz / P2 >= 16 && 16 * P2 * ch >= 15 * slots) {
      r.parts = int(P2);
      r.blocks = P2 * ch;
      r.rounds = 2;
    }
  }
  return r;
}

// The resident blocks a launch may fill when it leaves reserveCUs of the device's `cus` CUs (at most half of them) to
// the kernels of another stream (the transports beside an overlapped sweep): the one slots formula of every kernel
inline int64_t slots_less_reserved(int64_t resident, int reserveCUs, int cus) {
  const int64_t perCU = std::max<int64_t>(1, resident / std::max(1, cus));
  return std::max<int64_t>(perCU, resident - perCU * std::min(reserveCUs, cus / 2));
}

// The kernel form of a fused-pair sweep (stencil7x2), decided in one place for stencil7x2_apply, its launch report
// (stencil7x2_launch_info), stencil7x2_row_kernel_used and stencil7x2_wrappable_axes. The row forms (fp32 only) run
// one wave per whole periodic row with x wrapped in-kernel: Row = 512 cells, two chunks per lane; Ragged2 / Ragged3 =
// 257-511 / 513-768 cells, 2 / 3 chunks per lane with the row-end cells broadcast for the wrap; Tail = 769-832 cells,
// three chunks plus one tail cell per lane. Col2 = x a whole number of two-chunk columns (512 fp32 / 256 fp64 cells);
// Column = the one-chunk column kernel, which takes everything else.
enum class X2Form : int { Row = 0, Ragged2, Ragged3, Tail, Col2, Column };
inline bool x2_row_form(X2Form f) { return f <= X2Form::Tail; }
// the row widths some row form takes
inline bool x2_row_width(int64_t nx) { return nx > 256 && nx <= 832; }
// elemSize 4 / 8; nx = the region's x extent; x0 = its first x cell counted from the first interior cell of the row
// (16-B aligned in memory: the forms other than Column need the region to start on a chunk); wrap, x2row as
// StencilTune's; publishing = tune.publish set (only the row forms publish: any other form is reported as Column, and
// apply refuses it); bufferBytes = LocalDomain::buffer_bytes (the row forms address the field by 32-bit buffer offsets).
// Pure host code, no GPU.
inline X2Form stencil7x2_form(int64_t elemSize, int64_t nx, int64_t x0, int wrap, int x2row, bool publishing,
                              int64_t bufferBytes) {
  if (!x2row) return X2Form::Column;
  const int64_t V = 16 / elemSize, cw = 128 * V; // cells per chunk, per two-chunk column
  const bool onChunk = x0 % V == 0;
  if (elemSize == 4 && (wrap & 1) && onChunk && x2_row_width(nx) && bufferBytes < (int64_t(1) << 32) - 4096) {
    // Ragged periodic rows: H = 2 / 3 chunks per lane (one plane of lookahead: the 3-chunk window leaves no registers
    // for more). Four chunks per lane (rows of 769-1024) need 10-wave blocks for the LDS and spill at their 168-VGPR
    // budget: 358 vs 668 Gcells/s for the column kernel at 813x407x407 (profiles/r2/r2_ragged_shapes.log); 8-wave
    // blocks (2 waves per SIMD, 200 VGPRs, 4 output rows of 8) 597 vs 668 (r2_ragged_h4_8waves.log). Not instantiated:
    // rows of 769-832 cells (the 4-GPU ladder's 813) run three chunks per lane plus one tail cell per lane.
    return nx == 512 ? X2Form::Row : nx < 512 ? X2Form::Ragged2 : nx <= 768 ? X2Form::Ragged3 : X2Form::Tail;
  }
  return !publishing && onChunk && nx % cw == 0 ? X2Form::Col2 : X2Form::Column;
}

// The block schedule of a fused-pair sweep, decided in one place for every form: `cols` block columns (row groups x
// column strips) of nz planes, `resident` blocks resident at once, `slots` of them for this launch
// (slots_less_reserved).
//   seg 0: fixed z chunks of zc planes (tune.x2sched = 0, or tune.zchunk given; auto: pick_zchunk), blocks = cols gz;
//   seg 1: the balanced (column, plane) split over `blocks` blocks, pieces of at least 16 planes;
//   seg 2: `parts` lockstep z parts over blocks / parts columns, the other columns as second segments;
//   seg 3: `rounds` lockstep rounds of `parts` z parts over blocks / parts columns each (x2_lockstep_schedule).
// The one-chunk column form never runs lockstep, the two-chunk column form only with its columns y-major
// (!tune.x2xfast: y-adjacent columns are consecutive), the row forms always may. Pure host code, no GPU.
struct X2SweepSchedule {
  int seg = 1, parts = 0, rounds = 1;
  int64_t blocks = 0;
  int zc = 1, gz = 1;
};
X2SweepSchedule stencil7x2_schedule(X2Form form, int64_t cols, int nz, int64_t resident, int64_t slots,
                                    const StencilTune &tune);
// What stencil7x2_apply would launch for this region, kind and tune (nothing is launched; the same refusals raise; an
// empty region reports blocks = 0): the kernel form, its in-kernel wrap variant (0 none, 1 y / z, 2 x too), the
// schedule's inputs (slots: the occupancy query less tune.reserveCUs' share) and the schedule
struct X2LaunchInfo {
  X2Form form = X2Form::Column;
  int wrapVariant = 0;
  int64_t cols = 0, slots = 0;
  int seg = 0, parts = 0, rounds = 1;
  int64_t blocks = 0;
  int zchunk = 0, gz = 0;
};
X2LaunchInfo stencil7x2_launch_info(const LocalDomain &dom, int64_t qi, const Rect3 &region, StencilKind kind,
                                    const Spheres &sph, const StencilTune &tune = StencilTune());

// The launch schedule of a fused-triple sweep (stencil7x3), decided in one place for stencil7x3_apply, the planner
// (stencil7x3_plan) and the tests: `cols` (row group, column) pairs of `nz` planes on `slots` resident blocks.
//   seg 1: the balanced (column, plane) split over `blocks` blocks (parts 0);
//   seg 2: `parts` lockstep z parts over blocks / parts row groups, the other groups as second segments (the host plan,
//          x3_plan, may still refine parts and blocks);
//   seg 3: `rounds` lockstep rounds of `parts` z parts over blocks / parts column groups each.
// Rounds exist only in the XH kernel (columns with x halos): the whole-row form (xh = false) never gets them, and
// neither form does while publishing boundary planes (the publishing pass order is written for two passes). Such
// sweeps run what the schedule gives without its rounds branches: seg 2 with the leftover groups as second segments,
// or seg 1 where no part count is admissible. Pure host code, no GPU.
struct X3Schedule {
  int seg = 1, parts = 0;
  int64_t blocks = 0;
  int rounds = 1;
};
X3Schedule stencil7x3_schedule(bool xh, int64_t cols, int64_t nz, int64_t slots, const StencilTune &tune,
                               bool publishing);
// What stencil7x3_apply would launch for this sub-domain, kind and tune (nothing is launched): the kernel form, the
// schedule's inputs (slots: the occupancy query less tune.reserveCUs' share, as apply computes it) and the launch after
// the host plan. supported = false (every other field default) where stencil7x3_supported refuses.
struct X3LaunchInfo {
  bool supported = false;
  bool xh = false, ragged = false; // columns with x halos (else whole rows wrapped in-kernel); a partial last column
  int64_t cols = 0, slots = 0;
  int seg = 0, parts = 0;
  int64_t blocks = 0;
  int rounds = 0;
};
X3LaunchInfo stencil7x3_launch_info(const LocalDomain &dom, int64_t qi, const Rect3 &region, StencilKind kind,
                                    const Spheres &sph, const StencilTune &tune);

// axes (mask as StencilTune::wrap) stencil7_apply can wrap in-kernel for this quantity's layout: with tune.wrap set
// the single step reads the periodic image along those axes instead of the halo (the region must span them)
int stencil7_wrappable_axes(const LocalDomain &dom, int64_t qi);
// MFMA variant of the single step (fp32 Jacobi; StencilTune::variant == kMfma routes stencil7_apply here)
bool stencil7_mfma_supported(const LocalDomain &dom, int64_t qi);
void stencil7_mfma_apply(const LocalDomain &dom, int64_t qi, const Rect3 &region, StencilKind kind, const Spheres &sph,
                         hipStream_t stream, const StencilTune &tune = StencilTune());
// same for several regions in one call (e.g. the exterior slabs)
void stencil7_apply_regions(const LocalDomain &dom, int64_t qi, const std::vector<Rect3> &regions, StencilKind kind,
                            const Spheres &sph, hipStream_t stream, const StencilTune &tune = StencilTune());

// Weighted star stencil of radius 1-3 (stencil_star.hip): for a quantity of element type T (fp32 / fp64)
//   acc = center * u(c); for axis in x, y, z: for k in 1..radius: acc += w[axis][-][k] * u(c - k e); acc += w[axis][+][k] * u(c + k e)
// with the weights converted to T once on the host and every product and sum its own IEEE rounding in T in exactly
// this order (no FMA contraction; zero weights are multiplied like any other, so NaN / Inf propagate). All 6 radius + 1
// weights are independent (upwind stars work). Bitwise equal to stencil2_amd.ops.star_step_reference.
struct StarWeights {
  int radius = 1;
  double center = 0;
  double w[3][2][3] = {}; // [axis x, y, z][0: -, 1: +][k - 1]
};
// an fp32 / fp64 quantity (or opaque 4- / 8-byte elements), radius 1..3 and all six face radii >= radius
bool stencil_star_supported(const LocalDomain &dom, int64_t qi, const StarWeights &w);
// next(region) = star(curr) for one quantity of one LocalDomain; only cells of `region` (global coordinates, inside
// the compute region; empty: no-op) are written. Neighbours come from the halos of curr (exchange() first; edges and
// corners are not read: Radius::face_edge_corner(radius, 0, 0) suffices). Device sub-domains in the aligned vector
// layout (as stencil7_apply's) run a 2.5D z-march: one 16-B x chunk of 2 rows per lane, a register ring of the
// 2 radius + 1 planes, the block's 16 rows plus `radius` halo rows each side shared through LDS, x neighbours from
// adjacent lanes, each source cell read from HBM about once per sweep; any other layout runs one thread per cell,
// Backend::Host a plain loop. Of `tune`: zchunk (0 = one round of resident blocks, at most two per CU, chunks of >= 16 planes),
// nontemporal, xcdRemap, alternateZ; tune.wrap != 0 is refused (no in-kernel wrap, forwarding or temporal fusion).
void stencil_star_apply(const LocalDomain &dom, int64_t qi, const Rect3 &region, const StarWeights &w,
                        hipStream_t stream, const StencilTune &tune = StencilTune());
// What stencil_star_apply would run for these arguments (nothing is launched; the same refusals raise)
struct StarLaunchInfo {
  int path = 0;       // -1 nothing (empty region), 0 host loop, 1 one thread per cell, 2 the z-march kernel
  int zchunk = 0;     // z-march: planes per block
  int zchunks = 0;    // z-march: chunks along z
  int64_t blocks = 0; // z-march: blocks of the launch
};
StarLaunchInfo stencil_star_launch_info(const LocalDomain &dom, int64_t qi, const Rect3 &region, const StarWeights &w,
                                        const StencilTune &tune = StencilTune());

// Weighted 27-point box stencil (stencil_box.hip): for a quantity of element type T (fp32 / fp64)
//   acc = w[-1][-1][-1] * u(c + (-1, -1, -1)); then for (dz, dy, dx) in lexicographic order, dz slowest, dx fastest:
//   acc += w[dz][dy][dx] * u(c + (dx, dy, dz))
// with the weights converted to T once on the host and every product and sum its own IEEE rounding in T in exactly
// this order whatever direction a block marches in z (no FMA contraction; zero weights are multiplied like any other,
// so NaN / Inf propagate). All 27 weights are independent. Bitwise equal to stencil2_amd.ops.box_step_reference.
struct BoxWeights {
  double w[3][3][3] = {}; // [dz + 1][dy + 1][dx + 1]
};
// an fp32 / fp64 quantity (or opaque 4- / 8-byte elements) and all 26 direction radii >= 1 (a 19-point user still needs
// the corners exchanged: zero weights are multiplied, and an unexchanged corner may hold anything)
bool stencil_box_supported(const LocalDomain &dom, int64_t qi);
// next(region) = box(curr) for one quantity of one LocalDomain; only cells of `region` (global coordinates, inside
// the compute region; empty: no-op) are written. Neighbours come from the face, edge and corner halos of curr
// (exchange() first; Radius::face_edge_corner(1, 1, 1) suffices). Device sub-domains in the aligned vector layout (as
// stencil7_apply's) run a 2.5D z-march: one 16-B x chunk of 2 rows per lane, every block marching upwards with three
// partial sums per output cell in flight (the plane at z finishes out(z - 1), continues out(z) and starts out(z + 1),
// so dz = -1 is summed first), each plane published to LDS once (the block's 16 rows plus one halo row each side) for
// the row above and below a lane's own, x neighbours from adjacent lanes, fp32 sums as packed pairs, each source cell
// read from HBM about once per sweep; any other layout runs one thread per cell, Backend::Host a plain loop. Of
// `tune`: zchunk (0 = one round of resident blocks, at most two per CU, chunks of >= 16 planes), nontemporal and
// xcdRemap; alternateZ is ignored (a downward march would sum dz = +1 first); tune.wrap != 0 is refused (no in-kernel
// wrap, forwarding or temporal fusion).
void stencil_box_apply(const LocalDomain &dom, int64_t qi, const Rect3 &region, const BoxWeights &w,
                       hipStream_t stream, const StencilTune &tune = StencilTune());
// What stencil_box_apply would run for these arguments (nothing is launched; the same refusals raise)
struct BoxLaunchInfo {
  int path = 0;       // -1 nothing (empty region), 0 host loop, 1 one thread per cell, 2 the z-march kernel
  int zchunk = 0;     // z-march: planes per block
  int zchunks = 0;    // z-march: chunks along z
  int64_t blocks = 0; // z-march: blocks of the launch
};
BoxLaunchInfo stencil_box_launch_info(const LocalDomain &dom, int64_t qi, const Rect3 &region, const BoxWeights &w,
                                      const StencilTune &tune = StencilTune());

// Variable-coefficient diffusion stencil (stencil_varcoef.hip): for a quantity u and a coefficient quantity k of the
// same element type T (fp32 / fp64) in one LocalDomain
//   acc = shift * u(c); for axis a in x, y, z:
//     km = k(c) + k(c - e_a); dm = u(c - e_a) - u(c); fm = km * dm; tm = h[a] * fm; acc = acc + tm
//     kp = k(c) + k(c + e_a); dp = u(c + e_a) - u(c); fp = kp * dp; tp = h[a] * fp; acc = acc + tp
//   next(u)(c) = acc
// with shift and h converted to T once on the host and every sum, difference and product its own IEEE rounding in T in
// exactly this order (no FMA contraction; zero factors are multiplied like any other, so NaN / Inf propagate). The
// face coefficient is the arithmetic mean with the 1/2 inside h: div(k grad u) at spacing hx takes h[0] = 1 / (2 hx^2).
// k(c) + k(n) is commutative, so the coupling of two cells is bitwise the same from both sides: the operator is
// symmetric by construction. Bitwise equal to stencil2_amd.ops.varcoef_step_reference.
struct VarCoefWeights {
  double shift = 0;
  double h[3] = {0, 0, 0}; // one scale per axis x, y, z
};
// fp32 / fp64 quantities (or opaque 4- / 8-byte elements) of one element size and row pitch in a realized domain
// whose six face radii are >= 1
bool stencil_varcoef_supported(const LocalDomain &dom, int64_t qu, int64_t qk);
// next(u)(region) = the operator above on curr(u) and curr(k); only next(u) is written, and only cells of `region`
// (global coordinates, inside the compute region; empty: no-op), so qk == qu is allowed. Face neighbours of u and of k
// come from the halos of their curr buffers (exchange() both first; Radius::face_edge_corner(1, 0, 0) suffices). Device
// sub-domains in the aligned vector layout (as stencil_star_apply's) run a 2.5D z-march carrying both fields: one 16-B
// x chunk of 2 rows per lane, per field the centre plane, the plane ahead and the entering plane in registers (the
// face term towards the plane behind is computed a step early from the same operands and carried), the block's 16 rows
// plus one halo row each side of both fields shared through LDS (73 728 B per block), x neighbours from adjacent lanes,
// each source cell of both fields read from HBM about once per sweep; any other layout runs one thread per cell,
// Backend::Host a plain loop. Of `tune`: zchunk (0 = one round of resident blocks, at most two per CU, chunks of >= 16 planes), nontemporal,
// xcdRemap, alternateZ; tune.wrap != 0 is refused.
void stencil_varcoef_apply(const LocalDomain &dom, int64_t qu, int64_t qk, const Rect3 &region, const VarCoefWeights &w,
                           hipStream_t stream, const StencilTune &tune = StencilTune());
// What stencil_varcoef_apply would run for these arguments (nothing is launched; the same refusals raise)
struct VarCoefLaunchInfo {
  int path = 0;       // -1 nothing (empty region), 0 host loop, 1 one thread per cell, 2 the z-march kernel
  int zchunk = 0;     // z-march: planes per block
  int zchunks = 0;    // z-march: chunks along z
  int64_t blocks = 0; // z-march: blocks of the launch
};
VarCoefLaunchInfo stencil_varcoef_launch_info(const LocalDomain &dom, int64_t qu, int64_t qk, const Rect3 &region,
                                              const VarCoefWeights &w, const StencilTune &tune = StencilTune());

// Residual and damped-Jacobi sweep of the operator above (stencil_varcoef_relax.hip): for quantities u, k and f of one
// element type T and row pitch in one LocalDomain and a destination buffer dst
//   acc exactly as stencil_varcoef_apply; dg = shift; for axis x, y, z, low face then high face:
//     ks = k(c) + k(n) (the sum acc uses); g = h[axis] * ks; dg = dg - g
//   r = f(c) - acc
//   Residual: dst(c) = r          Jacobi: q = r / dg; s = omega_T * q; dst(c) = u(c) + s
// with shift, h and omega converted to T once on the host and every sum, difference, product and quotient its own IEEE
// rounding in T (no FMA contraction, a true division; dg = 0 is not special: +-inf and NaN propagate). dg is the
// diagonal of the operator at the cell. Bitwise equal to stencil2_amd.ops.varcoef_relax_reference.
enum class VarCoefRelaxMode { Residual, Jacobi };
// fp32 / fp64 quantities (or opaque 4- / 8-byte elements) of one element size and row pitch in a realized domain
// whose six face radii are >= 1
bool stencil_varcoef_relax_supported(const LocalDomain &dom, int64_t qu, int64_t qk, int64_t qf, int64_t qdst);
// dst(region) = the update above from curr(u), curr(k) and curr(f); dst is the curr (dstCurr) or next buffer of
// quantity qdst, and only its cells of `region` are written. dst must not be curr(u) or curr(k), whose neighbours are
// read (refused); it may be curr(f): a cell's f is read only by the lane that stores that cell, before the store. The
// three paths, the halos needed and `tune` are those of stencil_varcoef_apply; the z-march reads f at the centre only
// and carries the diagonal's share of the face behind beside the face term.
void stencil_varcoef_relax(const LocalDomain &dom, int64_t qu, int64_t qk, int64_t qf, int64_t qdst, bool dstCurr,
                           const Rect3 &region, const VarCoefWeights &w, VarCoefRelaxMode mode, double omega,
                           hipStream_t stream, const StencilTune &tune = StencilTune());
// What stencil_varcoef_relax would run for these arguments (nothing is launched; the same refusals raise)
using VarCoefRelaxLaunchInfo = VarCoefLaunchInfo;
VarCoefRelaxLaunchInfo stencil_varcoef_relax_launch_info(const LocalDomain &dom, int64_t qu, int64_t qk, int64_t qf,
                                                         int64_t qdst, bool dstCurr, const Rect3 &region,
                                                         const VarCoefWeights &w, VarCoefRelaxMode mode,
                                                         const StencilTune &tune = StencilTune());

// Jacobi init: curr = 0.5 on `region` (reference bin/jacobi3d.cu:18-29)
void jacobi_init(const LocalDomain &dom, int64_t qi, const Rect3 &region, hipStream_t stream);
// Astaroth init: interior = sin(2*pi/period*(origin+x+y+z)) (x,y,z raw indices), halo = -10 (astaroth_sim.cu:14-61)
void astaroth_init(const LocalDomain &dom, int64_t qi, double period, hipStream_t stream);
// fill every cell of the full region (halo included) of curr with a value
void fill_value(const LocalDomain &dom, int64_t qi, double value, bool curr, hipStream_t stream);

} // namespace stencil
