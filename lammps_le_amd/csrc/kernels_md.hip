// kernels_md.hip — per-timestep kernels: integrate, pair+bond forces, Langevin, kinetic energy.
//
// All arithmetic is IEEE double in the reference's operation order (compiled with
// -ffp-contract=off), so a single call differs from the CPU oracle only through the order in
// which a bead's pair/bond contributions are summed.
//
// Reference semantics restated here:
//   FixNVE::initial_integrate / final_integrate   src/fix_nve.cpp:64-104, :108-141
//   PairLJCut::compute                            src/pair_lj_cut.cpp:68-140
//   PairSoft::compute                             src/pair_soft.cpp:54-122 (the SOFT variants; arithmetic in soft_inl.h)
//   BondFENE::compute / BondHarmonic::compute     src/MOLECULE/bond_fene.cpp:52-128, bond_harmonic.cpp:48-101
//   FixLangevin::post_force_templated<0,...>      src/fix_langevin.cpp:585-778
//   Neighbor::check_distance                      src/neighbor.cpp:1962-2014
//   FixWallRegion::post_force + Region::surface   src/fix_wall_region.cpp:220-302, :353-453, src/region.cpp:138-196,
//                                                 region_sphere.cpp:152-196, region_block.cpp:213-329, region_cylinder.cpp:287-420
#include "device.h"
#include "bin_inl.h"
#include "soft_inl.h"
#include "indent_inl.h"
#include <hip/hip_ext.h>
#include <cstring>

namespace lmp_le {

constexpr int BLOCK = 256;
// the throughput variant of k_step is bound by (resident wavefronts) / (lifetime of one wavefront): occupancy was
// varied on purpose with unused LDS and 16 -> 12 -> 8 waves per CU cost x1.22 and x1.79.  Asking the compiler for five
// waves per SIMD makes it fit 92 VGPRs without scratch (it takes 126 when left alone).
#ifndef STEP_STAGE_W
#define STEP_STAGE_W 4
#endif
#ifndef STEP_WAVES_PER_SIMD
#define STEP_WAVES_PER_SIMD 4
#endif
#define TWO_1_3 1.2599210498948732

// XCD-aware block remap (cdna_hip_programming.md T1): blocks b and b+8 share an XCD, so give
// each XCD one contiguous slab of atoms; its private L2 then holds only that slab's neighborhood.
__device__ __forceinline__ int logical_block(int nblocks_logical) {
  int per = (nblocks_logical + 7) >> 3;
  return (blockIdx.x & 7) * per + (blockIdx.x >> 3);
}
static inline int xcd_grid(int nblocks_logical) { return 8 * ((nblocks_logical + 7) / 8); }

// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_initial_integrate(int n, double4 *__restrict__ pos,
                                                             double *__restrict__ vx, double *__restrict__ vy,
                                                             double *__restrict__ vz, const double *__restrict__ fx,
                                                             const double *__restrict__ fy,
                                                             const double *__restrict__ fz,
                                                             const double4 *__restrict__ xhold, TypeTables tt,
                                                             double dtv, double triggersq, int check,
                                                             int *__restrict__ flags, const int *__restrict__ tag,
                                                             const int *__restrict__ gmask, int groupbit) {
  int p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= n) return;
  double4 r = pos[p];
  // fix nve on a group (`mask[i] & groupbit`, src/fix_nve.cpp:82): the others are not moved by THIS fix - the displacement
  // test below (Neighbor::check_distance, every atom) still looks at them: another fix nve may have moved them
  if (!gmask || (gmask[tag[p]] & groupbit)) {
    double dtfm = tt.dtfm[(int)r.w];
    double a = vx[p], b = vy[p], c = vz[p];
    a += dtfm * fx[p];
    b += dtfm * fy[p];
    c += dtfm * fz[p];
    r.x += dtv * a;
    r.y += dtv * b;
    r.z += dtv * c;
    vx[p] = a; vy[p] = b; vz[p] = c;
    pos[p] = r;
  }
  if (check) {
    double4 h = xhold[p];
    double dx = r.x - h.x, dy = r.y - h.y, dz = r.z - h.z;
    double rsq = dx * dx + dy * dy + dz * dz;
    if (rsq > triggersq) flags[FLAG_MOVED] = 1;
  }
}

__global__ __launch_bounds__(BLOCK) void k_final_integrate(int n, const double4 *__restrict__ pos,
                                                           double *__restrict__ vx, double *__restrict__ vy,
                                                           double *__restrict__ vz, const double *__restrict__ fx,
                                                           const double *__restrict__ fy,
                                                           const double *__restrict__ fz, TypeTables tt,
                                                           const int *__restrict__ tag, const int *__restrict__ gmask,
                                                           int groupbit) {
  int p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= n) return;
  if (gmask && !(gmask[tag[p]] & groupbit)) return;
  double dtfm = tt.dtfm[(int)pos[p].w];
  vx[p] += dtfm * fx[p];
  vy[p] += dtfm * fy[p];
  vz[p] += dtfm * fz[p];
}

// Langevin post_force, optionally fused with FixNVE::final_integrate
template <bool FUSE_FINAL, bool IDENT>
__global__ __launch_bounds__(BLOCK) void k_langevin(int n, const double4 *__restrict__ pos,
                                                    const int *__restrict__ tag, const int *__restrict__ crank,
                                                    const uint32_t *__restrict__ draws, double *__restrict__ vx,
                                                    double *__restrict__ vy, double *__restrict__ vz,
                                                    double *__restrict__ fx, double *__restrict__ fy,
                                                    double *__restrict__ fz, TypeTables tt, const int *__restrict__ gmask,
                                                    int groupbit) {
  int p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= n) return;
  int type = (int)pos[p].w;
  int t = tag[p];
  // fix langevin on a group: only members draw (src/fix_langevin.cpp:660-661), in local order - `crank` is then the rank
  // among the members (DeviceState::lgrank)
  if (gmask && !(gmask[t] & groupbit)) return;
  int rank = IDENT ? (t - 1) : crank[t];
  double gamma1 = tt.g1[type], gamma2 = tt.g2[type];
  const double inv = 1.0 / 16777216.0;
  double r0 = (double)draws[3 * (size_t)rank] * inv;
  double r1 = (double)draws[3 * (size_t)rank + 1] * inv;
  double r2 = (double)draws[3 * (size_t)rank + 2] * inv;
  double fran0 = gamma2 * (r0 - 0.5), fran1 = gamma2 * (r1 - 0.5), fran2 = gamma2 * (r2 - 0.5);
  double a = vx[p], b = vy[p], c = vz[p];
  double fdrag0 = gamma1 * a, fdrag1 = gamma1 * b, fdrag2 = gamma1 * c;
  double f0 = fx[p], f1 = fy[p], f2 = fz[p];
  f0 += fdrag0 + fran0;
  f1 += fdrag1 + fran1;
  f2 += fdrag2 + fran2;
  fx[p] = f0; fy[p] = f1; fz[p] = f2;
  if (FUSE_FINAL) {
    double dtfm = tt.dtfm[type];
    a += dtfm * f0;
    b += dtfm * f1;
    c += dtfm * f2;
    vx[p] = a; vy[p] = b; vz[p] = c;
  }
}

// ------------------------------------------------------------------------------------------
// block reduction of NV doubles per thread -> partial[block][16]
template <int NV>
__device__ __forceinline__ void block_reduce_store(double (&val)[NV], double *__restrict__ partial, int block,
                                                   int col0) {
  __shared__ double red[BLOCK / 64][NV];
  int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; k++) {
    double s = val[k];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double s = 0.0;
    for (int w = 0; w < BLOCK / 64; w++) s += red[w][threadIdx.x];
    partial[(size_t)block * 16 + col0 + threadIdx.x] = s;
  }
}

// column sums of a [nb][W] table of block partials in ONE workgroup, the same order on every run: thread (g, c) adds rows
// g, g + G, g + 2G .. of column c (G = BLOCK / W row groups), then the G group sums are added in group order.  A thermo step
// used to copy the table to the host and add it there (0.5 MB + 65k additions at 1M beads: most of the 190 us a thermo step
// spent outside kernels); now 16 doubles cross
template <int W>
__global__ __launch_bounds__(BLOCK) void k_colsum(int nb, const double *__restrict__ in, double *__restrict__ out) {
  constexpr int G = BLOCK / W;
  __shared__ double part[G][W];
  const int c = threadIdx.x % W, g = threadIdx.x / W;
  double s = 0.0;
  for (int b = g; b < nb; b += G) s += in[(size_t)b * W + c];
  part[g][c] = s;
  __syncthreads();
  if (threadIdx.x < W) {
    double t = 0.0;
    for (int k = 0; k < G; k++) t += part[k][threadIdx.x];
    out[threadIdx.x] = t;
  }
}
__global__ __launch_bounds__(BLOCK) void k_ke(int n, const double4 *__restrict__ pos, const double *__restrict__ vx,
                                              const double *__restrict__ vy, const double *__restrict__ vz,
                                              TypeTables tt, double *__restrict__ partial) {
  int p = blockIdx.x * BLOCK + threadIdx.x;
  double val[1] = {0.0};
  if (p < n) {
    double a = vx[p], b = vy[p], c = vz[p];
    val[0] = (a * a + b * b + c * c) * tt.mass[(int)pos[p].w];
  }
  block_reduce_store<1>(val, partial, blockIdx.x, 14);
}

// ------------------------------------------------------------------------------------------
// force on bead p: pair lj/cut over the full ELL neighbor list + its own bonds (no atomics: every pair
// and bond is evaluated from both ends, which is also what keeps the summation order deterministic)
struct ForceArgs {
  int n, npad, nblocks, bpa, nt;
  const double4 *pos;
  const int *neigh, *numneigh, *bpart;
  const unsigned long long *bshift;   // frozen partner images of the bonds (DeviceState::bshift)
  int bond_minimg;                    // DeviceState::bond_minimg: per-step minimum image is provably the frozen image
  const double *pairtab;
  double sl0, sl1, sl2, sl3;
  // all type pairs share one coefficient set (pair_coeff * * ...): scalars instead of the LDS table
  int uniform;
  double u_cutsq, u_lj1, u_lj2, u_lj3, u_lj4, u_off;
  int has_sb;            // some special weight is neither 0 nor 1 -> list entries carry special bits
  double margin;         // beads farther than this from every box face need no minimum image
  int maxrow;            // highest list row a lane may touch before it knows its count: (maxneigh - 1 - sub) / LPB >= this
  int nn_limit;          // diagnostics only (LAMMPS_LE_NN_LIMIT): cap on neighbors visited per bead
  int diag;              // diagnostics only (LAMMPS_LE_DIAG_STEP): extra launch with parts off, see launch_step
  // ---- from here on read by the step kernel only (k_force carries them unused).  They stay here because the kernel-argument
  // layout decides which scalar loads the compiler merges: with these members behind the type tables the NEXT wall variants,
  // which are bound by SGPRs, spill several times as many of them (1 -> 7, 4 -> 19, 7 -> 54) ----
  // a launch that tests the skin/2 displacement (a rebuild may follow) also bins the new positions: cell, arrival order
  // inside the cell and the cell counts, i.e. everything k_wrap_bin would produce except Domain::pbc itself (k_permute)
  const float4 *holdf;   // float copy of xhold (= posf of the last build; nullptr: use xhold only)
  double hold_band;
  int bin, ncx, ncy, ncz, rtile;
  double cix, ciy, ciz, zlo_ext;
  int *cell_of, *cell_count, *cell_rank;
  // decomposed runs: border beads also write their new position into the halo send buffer (no pack launch per step)
  const int *sendslot;   // (behind its npad words: the {slot below, slot above} pairs of the beads in both lists, DeviceState::sendboth)
  double4 *send_dn, *send_up;   // the staging buffer's two halves, or the neighbours' windows (kernels_dd.hip, fast halo)
};

// The run-time arguments of the step kernel (k_step) by name, one by-value kernel argument; launch_step_kernel fills it, a
// member that the launched instantiation does not use is null.  Two things a member of a by-value struct does not get, and what
// is done about them:
//  - `noalias`: k_step hands the pointers on to the __restrict__ parameters of step_body, which restores it where the loads
//    are scheduled;
//  - an invariant load: a direct kernel argument is loaded where it is used (the load can be rematerialised), a member at the
//    kernel's entry, and it then holds its SGPRs to the end.  The five pointers the kernel uses last - fx, fy, fz, pos_next,
//    xhold - are therefore direct arguments of k_step behind this struct: as members they cost the wall variants up to 17
//    SGPR spills, scratch and, in two of them, the fourth wave.
struct StepKernelArgs {
  const int *tag;
  const int *ranks;      // tag -> rank the draws go by: canonical, or among the members of fix langevin's group (GRP)
  const uint32_t *draws;
  double *vx, *vy, *vz;
  double dtv, triggersq;
  int check;
  int *flags;
  const unsigned char *phase;
  int which;             // decomposed runs with halo / compute overlap: the phase this launch handles (-1: every bead)
  const int *gmask;      // GRP: group masks by tag, and the bits of fix nve / fix langevin
  int nvebit, lgbit;
  const int *vperm;      // LAZYV: bead p reads its velocity at vperm[p] and stores it at p of vxo / vyo / vzo
  double *vxo, *vyo, *vzo;
  const WallTable *walls;   // WALL
  // ANG && NEXT: the bead's listed angles (k_angle_list), their counts and the coefficient table in device memory
  const int4 *angle_rec;
  const int *angle_n;
  const AngleTable *angles;
  double *partial;       // EF: block totals of energies and virial, rows of 16 as k_force<EFLAG> writes them
  // EXT (behind everything the other variants read, whose offsets stay what they were): the run's force-op table (its entries
  // hold the origin blocks), the image words [3][npad] in the order of pos, and the step's activity mask - bit k: entry k acts
  // on the step whose forces this launch computes.  `gmask` above is set when an entry acts on a group other than all
  const ForceOpTable *ext;
  const int *img;
  unsigned ext_active;
  // INDENT (behind everything else, as above): the indenters of fix indent with the geometry of the step whose forces this launch
  // computes - by value, so a radius that is a formula of the step costs no copy on the stream and no wait (n = 0: none)
  IndentTable indents;
};

// reciprocal by v_rcp_f64 + two Newton steps (<= 1 ulp from the IEEE quotient 1/x; an IEEE divide is ~35 instructions)
__device__ __forceinline__ double rcp_nr(double x) {
#pragma clang fp contract(fast)
  double r = __builtin_amdgcn_rcp(x);
  r = r * (2.0 - x * r);
  r = r * (2.0 - x * r);
  return r;
}

// bond coefficients in LDS, one row per bond type, with the per-type constants of BondFENE::compute folded once per
// block: a by-value table indexed by a per-lane type is read through memory (a dependent load for every coefficient)
constexpr int BT_W = 8;   // style, K, 1/R0^2 (fene) or r0 (harmonic), 48 eps, sigma^2, 2^(1/3) sigma^2, R0^2, eps
__device__ __forceinline__ void fill_bond_table(const BondTable &bt, double *__restrict__ s_bt) {
  const int t = threadIdx.x;
  if (t <= MAXTYPES) {
    const int st = bt.style[t];
    const double K = bt.p0[t], R0 = bt.p1[t], epsb = bt.p2[t], sigb = bt.p3[t];
    double *row = s_bt + t * BT_W;
    row[0] = (double)st;
    row[1] = K;
    row[2] = (st == 1) ? 1.0 / (R0 * R0) : R0;     // harmonic: r0; morse: alpha
    row[3] = 48.0 * epsb;
    row[4] = sigb * sigb;
    row[5] = TWO_1_3 * sigb * sigb;
    row[6] = (st == 3) ? epsb : R0 * R0;            // morse: r0 (third coefficient)
    row[7] = epsb;
  }
}

// one pair term.  The hot loop is written for issue-bound FP64 on CDNA4: branch-free minimum image
// (v_rndne), reciprocal by v_rcp_f64 + two Newton steps (<= 1 ulp from the reference's IEEE divide),
// FMA contraction allowed inside this function only (everything else is compiled -ffp-contract=off).
// SOFT: pair_style soft - the same six table columns / u_* scalars hold cutsq, A pi/rc, pi/rc, A (Engine::init_pair_coeffs)
template <bool EFLAG, bool MINIMG, bool UNIFORM, bool HAS_SB, bool SOFT = false>
__device__ __forceinline__ void pair_term(const ForceArgs &A, const Box &box, const double *__restrict__ s_tab,
                                          int itype, const double4 &ri, int jraw, const double4 &rj, bool valid,
                                          double &fxi, double &fyi, double &fzi, double (&e)[14]) {
#pragma clang fp contract(fast)
  double delx = ri.x - rj.x, dely = ri.y - rj.y, delz = ri.z - rj.z;
  if (MINIMG) {
    delx -= box.prd[0] * __builtin_rint(delx * box.iprd[0]);
    dely -= box.prd[1] * __builtin_rint(dely * box.iprd[1]);
    delz -= box.prd[2] * __builtin_rint(delz * box.iprd[2]);
  }
  double rsq = delx * delx + dely * dely + delz * delz;
  double cutsq, lj1, lj2, lj3 = 0.0, lj4 = 0.0, offs = 0.0;
  if (UNIFORM) { cutsq = A.u_cutsq; lj1 = A.u_lj1; lj2 = A.u_lj2; if (EFLAG) { lj3 = A.u_lj3; lj4 = A.u_lj4; offs = A.u_off; } }
  else {
    const int nt2 = A.nt * A.nt, ij = itype * A.nt + (int)rj.w;
    cutsq = s_tab[ij]; lj1 = s_tab[nt2 + ij]; lj2 = s_tab[2 * nt2 + ij];
    if (EFLAG) { lj3 = s_tab[3 * nt2 + ij]; lj4 = s_tab[4 * nt2 + ij]; offs = s_tab[5 * nt2 + ij]; }
  }
  if (SOFT) {
    if (rsq < cutsq && valid) {
      double evdwl = 0.0;
      double fpair = soft_pair<EFLAG>(rsq, __builtin_amdgcn_rsq(rsq), lj1, lj2, lj3, evdwl);
      double factor_lj = 1.0;
      if (HAS_SB) {
        int sb = (jraw >> NEIGH_SB_SHIFT) & 3;
        factor_lj = (sb == 0) ? A.sl0 : (sb == 1) ? A.sl1 : (sb == 2) ? A.sl2 : A.sl3;
        fpair *= factor_lj;
      }
      fxi += delx * fpair; fyi += dely * fpair; fzi += delz * fpair;
      if (EFLAG) {
        evdwl *= factor_lj;
        e[0] += 0.5 * evdwl;
        e[2] += 0.5 * delx * delx * fpair; e[3] += 0.5 * dely * dely * fpair; e[4] += 0.5 * delz * delz * fpair;
        e[5] += 0.5 * delx * dely * fpair; e[6] += 0.5 * delx * delz * fpair; e[7] += 0.5 * dely * delz * fpair;
      }
    }
    return;
  }
  if (rsq < cutsq && valid) {
    double r2inv = __builtin_amdgcn_rcp(rsq);
    r2inv = r2inv * (2.0 - rsq * r2inv);
    r2inv = r2inv * (2.0 - rsq * r2inv);
    double r6inv = r2inv * r2inv * r2inv;
    double forcelj = r6inv * (lj1 * r6inv - lj2);
    double fpair = forcelj * r2inv;
    double factor_lj = 1.0;
    if (HAS_SB) {
      int sb = (jraw >> NEIGH_SB_SHIFT) & 3;
      factor_lj = (sb == 0) ? A.sl0 : (sb == 1) ? A.sl1 : (sb == 2) ? A.sl2 : A.sl3;
      fpair *= factor_lj;
    }
    fxi += delx * fpair; fyi += dely * fpair; fzi += delz * fpair;
    if (EFLAG) {
      double evdwl = r6inv * (lj3 * r6inv - lj4) - offs;
      evdwl *= factor_lj;
      e[0] += 0.5 * evdwl;
      e[2] += 0.5 * delx * delx * fpair; e[3] += 0.5 * dely * dely * fpair; e[4] += 0.5 * delz * delz * fpair;
      e[5] += 0.5 * delx * dely * fpair; e[6] += 0.5 * delx * delz * fpair; e[7] += 0.5 * dely * delz * fpair;
    }
  }
}

// everything a bead's force needs that is addressed by the bead's own index alone: fetched in ONE batch at the top of
// the kernel, before any of it is used.  A small system's step time is the chain of dependent loads one wavefront
// walks (every level costs a trip to the memory-side cache: each kernel starts with a cold L2), so the chain is kept
// at own data -> partners' positions -> next list stage.
struct BeadPre {
  int nall;                // list length word: entries | bond entries << NN_BOND_SHIFT (device.h)
  int j0, j1, j2, j3;      // first list stage (rows below maxneigh always exist; masked once the length is known)
};
template <bool HAS_PAIR, int LPB, bool AHEAD>
__device__ __forceinline__ BeadPre bead_preload(const ForceArgs &A, int p, int sub) {
  BeadPre L;
  if (!AHEAD) {            // throughput-bound sizes: loads stay where they are consumed (measured faster at 1M beads)
    L.nall = HAS_PAIR ? A.numneigh[p] : 0;
    L.j0 = L.j1 = L.j2 = L.j3 = p;
    return L;
  }
  if (HAS_PAIR) {
    const size_t st = (size_t)LPB * A.npad;
    const int *col = A.neigh + p + (size_t)sub * A.npad;
    L.nall = A.numneigh[p];
    L.j0 = col[0]; L.j1 = col[min(1, A.maxrow) * st]; L.j2 = col[min(2, A.maxrow) * st]; L.j3 = col[min(3, A.maxrow) * st];
  } else {
    L.nall = 0; L.j0 = L.j1 = L.j2 = L.j3 = p;
  }
  return L;
}

// one bond term seen from bead p (BondFENE::compute / BondHarmonic::compute; every bond is evaluated from both ends).
// `eb` = (bond type << BOND_TYPE_SHIFT) | partner's index, rj = the partner's position.
// `sh` = the partner's periodic image as frozen at the last reneighbor (BSHIFT_BITS of DeviceState::bshift; 0 for nearly
// every bond): the reference evaluates a bond against the ghost Domain::closest_image picked when the bond list was built
// (src/ntopo_bond_all.cpp:52-73), i.e. x_j + S with a fixed S, not against the minimum image of every step.
template <bool EFLAG, bool ALLSTYLES = false>
__device__ __forceinline__ void bond_term(const Box &box, const double *__restrict__ s_bt, int p, const double4 &ri,
                                          int eb, const double4 &rj, unsigned sh, bool minimg, double &fxi, double &fyi,
                                          double &fzi, double (&e)[14], int *__restrict__ flags) {
  const int q = eb & BOND_IDX_MASK, type = eb >> BOND_TYPE_SHIFT;
  const double *row = s_bt + type * BT_W;
  const int style = (int)row[0];
  if (style == 0) return;
  double xj = rj.x, yj = rj.y, zj = rj.z;
  if (sh) {
    if (sh & 1u) xj += box.prd[0]; else if (sh & 2u) xj -= box.prd[0];
    if (sh & 4u) yj += box.prd[1]; else if (sh & 8u) yj -= box.prd[1];
    if (sh & 16u) zj += box.prd[2]; else if (sh & 32u) zj -= box.prd[2];
  }
  double delx = ri.x - xj, dely = ri.y - yj, delz = ri.z - zj;
  if (minimg) {     // (wave-uniform) all-FENE systems in a large box: see DeviceState::bond_minimg
    const double hx = box.half[0], hy = box.half[1], hz = box.half[2];
    if (delx > hx) delx -= box.prd[0]; else if (delx < -hx) delx += box.prd[0];
    if (dely > hy) dely -= box.prd[1]; else if (dely < -hy) dely += box.prd[1];
    if (delz > hz) delz -= box.prd[2]; else if (delz < -hz) delz += box.prd[2];
  }
  double rsq = delx * delx + dely * dely + delz * delz;
  double fbond, ebond = 0.0;
  if (style == 1) {
    // BondFENE::compute with its four divisions done as products with reciprocals (each <= 1 ulp from the quotient)
    const double K = row[1], inv_r0sq = row[2];
    double rlogarg = 1.0 - rsq * inv_r0sq;
    double sr6 = 0.0;
    if (rlogarg < 0.1) {
      // each bond is visited from both ends: count the warning once (lower index)
      if (p < q) atomicAdd(&flags[FLAG_FENE_WARN], 1);
      if (rlogarg <= -3.0) flags[FLAG_ERROR] = ERR_BAD_FENE;
      rlogarg = 0.1;
    }
    fbond = -K * rcp_nr(rlogarg);
    if (rsq < row[5]) {
      const double rinv = rcp_nr(rsq);
      double sr2 = row[4] * rinv;
      sr6 = sr2 * sr2 * sr2;
      fbond += row[3] * sr6 * (sr6 - 0.5) * rinv;
    }
    if (EFLAG) {
      ebond = -0.5 * K * row[6] * log(rlogarg);
      if (rsq < row[5]) ebond += 4.0 * row[7] * sr6 * (sr6 - 1.0) + row[7];
    }
  } else if (ALLSTYLES && style == 3) {
    // BondMorse::compute (src/MOLECULE/bond_morse.cpp:50-115): D = row[1], alpha = row[2], r0 = row[6]
    const double r = sqrt(rsq), dr = r - row[6], ralpha = exp(-row[2] * dr);
    fbond = (r > 0.0) ? -2.0 * row[1] * row[2] * (1 - ralpha) * ralpha / r : 0.0;
    if (EFLAG) ebond = row[1] * (1 - ralpha) * (1 - ralpha);
  } else {
    double r = sqrt(rsq);
    double dr = r - row[2];
    double rk = row[1] * dr;
    fbond = (r > 0.0) ? -2.0 * rk / r : 0.0;
    if (EFLAG) ebond = rk * dr;
  }
  fxi += delx * fbond; fyi += dely * fbond; fzi += delz * fbond;
  if (EFLAG) {
    e[1] += 0.5 * ebond;
    e[8] += 0.5 * delx * delx * fbond; e[9] += 0.5 * dely * dely * fbond; e[10] += 0.5 * delz * delz * fbond;
    e[11] += 0.5 * delx * dely * fbond; e[12] += 0.5 * delx * delz * fbond; e[13] += 0.5 * dely * delz * fbond;
  }
}

// LPB = lanes per bead: lane `sub` of a bead's LPB lanes takes list entries sub, sub + LPB, ... (see k_step).
// The first `nb` entries of a bead's list are its BONDS ((type << BOND_TYPE_SHIFT) | partner, written by the list build
// from the bond-partner table), the pair entries follow: a bonded partner's position travels through the same pipelined
// gathers as the pair partners', instead of a chain of dependent loads (table entry -> position, one bond after the
// other) behind the pair loop.  Stages that hold a bond entry in some lane (the first one; the second for a wavefront
// with an extruder anchor) run the mixed body, all later ones the plain pair body.
template <bool EFLAG, bool MINIMG, bool UNIFORM, bool HAS_SB, int LPB, bool AHEAD, bool DIAGP = false, bool ALLSTYLES = false, bool SOFT = false>
__device__ __forceinline__ void pair_loop(const ForceArgs &A, const Box &box, const double *__restrict__ s_tab,
                                          const double *__restrict__ s_bt, int p, int sub, const BeadPre &L, int nall,
                                          int nb, unsigned long long bsh, const double4 &ri, double &fxi, double &fyi,
                                          double &fzi, double (&e)[14], int *__restrict__ flags) {
  // software pipeline, W neighbors per stage: while the W position gathers of the current stage are in flight the
  // (coalesced) index loads of the next stage are issued, so a stage costs one exposed round trip.  Lists are
  // consumed in groups of W; slots past the end are predicated off (index = own bead, cached).
  // (the soft term holds more live values per slot than lj/cut's: with four slots per stage the throughput shape needs 3 to 5
  //  registers more than its 128 and the compiler takes them from scratch - 12 to 20 bytes per lane in six of the eight
  //  instantiations; three slots fit, at 124 to 128 registers, and keep the fourth wave)
  constexpr int W = AHEAD ? 4 : SOFT ? 3 : STEP_STAGE_W;
  const int itype = (int)ri.w;
  const size_t npad = (size_t)LPB * A.npad;                                             // stride between a lane's entries
  const int *col = A.neigh + p + (size_t)sub * A.npad;
  const int nn = (LPB == 1) ? nall : (nall > sub ? (nall - sub + LPB - 1) / LPB : 0);   // entries of this lane
  const bool bonds_on = !(DIAGP && (A.diag & 1));
  int j[W];
  if (AHEAD) { j[0] = (0 < nn) ? L.j0 : p; j[1] = (1 < nn) ? L.j1 : p; j[2] = (2 < nn) ? L.j2 : p; j[3] = (3 < nn) ? L.j3 : p; }
  else {
#pragma unroll
    for (int u = 0; u < W; u++) j[u] = (u < nn) ? col[u * npad] : p;
  }
  for (int k = 0; k < nn; k += W) {
    if (DIAGP && (A.diag & 8)) {          // diagnostics: same arithmetic, gathers replaced by coalesced loads
#pragma unroll
      for (int u = 0; u < W; u++) j[u] = min(p + k + u + 1, A.n - 1);
    }
    const int g0 = k * LPB + sub;                                                       // list row of this lane's slot 0
    const bool mixed = __any(g0 < nb);                                                  // (bond entries come first)
    double4 r[W];
    int c[W];
    if (mixed) {
#pragma unroll
      for (int u = 0; u < W; u++) r[u] = A.pos[j[u] & (g0 + u * LPB < nb ? BOND_IDX_MASK : NEIGH_MASK)];
    } else {
#pragma unroll
      for (int u = 0; u < W; u++) r[u] = A.pos[j[u] & NEIGH_MASK];
    }
    const int kn = k + W;
#pragma unroll
    for (int u = 0; u < W; u++) { c[u] = j[u]; j[u] = (kn + u < nn) ? col[(size_t)(kn + u) * npad] : p; }
    if (mixed && AHEAD) {
      // small systems (one wavefront's chain of dependent work is what counts, registers are plentiful): unrolled
#pragma unroll
      for (int u = 0; u < W; u++) {
        if (g0 + u * LPB < nb) { if (bonds_on) bond_term<EFLAG, ALLSTYLES>(box, s_bt, p, ri, c[u], r[u], (unsigned)(bsh >> (BSHIFT_BITS * (g0 + u * LPB))) & 63u, A.bond_minimg != 0, fxi, fyi, fzi, e, flags); }
        else pair_term<EFLAG, MINIMG, UNIFORM, HAS_SB, SOFT>(A, box, s_tab, itype, ri, c[u], r[u], k + u < nn, fxi, fyi, fzi, e);
      }
    } else if (mixed) {
      // rolled over the slots (one copy of each body in the code; unrolled, the two bodies per slot cost ~20 registers)
#pragma unroll 1
      for (int u = 0; u < W; u++) {
        int cu = c[0];
        double4 ru = r[0];
#pragma unroll
        for (int w = 1; w < W; w++) if (u == w) { cu = c[w]; ru = r[w]; }
        if (g0 + u * LPB < nb) { if (bonds_on) bond_term<EFLAG, ALLSTYLES>(box, s_bt, p, ri, cu, ru, (unsigned)(bsh >> (BSHIFT_BITS * (g0 + u * LPB))) & 63u, A.bond_minimg != 0, fxi, fyi, fzi, e, flags); }
        else pair_term<EFLAG, MINIMG, UNIFORM, HAS_SB, SOFT>(A, box, s_tab, itype, ri, cu, ru, k + u < nn, fxi, fyi, fzi, e);
      }
    } else {
#pragma unroll
      for (int u = 0; u < W; u++)
        pair_term<EFLAG, MINIMG, UNIFORM, HAS_SB, SOFT>(A, box, s_tab, itype, ri, c[u], r[u], k + u < nn, fxi, fyi, fzi, e);
    }
  }
}

template <bool EFLAG, bool HAS_PAIR, int LPB, bool DIAG, bool AHEAD, bool ALLSTYLES = false, bool SOFT = false>
__device__ __forceinline__ void bead_force(const ForceArgs &A, const BondTable &bt, const Box &box,
                                           const double *__restrict__ s_tab, const double *__restrict__ s_bt, int p,
                                           int sub, const BeadPre &L, const double4 &ri, double &fxi, double &fyi,
                                           double &fzi, double (&e)[14], int *__restrict__ flags) {
  if (HAS_PAIR) {
    const int nall = (DIAG && (A.diag & 2)) ? 0 : min(L.nall & NN_COUNT_MASK, A.nn_limit);
    const int nb = min((L.nall >> NN_BOND_SHIFT) & NN_NBOND_MASK, nall);
    // frozen partner images: a word of the side table for the few beads that have a bond across a periodic face
    unsigned long long bsh = 0ull;
    if (L.nall & NN_SHIFTED_BIT) bsh = A.bshift[p];
    // wave-uniform choice: a wavefront whose 64 beads all sit deeper than `margin` inside the box skips
    // the minimum-image arithmetic of the pair terms (cell order makes most wavefronts interior)
    const double m = A.margin;
    bool interior = ri.x > box.lo[0] + m && ri.x < box.hi[0] - m && ri.y > box.lo[1] + m && ri.y < box.hi[1] - m &&
                    ri.z > box.lo[2] + m && ri.z < box.hi[2] - m;
    bool all_in = __all(interior);
#define LE_LOOP(MI, UN, SB) pair_loop<EFLAG, MI, UN, SB, LPB, AHEAD, DIAG, ALLSTYLES, SOFT>(A, box, s_tab, s_bt, p, sub, L, nall, nb, bsh, ri, fxi, fyi, fzi, e, flags)
    if (A.uniform && !A.has_sb) {
      if (all_in) LE_LOOP(false, true, false); else LE_LOOP(true, true, false);
    } else if (!A.has_sb) {
      if (all_in) LE_LOOP(false, false, false); else LE_LOOP(true, false, false);
    } else {
      LE_LOOP(true, false, true);
    }
#undef LE_LOOP
    return;
  }
  // no pair style (no list): the bonds come straight from the bond-partner table
  const int nbond = (DIAG && (A.diag & 1)) ? 0 : A.bpa;
  const unsigned long long bsh = A.bond_minimg ? 0ull : A.bshift[p];
  int slot = 0;                                    // the images are stored by compacted slot (k_bond_table)
  for (int m = 0; m < nbond; m++) {
    const int eb = A.bpart[(size_t)m * A.npad + p];
    if (eb < 0) continue;
    const int myslot = slot++;
    if ((m % LPB) != sub) continue;
    const double4 rj = A.pos[eb & BOND_IDX_MASK];
    bond_term<EFLAG, ALLSTYLES>(box, s_bt, p, ri, eb, rj, (unsigned)(bsh >> (BSHIFT_BITS * myslot)) & 63u, A.bond_minimg != 0, fxi, fyi, fzi, e, flags);
  }
}

// ------------------------------------------------------------------------------------------
// fix wall/region: the force of one wall on one bead (FixWallRegion::post_force for one atom).  Region::match first, then the
// contacts of the region's surface_interior / surface_exterior in their order - up to six for a block seen from inside, three
// for a cylinder -, each with fwall and eng of the style at the contact distance and fwall * del / r added to the force.  Plain
// IEEE arithmetic in the reference's operation order (this file is compiled without contraction; 1.0 / r is a divide).  The
// stored coordinates are taken as they are, the way the reference reads x[i] between reneighborings.  Every branch on the
// table is wave-uniform.  `acc` (EFLAG): eng, -fx, -fy, -fz, then fx*delx fy*dely fz*delz fx*dely fx*delz fy*delz.
// false: the bead does not match the region or sits on its surface (r <= 0) - it contributes nothing there, the caller raises
// ERR_WALL_OUTSIDE ("Particle outside surface of region used in fix wall/region")
template <bool EFLAG>
__device__ __forceinline__ bool wall_force(const double4 &x, const WallEntry &w, double &f0, double &f1, double &f2,
                                           double *__restrict__ acc) {
  const double cutoff = w.cutoff;
  const int kind = w.kind;
  const bool interior = w.interior != 0;
  // Region::match = !(inside ^ interior), closed surfaces; what the contacts below need is kept
  double d1 = 0.0, d2 = 0.0, rr = 0.0;       // sphere: rr = distance from the centre; cylinder: d1, d2, rr in the plane across the axis
  double xp = x.x, yp = x.y, zp = x.z;       // block from outside: the closest point of the block
  int nslots = 1;
  bool inside;
  if (kind == WALL_SPHERE) {
    const double delx = x.x - w.p[0], dely = x.y - w.p[1], delz = x.z - w.p[2];
    rr = sqrt(delx * delx + dely * dely + delz * delz);
    inside = rr <= w.p[3];
  } else if (kind == WALL_BLOCK) {
    inside = x.x >= w.p[0] && x.x <= w.p[1] && x.y >= w.p[2] && x.y <= w.p[3] && x.z >= w.p[4] && x.z <= w.p[5];
    if (interior) nslots = 6;
    else {
      if (x.x < w.p[0]) xp = w.p[0]; else if (x.x > w.p[1]) xp = w.p[1];
      if (x.y < w.p[2]) yp = w.p[2]; else if (x.y > w.p[3]) yp = w.p[3];
      if (x.z < w.p[4]) zp = w.p[4]; else if (x.z > w.p[5]) zp = w.p[5];
    }
  } else {
    const int ax = w.axis;
    const double a = ax == 0 ? x.x : ax == 1 ? x.y : x.z;
    d1 = (ax == 0 ? x.y : x.x) - w.p[0];
    d2 = (ax == 2 ? x.y : x.z) - w.p[1];
    rr = sqrt(d1 * d1 + d2 * d2);
    inside = rr <= w.p[2] && a >= w.p[3] && a <= w.p[4];
    nslots = 3;
  }
  if (inside != interior) return false;
  bool ok = true;
#pragma unroll 1
  for (int m = 0; m < nslots; m++) {
    double r, delx = 0.0, dely = 0.0, delz = 0.0;
    if (kind == WALL_SPHERE) {
      const double radius = w.p[3];
      if (interior && rr == 0.0) continue;           // (no contact at the centre)
      r = interior ? radius - rr : rr - radius;
      const double s = 1.0 - radius / rr;
      delx = (x.x - w.p[0]) * s; dely = (x.y - w.p[1]) * s; delz = (x.z - w.p[2]) * s;
    } else if (kind == WALL_BLOCK && interior) {
      // faces xlo xhi ylo yhi zlo zhi: delta = the distance, del = +-delta along the face's normal
      const int dim = m >> 1;
      const double c = dim == 0 ? x.x : dim == 1 ? x.y : x.z;
      r = (m & 1) ? w.p[m] - c : c - w.p[m];
      const double del = (m & 1) ? -r : r;
      if (dim == 0) delx = del; else if (dim == 1) dely = del; else delz = del;
    } else if (kind == WALL_BLOCK) {
      if (x.x <= w.p[0] - cutoff || x.x >= w.p[1] + cutoff || x.y <= w.p[2] - cutoff || x.y >= w.p[3] + cutoff ||
          x.z <= w.p[4] - cutoff || x.z >= w.p[5] + cutoff) continue;
      delx = x.x - xp; dely = x.y - yp; delz = x.z - zp;
      r = sqrt(delx * delx + dely * dely + delz * delz);
    } else {
      const int ax = w.axis;
      if (m == 0) {                                  // the curved surface, then the caps at lo and hi
        if (!(rr > 0.0)) continue;
        const double radius = w.p[2];
        r = radius - rr;
        const double s = 1.0 - radius / rr;
        const double e1 = d1 * s, e2 = d2 * s;
        if (ax == 0) { dely = e1; delz = e2; } else if (ax == 1) { delx = e1; delz = e2; } else { delx = e1; dely = e2; }
      } else {
        const double a = ax == 0 ? x.x : ax == 1 ? x.y : x.z;
        r = m == 1 ? a - w.p[3] : w.p[4] - a;
        const double del = m == 1 ? r : -r;
        if (ax == 0) delx = del; else if (ax == 1) dely = del; else delz = del;
      }
    }
    if (!(r < cutoff)) continue;
    if (r <= 0.0) { ok = false; continue; }          // on the surface: onflag, no force from this contact
    const double rinv = 1.0 / r;
    double fwall, eng = 0.0;
    const int style = w.style;
    if (style == WALL_LJ126) {
      const double r2inv = rinv * rinv;
      const double r6inv = r2inv * r2inv * r2inv;
      fwall = r6inv * (w.coeff[1] * r6inv - w.coeff[2]) * rinv;
      if (EFLAG) eng = r6inv * (w.coeff[3] * r6inv - w.coeff[4]) - w.offset;
    } else if (style == WALL_LJ93) {
      const double r2inv = rinv * rinv;
      const double r4inv = r2inv * r2inv;
      const double r10inv = r4inv * r4inv * r2inv;
      fwall = w.coeff[1] * r10inv - w.coeff[2] * r4inv;
      if (EFLAG) eng = w.coeff[3] * r4inv * r4inv * rinv - w.coeff[4] * r2inv * rinv - w.offset;
    } else if (style == WALL_LJ1043) {
      const double r2inv = rinv * rinv;
      const double r4inv = r2inv * r2inv;
      const double r10inv = r4inv * r4inv * r2inv;
      fwall = w.coeff[5] * r10inv * rinv - w.coeff[6] * r4inv * rinv - w.coeff[7] * pow(r + w.coeff[4], -4.0);
      if (EFLAG) eng = w.coeff[1] * r10inv - w.coeff[2] * r4inv - w.coeff[3] * pow(r + w.coeff[4], -3.0) - w.offset;
    } else if (style == WALL_MORSE) {
      const double dr = r - w.sigma;
      const double dexp = exp(-w.alpha * dr);
      fwall = w.coeff[1] * (dexp * dexp - dexp) / r;
      if (EFLAG) eng = w.epsilon * (dexp * dexp - 2.0 * dexp) - w.offset;
    } else {
      const double dr = cutoff - r;
      fwall = 2.0 * w.epsilon * dr;
      if (EFLAG) eng = w.epsilon * dr * dr;
    }
    const double fx = fwall * delx * rinv, fy = fwall * dely * rinv, fz = fwall * delz * rinv;
    f0 += fx; f1 += fy; f2 += fz;
    if (EFLAG) {
      acc[0] += eng; acc[1] -= fx; acc[2] -= fy; acc[3] -= fz;
      acc[4] += fx * delx; acc[5] += fy * dely; acc[6] += fz * delz;
      acc[7] += fx * dely; acc[8] += fx * delz; acc[9] += fy * delz;
    }
  }
  return ok;
}
// the walls of one place among the post-force fixes (`phase`: 0 before fix langevin or without one, 1 behind it) on a bead of
// group all - what the wall variant of the step kernel runs
__device__ __forceinline__ void walls_on_bead(const WallTable *__restrict__ wt, int phase, const double4 &x, double &f0, double &f1,
                                              double &f2, int *__restrict__ flags) {
  const int nw = wt->n;
#pragma unroll 1
  for (int k = 0; k < nw; k++) {
    const WallEntry &w = wt->w[k];
    if (w.after_langevin != phase) continue;
    if (!wall_force<false>(x, w, f0, f1, f2, nullptr)) flags[FLAG_ERROR] = ERR_WALL_OUTSIDE;
  }
}
// the unfused post-force kernel of fix wall/region: the walls of one `phase` added to f for the members of each wall's group;
// EFLAG: per wall the block sums of the ten columns of wall_force into rows of 16 (k_colsum<16> adds them up)
constexpr int WALL_COLS = 10;
template <bool EFLAG>
__global__ __launch_bounds__(BLOCK) void k_wall(int n, const double4 *__restrict__ pos, const int *__restrict__ tag,
                                                const int *__restrict__ gmask, const WallTable *__restrict__ wt, int phase,
                                                double *__restrict__ fx, double *__restrict__ fy, double *__restrict__ fz,
                                                double *__restrict__ partial, int rows, int *__restrict__ flags) {
  const int p = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = p < n;
  double4 x = make_double4(0.0, 0.0, 0.0, 0.0);
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  int gm = 1;
  if (live) {
    x = pos[p];
    f0 = fx[p]; f1 = fy[p]; f2 = fz[p];
    if (gmask) gm = gmask[tag[p]] | 1;
  }
  const int nw = wt->n;
  for (int k = 0; k < nw; k++) {
    const WallEntry &w = wt->w[k];
    if (w.after_langevin != phase) continue;
    double acc[WALL_COLS];
#pragma unroll
    for (int c = 0; c < WALL_COLS; c++) acc[c] = 0.0;
    if (live && (gm & w.groupbit))
      if (!wall_force<EFLAG>(x, w, f0, f1, f2, acc)) flags[FLAG_ERROR] = ERR_WALL_OUTSIDE;
    if (EFLAG) {
      block_reduce_store<WALL_COLS>(acc, partial + (size_t)k * rows * 16, blockIdx.x, 0);
      __syncthreads();       // (the next wall reuses the reduction's LDS)
    }
  }
  if (live) { fx[p] = f0; fy[p] = f1; fz[p] = f2; }
}

// fix indent (indent_inl.h): the indenters of one place among the post-force fixes on a bead of group all, in table order -
// what the indent variants of the step kernel run behind that place's walls.  The table is a kernel argument: n, the phases and
// the kinds are the same for every lane
__device__ __forceinline__ void indents_on_bead(const IndentTable &it, int phase, const double4 &x, const Box &box, double &f0,
                                                double &f1, double &f2) {
  const int ni = it.n;
#pragma unroll 1
  for (int k = 0; k < ni; k++) {
    const IndentEntry &o = it.e[k];
    if (o.phase != phase) continue;
    indent_force<false>(x.x, x.y, x.z, o, box, f0, f1, f2, nullptr);
  }
}
// the unfused post-force kernel of fix indent: the indenters of one `phase` added to f for the members of each fix's group;
// EFLAG: per indenter the block sums of the four columns of indent_force into rows of 16 (k_colsum<16> adds them up)
template <bool EFLAG>
__global__ __launch_bounds__(BLOCK) void k_indent(int n, const double4 *__restrict__ pos, const int *__restrict__ tag,
                                                  const int *__restrict__ gmask, IndentTable it, Box box, int phase,
                                                  double *__restrict__ fx, double *__restrict__ fy, double *__restrict__ fz,
                                                  double *__restrict__ partial, int rows) {
  const int p = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = p < n;
  double4 x = make_double4(0.0, 0.0, 0.0, 0.0);
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  int gm = 1;
  if (live) {
    x = pos[p];
    f0 = fx[p]; f1 = fy[p]; f2 = fz[p];
    if (gmask) gm = gmask[tag[p]] | 1;
  }
  const int ni = it.n;
  for (int k = 0; k < ni; k++) {
    const IndentEntry &o = it.e[k];
    if (o.phase != phase) continue;
    double acc[INDENT_COLS];
#pragma unroll
    for (int c = 0; c < INDENT_COLS; c++) acc[c] = 0.0;
    if (live && (gm & o.groupbit)) indent_force<EFLAG>(x.x, x.y, x.z, o, box, f0, f1, f2, acc);
    if (EFLAG) {
      block_reduce_store<INDENT_COLS>(acc, partial + (size_t)k * rows * 16, blockIdx.x, 0);
      __syncthreads();       // (the next indenter reuses the reduction's LDS)
    }
  }
  if (live) { fx[p] = f0; fy[p] = f1; fz[p] = f2; }
}

// ------------------------------------------------------------------------------------------
// fix spring/self | addforce | setforce: the entries [k0, k1) of the run's table that belong to `phase` (0 before fix langevin or
// without one, 1 behind it) and act on this step (`active`, bit k) applied to one bead, in table = fix order - setforce overwrites
// what the entries before it left, the foriginal sums of addforce and setforce see it.  `gm`: the bead's group bits with bit 0
// (all) set; `t`: its tag, which the origins go by.  Only a member of a tether, or of an addforce whose sums are wanted, reads its
// three image words, and only a tether's member its origin.  Plain IEEE arithmetic in the reference's operation order (this file
// is compiled without contraction): unwrap = x + image * prd (Domain::unmap), d = unwrap - origin, f -= K * d.
// `acc` (EFLAG), ten columns that the caller keeps per entry: spring/self  K * |d|^2 (the host halves the sum);  addforce
// -(f . unwrap), the force before the fix acted (3), f_a * unwrap_b xx yy zz xy xz yz;  setforce  the force before it acted (3)
template <bool EFLAG>
__device__ __forceinline__ void forceops_on_bead(const ForceOpTable *__restrict__ ft, int k0, int k1, int phase, unsigned active,
                                                 const double4 &x, int gm, int t, const int *__restrict__ img, int npad, int p,
                                                 const Box &box, double &f0, double &f1, double &f2, double *__restrict__ acc) {
  double u0 = 0.0, u1 = 0.0, u2 = 0.0;
  bool unwrapped = false;
#pragma unroll 1
  for (int k = k0; k < k1; k++) {
    const ForceOpEntry &o = ft->e[k];
    if (o.phase != phase || !((active >> k) & 1u) || !(gm & o.groupbit)) continue;
    const int kind = o.kind;
    if (!unwrapped && (kind == FORCEOP_SPRING || (EFLAG && kind == FORCEOP_ADD))) {
      u0 = x.x + img[p] * box.prd[0];
      u1 = x.y + img[npad + p] * box.prd[1];
      u2 = x.z + img[2 * (size_t)npad + p] * box.prd[2];
      unwrapped = true;
    }
    if (kind == FORCEOP_SPRING) {
      const double *__restrict__ og = o.origin + t;
      const size_t stride = (size_t)ft->stride;
      double dx = u0 - og[0], dy = u1 - og[stride], dz = u2 - og[2 * stride];
      const int m = o.mask;
      if (!(m & 1)) dx = 0.0;
      if (!(m & 2)) dy = 0.0;
      if (!(m & 4)) dz = 0.0;
      const double K = o.k;
      f0 -= K * dx; f1 -= K * dy; f2 -= K * dz;
      if (EFLAG) acc[0] += K * (dx * dx + dy * dy + dz * dz);
    } else if (kind == FORCEOP_ADD) {
      const double v0 = o.v[0], v1 = o.v[1], v2 = o.v[2];
      if (EFLAG) {
        acc[0] -= v0 * u0 + v1 * u1 + v2 * u2;
        acc[1] += f0; acc[2] += f1; acc[3] += f2;
        acc[4] += v0 * u0; acc[5] += v1 * u1; acc[6] += v2 * u2;
        acc[7] += v0 * u1; acc[8] += v0 * u2; acc[9] += v1 * u2;
      }
      f0 += v0; f1 += v1; f2 += v2;
    } else {
      if (EFLAG) { acc[1] += f0; acc[2] += f1; acc[3] += f2; }
      const int m = o.mask;
      if (m & 1) f0 = o.v[0];
      if (m & 2) f1 = o.v[1];
      if (m & 4) f2 = o.v[2];
    }
  }
}
// the unfused post-force kernel of the three: the entries of one `phase` applied to f in table order; EFLAG: per entry the block
// sums of the ten columns into rows of 16 (k_colsum<16> adds them up).  An entry that does not act on this step leaves its rows
// as they are
template <bool EFLAG>
__global__ __launch_bounds__(BLOCK) void k_fixforce(int n, int npad, const double4 *__restrict__ pos, const int *__restrict__ tag,
                                                    const int *__restrict__ gmask, const int *__restrict__ img, Box box,
                                                    const ForceOpTable *__restrict__ ft, int phase, unsigned active,
                                                    double *__restrict__ fx, double *__restrict__ fy, double *__restrict__ fz,
                                                    double *__restrict__ partial, int rows) {
  const int p = blockIdx.x * BLOCK + threadIdx.x;
  const bool live = p < n;
  double4 x = make_double4(0.0, 0.0, 0.0, 0.0);
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  int gm = 1, t = 0;
  if (live) {
    x = pos[p];
    f0 = fx[p]; f1 = fy[p]; f2 = fz[p];
    t = tag[p];
    if (gmask) gm = gmask[t] | 1;
  }
  const int nk = ft->n;
  for (int k = 0; k < nk; k++) {
    if (ft->e[k].phase != phase || !((active >> k) & 1u)) continue;      // (the same for every lane of the grid)
    double acc[FORCEOP_COLS];
#pragma unroll
    for (int c = 0; c < FORCEOP_COLS; c++) acc[c] = 0.0;
    if (live) forceops_on_bead<EFLAG>(ft, k, k + 1, phase, active, x, gm, t, img, npad, p, box, f0, f1, f2, acc);
    if (EFLAG) {
      block_reduce_store<FORCEOP_COLS>(acc, partial + (size_t)k * rows * 16, blockIdx.x, 0);
      __syncthreads();       // (the next entry reuses the reduction's LDS)
    }
  }
  if (live) { fx[p] = f0; fy[p] = f1; fz[p] = f2; }
}

// forces only (setup, thermo steps, runs without the standard nve+langevin pair of fixes)
// NOBOND: the bond entries at the head of the lists are skipped (run_style respa with pair and bond forces on different levels)
template <bool EFLAG, bool HAS_PAIR, bool NOBOND = false, bool SOFT = false>
__global__ __launch_bounds__(BLOCK) void k_force(ForceArgs A, BondTable bt, Box box, double *__restrict__ fx,
                                                 double *__restrict__ fy, double *__restrict__ fz,
                                                 double *__restrict__ partial, int *__restrict__ flags) {
  __shared__ double s_tab[6 * (MAXTYPES + 1) * (MAXTYPES + 1)];
  __shared__ double s_bt[(MAXTYPES + 1) * BT_W];
  fill_bond_table(bt, s_bt);
  if (HAS_PAIR && !(A.uniform && !A.has_sb))     // one coefficient set and no fractional special weights: scalars, no table
    for (int k = threadIdx.x; k < 6 * A.nt * A.nt; k += BLOCK) s_tab[k] = A.pairtab[k];
  __syncthreads();
  int lb = logical_block(A.nblocks);
  int p = lb * BLOCK + threadIdx.x;
  double e[14];
#pragma unroll
  for (int k = 0; k < 14; k++) e[k] = 0.0;
  if (lb < A.nblocks && p < A.n) {
    double4 ri = A.pos[p];
    const BeadPre L = bead_preload<HAS_PAIR, 1, true>(A, p, 0);
    double fxi = 0.0, fyi = 0.0, fzi = 0.0;
    bead_force<EFLAG, HAS_PAIR, 1, NOBOND, true, true, SOFT>(A, bt, box, s_tab, s_bt, p, 0, L, ri, fxi, fyi, fzi, e, flags);   // (DIAG = NOBOND: A.diag = 1 switches the bonds off)
    fx[p] = fxi; fy[p] = fyi; fz[p] = fzi;
  }
  if (EFLAG && lb < A.nblocks) block_reduce_store<14>(e, partial, lb, 0);
}

// the whole force-side of a timestep in ONE pass over the beads:
//   f(x_n) -> [+ Langevin drag/random, 3 draws by canonical rank] -> final half-kick (FixNVE::final_integrate)
//   -> [NEXT: first half-kick + drift of step n+1 (FixNVE::initial_integrate) into the second position
//       buffer + the skin/2 displacement test of Neighbor::check_distance]
// x, v never round-trip through HBM between these stages and f is only stored when a later kernel needs it.
// LPB (lanes per bead) = 4 is the small-system variant: below ~10^5 beads the kernel is not bound by throughput but by
// the chain of dependent loads ONE wavefront walks (index -> position, five stages deep for 18 neighbors, then the
// bonds one after the other: 10 us at 32k beads whatever the chip could stream).  Four lanes share a bead, each takes
// every fourth list entry and every fourth bond slot, the partial forces meet in a two-step butterfly and lane 0
// integrates: the chain shrinks to one or two stages.
// ANG: runs with an angle style - the angle forces of this step were written into fx / fy / fz by k_angle<.., OVERWRITE>
// right before this launch and are added to the bead's sums (a bit of the kernel's key, not a run-time test: the step kernel's
// schedule is sensitive - a pointer test here cost every run 2 us per launch)
#define ANGLE_SMALL 0.001
// the listed angles of one bead (records of k_angle_list): its own share of every one - f1 as atom 1, -(f1 + f3) as the
// centre, f3 as atom 3 - and, EFLAG, a third of the energy / virial each (Angle::ev_tally, newton_bond off)
template <bool EFLAG, typename TABLE>
__device__ __forceinline__ void bead_angles(int p, const double4 &rp, int na, const int4 *__restrict__ rec, int npad,
                                            const double4 *__restrict__ pos, const Box &box, const TABLE &at, double &f0, double &f1v,
                                            double &f2, double (&acc)[8]) {
  for (int m = 0; m < na; m++) {
    const int4 r = rec[(size_t)m * npad + p];
    const int type = r.x;
    if (type <= 0 || at.style[type] == 0) continue;
    const int p1 = r.y, p2 = r.z, p3 = r.w;
    const double4 r1 = (p1 == p) ? rp : pos[p1], r2 = (p2 == p) ? rp : pos[p2], r3 = (p3 == p) ? rp : pos[p3];
    double delx1 = r1.x - r2.x, dely1 = r1.y - r2.y, delz1 = r1.z - r2.z;
    double delx2 = r3.x - r2.x, dely2 = r3.y - r2.y, delz2 = r3.z - r2.z;
    const double hx = box.half[0], hy = box.half[1], hz = box.half[2];
    if (delx1 > hx) delx1 -= box.prd[0]; else if (delx1 < -hx) delx1 += box.prd[0];
    if (dely1 > hy) dely1 -= box.prd[1]; else if (dely1 < -hy) dely1 += box.prd[1];
    if (delz1 > hz) delz1 -= box.prd[2]; else if (delz1 < -hz) delz1 += box.prd[2];
    if (delx2 > hx) delx2 -= box.prd[0]; else if (delx2 < -hx) delx2 += box.prd[0];
    if (dely2 > hy) dely2 -= box.prd[1]; else if (dely2 < -hy) dely2 += box.prd[1];
    if (delz2 > hz) delz2 -= box.prd[2]; else if (delz2 < -hz) delz2 += box.prd[2];
    const double rsq1 = delx1 * delx1 + dely1 * dely1 + delz1 * delz1, ra = sqrt(rsq1);
    const double rsq2 = delx2 * delx2 + dely2 * dely2 + delz2 * delz2, rb = sqrt(rsq2);
    double cs = delx1 * delx2 + dely1 * dely2 + delz1 * delz2;
    cs /= ra * rb;
    if (cs > 1.0) cs = 1.0;
    if (cs < -1.0) cs = -1.0;
    double a, eangle = 0.0;
    if (at.style[type] == 1) {
      double sn = sqrt(1.0 - cs * cs);
      if (sn < ANGLE_SMALL) sn = ANGLE_SMALL;
      sn = 1.0 / sn;
      const double dtheta = acos(cs) - at.theta0[type], tk = at.k[type] * dtheta;
      if (EFLAG) eangle = tk * dtheta;
      a = -2.0 * tk * sn;
    } else {
      if (EFLAG) eangle = at.k[type] * (1.0 + cs);
      a = at.k[type];
    }
    const double a11 = a * cs / rsq1, a12 = -a / (ra * rb), a22 = a * cs / rsq2;
    const double f1x = a11 * delx1 + a12 * delx2, f1y = a11 * dely1 + a12 * dely2, f1z = a11 * delz1 + a12 * delz2;
    const double f3x = a22 * delx2 + a12 * delx1, f3y = a22 * dely2 + a12 * dely1, f3z = a22 * delz2 + a12 * delz1;
    if (p == p1) { f0 += f1x; f1v += f1y; f2 += f1z; }
    else if (p == p2) { f0 -= f1x + f3x; f1v -= f1y + f3y; f2 -= f1z + f3z; }
    else { f0 += f3x; f1v += f3y; f2 += f3z; }
    if (EFLAG) {
      const double third = 1.0 / 3.0;
      acc[0] += third * eangle;
      acc[1] += third * (delx1 * f1x + delx2 * f3x); acc[2] += third * (dely1 * f1y + dely2 * f3y);
      acc[3] += third * (delz1 * f1z + delz2 * f3z); acc[4] += third * (delx1 * f1y + delx2 * f3y);
      acc[5] += third * (delx1 * f1z + delx2 * f3z); acc[6] += third * (dely1 * f1z + dely2 * f3z);
    }
  }
}

// EF: a thermo step - the same pass also sums the energies and the virial of the pair and bond terms into `partial`
// (rows of 16 per block, as k_force<EFLAG> writes them), so that a step with thermo output is not a pass of k_force
// plus a Langevin / integrate kernel.  Only for NEXT = false, one lane per bead (the velocities thermo reads are those
// after final_integrate).
// GRP: fix nve and / or fix langevin act on a group (`mask[i] & groupbit`, src/fix_nve.cpp:82, src/fix_langevin.cpp:661): a bead
// outside fix nve's group keeps its position and velocity (its force is still computed - others feel it), a bead outside fix
// langevin's group gets neither drag nor noise and draws nothing; `ranks` is then the rank table the draws go by (the rank among
// the members when the thermostat is on a group)
// LAZYV: the first launch after a rebuild that left the velocities in the old order (DeviceState::v_pending) - bead p reads its
// velocity at vperm[p] and stores it at p of vxo / vyo / vzo: the velocity permutation costs this launch one index per bead
// instead of the rebuild 48 bytes per bead
// WALL: fix wall/region on group all (wall_force): the walls defined before fix langevin add their force before drag and noise,
// the ones behind it after - the order the reference's post_force hooks run in; the wall needs nothing but the bead's own
// position, which is in registers here (four lanes per bead: lane 0, behind the butterfly)
// INDENT: fix indent on group all (indent_force) on top of WALL, behind the walls of each place; a run with indenters alone
// carries a wall table with n = 0.  A flag of its own: sharing WALL's made wall-only runs 3.7 % slower (fix indent)
// EXT: fix spring/self, addforce, setforce (forceops_on_bead) at their place among the post-force fixes, as the walls; the bead's
// group bits come by tag (not loaded when every entry is on group all), its images and origin only if it is a member
// The parameters from `tag` on are the members of S and k_step's five direct pointers once more, __restrict__-qualified: the
// loads of level 0 / level 1 below and of the AHEAD shapes move ahead of the stores into `flags` only with it (StepKernelArgs).
// Read straight from S here, the members give 2 instantiations other VGPR counts and the wall variants vector loads of their table.
template <int KEY>
__device__ __forceinline__ void step_body(const ForceArgs &A, const BondTable &bt, const Box &box, const TypeTables &tt, const StepKernelArgs &S,
                                          const double *s_tab, const double *s_bt,
                                          const int *__restrict__ tag, const int *__restrict__ crank,
                                          const uint32_t *__restrict__ draws, double *__restrict__ vx,
                                          double *__restrict__ vy, double *__restrict__ vz,
                                          double *__restrict__ fx, double *__restrict__ fy,
                                          double *__restrict__ fz, double4 *__restrict__ pos_next,
                                          const double4 *__restrict__ xhold, double dtv, double triggersq,
                                          int check, int *__restrict__ flags,
                                          const unsigned char *__restrict__ phase, int which, double (&e)[14], double &ke,
                                          const int *__restrict__ gmask, int nvebit, int lgbit,
                                          const int *__restrict__ vperm, double *__restrict__ vxo,
                                          double *__restrict__ vyo, double *__restrict__ vzo,
                                          const WallTable *__restrict__ wt, const IndentTable &indents) {
  constexpr bool LANGEVIN = KEY & SK_LANGEVIN, NEXT = KEY & SK_NEXT, IDENT = KEY & SK_IDENT, HAS_PAIR = KEY & SK_PAIR, DIAG = KEY & SK_DIAG,
                 AHEAD = KEY & SK_AHEAD, ANG = KEY & SK_ANG, EF = KEY & SK_EF, GRP = KEY & SK_GRP, LAZYV = KEY & SK_LAZYV,
                 WALL = KEY & SK_WALL, SOFT = KEY & SK_SOFT, EXT = KEY & SK_EXT, INDENT = KEY & SK_INDENT;
  constexpr int LPB = (KEY & SK_LPB4) ? 4 : 1;      // lanes per bead
  int lb = logical_block(A.nblocks);
  const int sub = (LPB == 1) ? 0 : (int)(threadIdx.x % LPB);
  int p = lb * (BLOCK / LPB) + threadIdx.x / LPB;
  if (lb >= A.nblocks || p >= A.n) return;         // (the LPB lanes of a bead always leave together)
  if (which >= 0 && phase[p] != which) return;     // decomposed runs: this launch handles one phase of the step
  // a list of the build this launch follows did not fit: the host has not looked yet (Engine::reneighbor defers the
  // check behind this kernel); store nothing, it will rebuild and launch again
  // ---- level 0: all loads addressed by p, issued back to back before any of them is used ----
  double4 ri = A.pos[p];
  int pv = p;
  if (LAZYV) pv = vperm[p];
  double a = vx[pv], b = vy[pv], c = vz[pv];
  int t = 0;
  if (LANGEVIN || GRP || EXT) t = tag[p];
  const BeadPre L = bead_preload<HAS_PAIR, LPB, AHEAD>(A, p, sub);
  double4 hold = ri;
  if (AHEAD && NEXT && check) hold = xhold[p];
  const int poisoned = flags[FLAG_NEIGH_OVERFLOW];
  // ---- level 1: the draws (by canonical rank), then - inside bead_force - the partners' positions ----
  uint32_t d0 = 0, d1 = 0, d2 = 0;
  bool m_nve = true, m_lg = true;
  if (GRP) {
    const int gm = gmask[t];
    m_nve = nvebit == 1 || (gm & nvebit);
    m_lg = lgbit == 1 || (gm & lgbit);
  }
  int gm_ext = 1;
  if (EXT && gmask) gm_ext = gmask[t] | 1;
  if (LANGEVIN && !(DIAG && (A.diag & 4)) && (!GRP || m_lg)) {
    int rank = IDENT ? (t - 1) : crank[t];
    d0 = draws[3 * (size_t)rank]; d1 = draws[3 * (size_t)rank + 1]; d2 = draws[3 * (size_t)rank + 2];
  }
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  bead_force<EF, HAS_PAIR, LPB, DIAG, AHEAD, false, SOFT>(A, bt, box, s_tab, s_bt, p, sub, L, ri, f0, f1, f2, e, flags);
  if (LPB > 1) {
#pragma unroll
    for (int o = 1; o < LPB; o <<= 1) { f0 += __shfl_xor(f0, o); f1 += __shfl_xor(f1, o); f2 += __shfl_xor(f2, o); }
    if (sub) return;
  }
  if (ANG && !NEXT) { f0 += fx[p]; f1 += fy[p]; f2 += fz[p]; }     // Angle::compute follows Bond::compute (k_angle wrote them)
  if (ANG && NEXT) {
    // whole steps of a run with an angle style evaluate the bead's listed angles right here; a NEXT launch stores no forces,
    // so its three force pointers carry the angle data instead: records, counts, coefficient table (launch_step)
    double acc8[8];
    bead_angles<false>(p, ri, S.angle_n[p], S.angle_rec, A.npad, A.pos, box, *S.angles, f0, f1, f2, acc8);
  }
  const int type = (int)ri.w;
  // (a bead outside its region raises the error flag here, ahead of the `poisoned` test below: a launch that is discarded and
  //  repeated after a list overflow reports it one launch early, from the same positions the repeated launch reads)
  if (WALL) walls_on_bead(wt, 0, ri, f0, f1, f2, flags);
  if (INDENT) indents_on_bead(indents, 0, ri, box, f0, f1, f2);
  if (EXT) forceops_on_bead<false>(S.ext, 0, S.ext->n, 0, S.ext_active, ri, gm_ext, t, S.img, A.npad, p, box, f0, f1, f2, nullptr);
  if (LANGEVIN && (!GRP || m_lg)) {
    double gamma1 = tt.g1[type], gamma2 = tt.g2[type];
    const double inv = 1.0 / 16777216.0;
    double r0 = (double)d0 * inv;
    double r1 = (double)d1 * inv;
    double r2 = (double)d2 * inv;
    double fran0 = gamma2 * (r0 - 0.5), fran1 = gamma2 * (r1 - 0.5), fran2 = gamma2 * (r2 - 0.5);
    double fdrag0 = gamma1 * a, fdrag1 = gamma1 * b, fdrag2 = gamma1 * c;
    f0 += fdrag0 + fran0;
    f1 += fdrag1 + fran1;
    f2 += fdrag2 + fran2;
  }
  if (WALL && LANGEVIN) walls_on_bead(wt, 1, ri, f0, f1, f2, flags);
  if (INDENT && LANGEVIN) indents_on_bead(indents, 1, ri, box, f0, f1, f2);
  if (EXT && LANGEVIN) forceops_on_bead<false>(S.ext, 0, S.ext->n, 1, S.ext_active, ri, gm_ext, t, S.img, A.npad, p, box, f0, f1, f2, nullptr);
  if (poisoned) return;
  const double dtfm = tt.dtfm[type];
  if (!GRP || m_nve) { a += dtfm * f0; b += dtfm * f1; c += dtfm * f2; }          // final_integrate of this step
  if (EF) ke = (a * a + b * b + c * c) * tt.mass[type];    // the kinetic energy thermo reads (k_ke's term, column 14)
  if (NEXT) {
    if (!GRP || m_nve) {
      a += dtfm * f0; b += dtfm * f1; c += dtfm * f2;        // initial_integrate of the next step
      ri.x += dtv * a; ri.y += dtv * b; ri.z += dtv * c;
    }
    pos_next[p] = ri;
    if (A.sendslot) {
      const int sl = A.sendslot[p];
      if (sl >= 0) ((sl >> 30) ? A.send_up : A.send_dn)[sl & ((1 << 30) - 1)] = ri;
      else if (sl <= -2) {      // a slab below two ghost cutoffs: this bead is a ghost of both neighbours
        const int *__restrict__ b = A.sendslot + A.npad + 2 * (size_t)(-2 - sl);
        A.send_dn[b[0]] = ri;
        A.send_up[b[1]] = ri;
      }
    }
    if (check) {
      // Neighbor::check_distance.  Throughput shape: the float copy of the build-time positions (posf, 16 B, what the
      // list build reads anyway) decides unless the squared displacement lies within an error band of skin^2/4; only
      // then is the double reference fetched, so the flag is the one the FP64 test sets (32 MB less per test at 1M).
      bool moved;
      if (!AHEAD && A.holdf) {
        const float4 hf = A.holdf[p];
        double dx = ri.x - (double)hf.x, dy = ri.y - (double)hf.y, dz = ri.z - (double)hf.z;
        const double dsq = dx * dx + dy * dy + dz * dz;
        moved = dsq > triggersq;
        if (fabs(dsq - triggersq) < A.hold_band) {
          const double4 h = xhold[p];
          dx = ri.x - h.x; dy = ri.y - h.y; dz = ri.z - h.z;
          moved = dx * dx + dy * dy + dz * dz > triggersq;
        }
      } else {
        const double4 h = AHEAD ? hold : xhold[p];
        double dx = ri.x - h.x, dy = ri.y - h.y, dz = ri.z - h.z;
        moved = dx * dx + dy * dy + dz * dz > triggersq;
      }
      if (moved && !(DIAG && A.diag)) flags[FLAG_MOVED] = 1;
      if (!DIAG && A.bin) {     // (wave-uniform; the lanes still here: every LPB-th one up to the end of the array)
        double4 w = ri;
        int cell = 0;
        if (isfinite(w.x) && isfinite(w.y) && isfinite(w.z)) {
          int dix, diy, diz;
          wrap_into_box(w, box, dix, diy, diz);
          cell = cell_index(w, box, A.ncx, A.ncy, A.ncz, A.cix, A.ciy, A.ciz, A.zlo_ext, A.rtile);
        } else flags[FLAG_ERROR] = ERR_NONFINITE;
        A.cell_of[p] = cell;
        A.cell_rank[p] = count_into_cell<LPB>(cell, A.cell_count);
      }
    }
  } else {
    fx[p] = f0; fy[p] = f1; fz[p] = f2;
  }
  if (DIAG && (A.diag & 64)) { if (a == 1.2345e300) vx[p] = a; return; }   // diagnostic launch: v is left alone (the value is still computed)
  if (LAZYV) { vxo[p] = a; vyo[p] = b; vzo[p] = c; }
  else { vx[p] = a; vy[p] = b; vz[p] = c; }
}
// KEY: the instantiation, as the bits of step_plan.h (StepKeyBit) - a kernel trace shows k_step<1039>, and
// `python tests/step_census.py 1039` says which flags that is
template <int KEY>
__global__ __launch_bounds__(BLOCK, ((KEY & (SK_AHEAD | SK_EF)) ? 1 : STEP_WAVES_PER_SIMD)) void k_step(ForceArgs A, BondTable bt, Box box, TypeTables tt,
                                                                                                    StepKernelArgs S, double *__restrict__ fx,
                                                                                                    double *__restrict__ fy, double *__restrict__ fz,
                                                                                                    double4 *__restrict__ pos_next,
                                                                                                    const double4 *__restrict__ xhold) {
  // (fx, fy, fz: stored by launches without NEXT, read first when ANG && !NEXT; why these five are not members: StepKernelArgs)
  static_assert(sizeof(ForceArgs) + sizeof(BondTable) + sizeof(Box) + sizeof(TypeTables) + sizeof(StepKernelArgs) <= 4096,
                "the by-value arguments of k_step exceed the 4 KiB kernel-argument limit");
  static_assert(step_variant_exists(KEY), "no such variant of the step kernel (step_plan.h)");
  constexpr bool EF = KEY & SK_EF, HAS_PAIR = KEY & SK_PAIR;
  __shared__ double s_tab[6 * (MAXTYPES + 1) * (MAXTYPES + 1)];
  __shared__ double s_bt[(MAXTYPES + 1) * BT_W];
  fill_bond_table(bt, s_bt);
  if (HAS_PAIR && !(A.uniform && !A.has_sb))     // one coefficient set and no fractional special weights: scalars, no table
    for (int k = threadIdx.x; k < 6 * A.nt * A.nt; k += BLOCK) s_tab[k] = A.pairtab[k];
  __syncthreads();
  double e[14];
  double kev[1] = {0.0};
  if (EF) {
#pragma unroll
    for (int k = 0; k < 14; k++) e[k] = 0.0;
  }
  step_body<KEY>(
      A, bt, box, tt, S, s_tab, s_bt, S.tag, S.ranks, S.draws, S.vx, S.vy, S.vz, fx, fy, fz, pos_next, xhold, S.dtv, S.triggersq, S.check, S.flags,
      S.phase, S.which, e, kev[0], S.gmask, S.nvebit, S.lgbit, S.vperm, S.vxo, S.vyo, S.vzo, S.walls, S.indents);
  if (EF) {
    const int lb = logical_block(A.nblocks);
    if (lb < A.nblocks) {
      block_reduce_store<14>(e, S.partial, lb, 0);
      block_reduce_store<1>(kev, S.partial, lb, 14);
    }
  }
}

// ------------------------------------------------------------------------------------------
// `groupbit` != 1: the fix acts on a group (DeviceState::gmask by tag)
void launch_initial_integrate(DeviceState &d, const TypeTables &tt, double dtv, double triggersq, bool check, int groupbit) {
  int nb = (d.n + BLOCK - 1) / BLOCK;
  note_positions_replaced(d);     // the positions move
  settle_velocities(d);
  hipLaunchKernelGGL(k_initial_integrate, dim3(nb), dim3(BLOCK), 0, d.stream, d.n, d.pos, d.v[0], d.v[1], d.v[2],
                     d.f[0], d.f[1], d.f[2], d.xhold, tt, dtv, triggersq, check ? 1 : 0, d.flags, d.tag,
                     groupbit != 1 ? d.gmask : (const int *)nullptr, groupbit);
}
void launch_final_integrate(DeviceState &d, const TypeTables &tt, int groupbit) {
  int nb = (d.n + BLOCK - 1) / BLOCK;
  settle_velocities(d);
  hipLaunchKernelGGL(k_final_integrate, dim3(nb), dim3(BLOCK), 0, d.stream, d.n, d.pos, d.v[0], d.v[1], d.v[2],
                     d.f[0], d.f[1], d.f[2], tt, d.tag, groupbit != 1 ? d.gmask : (const int *)nullptr, groupbit);
}
// fix langevin `zero yes` (src/fix_langevin.cpp:725-729, 752-772): the members' random forces summed (block sums, then one
// workgroup adds them in block order and divides by the member count), and the mean taken off every member's force
template <bool IDENT>
__global__ __launch_bounds__(BLOCK) void k_langevin_fsum(int n, const double4 *__restrict__ pos, const int *__restrict__ tag,
                                                         const int *__restrict__ crank, const uint32_t *__restrict__ draws,
                                                         TypeTables tt, const int *__restrict__ gmask, int groupbit,
                                                         double *__restrict__ partial) {
  int p = blockIdx.x * BLOCK + threadIdx.x;
  double val[3] = {0.0, 0.0, 0.0};
  if (p < n) {
    int t = tag[p];
    if (!gmask || (gmask[t] & groupbit)) {
      int rank = IDENT ? (t - 1) : crank[t];
      double gamma2 = tt.g2[(int)pos[p].w];
      const double inv = 1.0 / 16777216.0;
      for (int k = 0; k < 3; k++) val[k] = gamma2 * ((double)draws[3 * (size_t)rank + k] * inv - 0.5);
    }
  }
  block_reduce_store<3>(val, partial, blockIdx.x, 0);
}
__global__ __launch_bounds__(BLOCK) void k_langevin_fsum_total(int nblocks, double inv_count, double *__restrict__ partial) {
  // one workgroup: thread k < 3 walks column k in block order (the same sum on every run)
  if (threadIdx.x < 3) {
    double s = 0.0;
    for (int b = 0; b < nblocks; b++) s += partial[(size_t)b * 16 + threadIdx.x];
    partial[(size_t)nblocks * 16 + threadIdx.x] = s * inv_count;
  }
}
__global__ __launch_bounds__(BLOCK) void k_langevin_zero(int n, const int *__restrict__ tag, const int *__restrict__ gmask,
                                                         int groupbit, const double *__restrict__ mean,
                                                         double *__restrict__ fx, double *__restrict__ fy,
                                                         double *__restrict__ fz) {
  int p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= n) return;
  if (gmask && !(gmask[tag[p]] & groupbit)) return;
  fx[p] -= mean[0]; fy[p] -= mean[1]; fz[p] -= mean[2];
}
// `host_sum3` (decomposed runs): this rank's three sums come back to the host instead, nothing is applied; the caller adds
// the ranks' sums and hands the mean to launch_langevin_zero_apply
void launch_langevin_zero(DeviceState &d, const TypeTables &tt, bool ident, int groupbit, long members, double *host_sum3) {
  int nb = std::max(1, (d.n + BLOCK - 1) / BLOCK);
  const int *gm = groupbit != 1 ? d.gmask : (const int *)nullptr;
  const int *rk = groupbit != 1 ? d.lgrank : d.crank;
  if (groupbit != 1) ident = false;
  with_flags([&](auto I) {
    hipLaunchKernelGGL((k_langevin_fsum<I>), dim3(nb), dim3(BLOCK), 0, d.stream, d.n, d.pos, d.tag, rk, d.rng_out, tt, gm,
                       groupbit, d.lgsum);
  }, ident);
  hipLaunchKernelGGL(k_langevin_fsum_total, dim3(1), dim3(BLOCK), 0, d.stream, nb, host_sum3 ? 1.0 : 1.0 / (double)members, d.lgsum);
  if (host_sum3) {
    HIP_CHECK(hipMemcpyAsync(d.partial_h, d.lgsum + (size_t)nb * 16, 3 * sizeof(double), hipMemcpyDeviceToHost, d.stream));
    stream_sync(d);
    for (int k = 0; k < 3; k++) host_sum3[k] = d.partial_h[k];
    return;
  }
  hipLaunchKernelGGL(k_langevin_zero, dim3(nb), dim3(BLOCK), 0, d.stream, d.n, d.tag, gm, groupbit,
                     d.lgsum + (size_t)nb * 16, d.f[0], d.f[1], d.f[2]);
}
void launch_langevin_zero_apply(DeviceState &d, int groupbit, const double *mean3) {
  int nb = std::max(1, (d.n + BLOCK - 1) / BLOCK);
  const int *gm = groupbit != 1 ? d.gmask : (const int *)nullptr;
  for (int k = 0; k < 3; k++) d.partial_h[k] = mean3[k];
  HIP_CHECK(hipMemcpyAsync(d.lgsum + (size_t)nb * 16, d.partial_h, 3 * sizeof(double), hipMemcpyHostToDevice, d.stream));
  hipLaunchKernelGGL(k_langevin_zero, dim3(nb), dim3(BLOCK), 0, d.stream, d.n, d.tag, gm, groupbit,
                     d.lgsum + (size_t)nb * 16, d.f[0], d.f[1], d.f[2]);
  stream_sync(d);          // (partial_h is reused by the next reduction)
}
void launch_langevin(DeviceState &d, const TypeTables &tt, bool ident, bool fuse_final, int groupbit) {
  int nb = (d.n + BLOCK - 1) / BLOCK;
  const int *gm = groupbit != 1 ? d.gmask : (const int *)nullptr;
  const int *rk = groupbit != 1 ? d.lgrank : d.crank;       // rank among the members of the group
  if (groupbit != 1) ident = false;
  settle_velocities(d);
  with_flags([&](auto F, auto I) {
    hipLaunchKernelGGL((k_langevin<F, I>), dim3(nb), dim3(BLOCK), 0, d.stream, d.n, d.pos, d.tag, rk,
                       d.rng_out, d.v[0], d.v[1], d.v[2], d.f[0], d.f[1], d.f[2], tt, gm, groupbit);
  }, fuse_final, ident);
}
// run_style respa: FixRespa's per-level force arrays (src/fix_respa.cpp), kept by tag so that the cell sort of a rebuild
// does not have to carry them; to_level: flevel[tag[p]] = f[p], else f[p] = flevel[tag[p]] (+= when `add`)
__global__ __launch_bounds__(BLOCK) void k_flevel_copy(int n, const int *__restrict__ tag, double *__restrict__ fx,
                                                       double *__restrict__ fy, double *__restrict__ fz,
                                                       double *__restrict__ flevel, int to_level, int add) {
  int p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= n) return;
  double *row = flevel + 3 * (size_t)tag[p];
  if (to_level) { row[0] = fx[p]; row[1] = fy[p]; row[2] = fz[p]; }
  else if (add) { fx[p] += row[0]; fy[p] += row[1]; fz[p] += row[2]; }
  else { fx[p] = row[0]; fy[p] = row[1]; fz[p] = row[2]; }
}
void launch_flevel_copy(DeviceState &d, double *flevel, bool to_level, bool add) {
  int nb = (d.n + BLOCK - 1) / BLOCK;
  hipLaunchKernelGGL(k_flevel_copy, dim3(nb), dim3(BLOCK), 0, d.stream, d.n, d.tag, d.f[0], d.f[1], d.f[2], flevel,
                     to_level ? 1 : 0, add ? 1 : 0);
}
// kinetic-energy tensor sum(m v_i v_j), order xx yy zz xy xz yz (ComputeTemp::compute_vector, src/compute_temp.cpp:108-140):
// block sums into the scratch rows of DeviceState::lgsum, added on the host in block order
__global__ __launch_bounds__(BLOCK) void k_ke_tensor(int n, const double4 *__restrict__ pos, const double *__restrict__ vx,
                                                     const double *__restrict__ vy, const double *__restrict__ vz,
                                                     TypeTables tt, double *__restrict__ partial) {
  int p = blockIdx.x * BLOCK + threadIdx.x;
  double val[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (p < n) {
    double a = vx[p], b = vy[p], c = vz[p], m = tt.mass[(int)pos[p].w];
    val[0] = m * a * a; val[1] = m * b * b; val[2] = m * c * c;
    val[3] = m * a * b; val[4] = m * a * c; val[5] = m * b * c;
  }
  block_reduce_store<6>(val, partial, blockIdx.x, 0);
}
void ke_tensor(DeviceState &d, const TypeTables &tt, double *out6) {
  const int nb = std::max(1, (d.n + BLOCK - 1) / BLOCK);
  settle_velocities(d);
  hipLaunchKernelGGL(k_ke_tensor, dim3(nb), dim3(BLOCK), 0, d.stream, d.n, d.pos, d.v[0], d.v[1], d.v[2], tt, d.lgsum);
  hipLaunchKernelGGL((k_colsum<16>), dim3(1), dim3(BLOCK), 0, d.stream, nb, d.lgsum, d.lgsum + (size_t)nb * 16);
  HIP_CHECK(hipMemcpyAsync(d.partial_h, d.lgsum + (size_t)nb * 16, 16 * sizeof(double), hipMemcpyDeviceToHost, d.stream));
  stream_sync(d);
  for (int k = 0; k < 6; k++) out6[k] = d.partial_h[k];
}
void launch_ke(DeviceState &d, const TypeTables &tt) {
  int nb = (d.n + BLOCK - 1) / BLOCK;
  settle_velocities(d);
  hipLaunchKernelGGL(k_ke, dim3(nb), dim3(BLOCK), 0, d.stream, d.n, d.pos, d.v[0], d.v[1], d.v[2], tt, d.partial);
}
static ForceArgs force_args(DeviceState &d, const double sl[4]) {
  ForceArgs A;
  A.n = d.n; A.npad = d.npad; A.nblocks = (d.n + BLOCK - 1) / BLOCK; A.bpa = d.bpa; A.nt = d.ntypes + 1;
  A.pos = d.pos; A.neigh = d.neigh; A.numneigh = d.numneigh; A.bpart = d.bpart; A.bshift = d.bshift; A.bond_minimg = d.bond_minimg; A.pairtab = d.pairtab;
  A.sl0 = sl[0]; A.sl1 = sl[1]; A.sl2 = sl[2]; A.sl3 = sl[3];
  A.uniform = d.pair_uniform; A.u_cutsq = d.pair_u[0]; A.u_lj1 = d.pair_u[1]; A.u_lj2 = d.pair_u[2];
  A.u_lj3 = d.pair_u[3]; A.u_lj4 = d.pair_u[4]; A.u_off = d.pair_u[5];
  A.has_sb = 0;     // some list entries carry a special level whose factor is not 1 (incl. lj weight 0 kept for its coul weight)
  for (int k = 1; k <= 3; k++) if (d.sflag[k] == 2) A.has_sb = 1;
  A.margin = d.cutneigh;
  static int lim = getenv("LAMMPS_LE_NN_LIMIT") ? atoi(getenv("LAMMPS_LE_NN_LIMIT")) : (1 << 30);
  A.nn_limit = lim;
  A.maxrow = d.maxneigh - 1;
  A.diag = 0;
  A.sendslot = nullptr; A.send_dn = A.send_up = nullptr;
  {
    // posf = (float)xhold: a coordinate is off by <= M * 2^-24, a squared displacement d^2 <= skin^2/4 .. by
    // <= 2 * sqrt(3) * |d| * e + 3 e^2; |d| <= ~skin near the threshold.  Band = four times that bound.
    double M = 0.0;
    for (int k = 0; k < 3; k++) M = std::max({M, fabs(d.box.lo[k]), fabs(d.box.hi[k])});
    const double e = M * 5.97e-8, dmax = 2.0 * d.cutneigh;
    A.holdf = (d.posf && !d.dd) ? d.posf : nullptr;
    A.hold_band = 4.0 * (2.0 * 1.7320508 * dmax * e + 3.0 * e * e);
  }
  A.bin = 0; A.ncx = d.ncell[0]; A.ncy = d.ncell[1]; A.ncz = d.ncell[2]; A.rtile = d.row_tile;
  A.cix = d.cellinv[0]; A.ciy = d.cellinv[1]; A.ciz = d.cellinv[2]; A.zlo_ext = d.zlo_ext;
  A.cell_of = d.cell_of; A.cell_count = d.cell_count; A.cell_rank = d.tag_tmp;
  return A;
}
// `parts`: 3 = pair + bond (the default), 1 = pair only, 2 = bond only, 0 = nothing (forces zeroed); run_style respa
void launch_force(DeviceState &d, const BondTable &bt, const double sl[4], bool eflag, bool has_pair, int parts, bool soft) {
  ForceArgs A = force_args(d, sl);
  int grid = xcd_grid(A.nblocks);
  if (!has_pair) parts &= 2;
  if (parts == 0) {
    for (int k = 0; k < 3; k++) HIP_CHECK(hipMemsetAsync(d.f[k], 0, (size_t)d.n * sizeof(double), d.stream));
    return;
  }
  if (parts == 1) A.diag = 1;      // pairs only (bonds only: straight from the bond-partner table)
  with_flags([&](auto E, auto P, auto NOBOND, auto SOFT) {
    if constexpr (force_variant_exists(E, P, NOBOND, SOFT)) {
      d.force_census[force_variant_key(E, P, NOBOND, SOFT)]++;
      hipLaunchKernelGGL((k_force<E, P, NOBOND, SOFT>), dim3(grid), dim3(BLOCK), 0, d.stream, A, bt, d.box, d.f[0], d.f[1], d.f[2], d.partial, d.flags);
    }
  }, eflag, (parts & 1) != 0, parts == 1, soft && (parts & 1) != 0);
}
// The launcher's table: the keys that exist, ascending, and k_step<key> of each at the same index - built at compile time from
// step_variant_exists, which is therefore the one statement of what is compiled.  step_kernel: the instantiation of a key by
// binary search, nullptr where there is none
struct StepKeys { int key[count_step_variants()]; };
constexpr StepKeys existing_step_keys() {
  StepKeys t{};
  for (int key = 0, n = 0; key < STEP_KEY_SPACE; key++) if (step_variant_exists(key)) t.key[n++] = key;
  return t;
}
constexpr StepKeys STEP_KEYS = existing_step_keys();
using StepKernel = decltype(&k_step<0>);
template <size_t... I>
static StepKernel step_kernel(int key, std::index_sequence<I...>) {
  static const StepKernel kernels[] = {k_step<STEP_KEYS.key[I]>...};
  const int *at = std::lower_bound(std::begin(STEP_KEYS.key), std::end(STEP_KEYS.key), key);
  return (at != std::end(STEP_KEYS.key) && *at == key) ? kernels[at - STEP_KEYS.key] : nullptr;
}
static StepKernel step_kernel(int key) { return step_kernel(key, std::make_index_sequence<count_step_variants()>{}); }
// Fills the kernel's argument record from the device state, the plan and the launch's arguments - the one place that does -
// and launches the instantiation the plan names.  ev_start / ev_stop (sampled launches only) take the kernel's own begin /
// end timestamps from its dispatch packet, the same clock rocprofv3 --kernel-trace reports
static void launch_step_kernel(DeviceState &d, const StepPlan &p, const ForceArgs &A, const StepArgs &a, hipEvent_t ev_start,
                               hipEvent_t ev_stop) {
  StepKernelArgs S = {};
  IndentTable itab{};
  S.tag = d.tag; S.draws = d.rng_out;
  // fixes on groups (GRP): the draws of a thermostat on a group go by the rank among its members
  S.ranks = p.member_ranks ? d.lgrank : d.crank;
  S.vx = d.v[0]; S.vy = d.v[1]; S.vz = d.v[2];
  S.dtv = a.dtv; S.triggersq = a.triggersq; S.check = p.check ? 1 : 0;
  S.flags = d.flags; S.phase = d.phase; S.which = p.which;
  S.nvebit = p.nvebit; S.lgbit = p.lgbit;
  S.vperm = d.perm; S.vxo = d.v_tmp[0]; S.vyo = d.v_tmp[1]; S.vzo = d.v_tmp[2];
  if (p.grp) {
    if (!d.gmask) throw LammpsError("internal: fused step on groups without group masks");
    S.gmask = d.gmask;
  }
  if (p.wall) {
    if (!d.walltab_dev) throw LammpsError("internal: fused wall step without the wall table");
    S.walls = d.walltab_dev;
  }
  // fix indent: a run with indenters takes the indent variants, and the launch carries the table of every one of them
  // (DeviceState::indent_count) - a launch without it would drop them silently
  if (p.fused && (p.indent != (d.indent_count > 0) || (p.indent && (!a.indents || a.indents->n != d.indent_count))))
    throw LammpsError("internal: fused step without the table of this run's indenters");
  if (p.indent) itab = *a.indents;
  if (p.ext) {
    if (!d.forceoptab_dev) throw LammpsError("internal: fused EXT step without the force-op table");
    if (d.forceop_grouped && !d.gmask) throw LammpsError("internal: fused EXT step on groups without group masks");
    S.ext = d.forceoptab_dev; S.img = d.img; S.ext_active = a.ext_active;
    if (d.forceop_grouped) S.gmask = d.gmask;
  }
  // a whole step of a run with an angle style (NEXT) evaluates the listed angles inside the kernel
  if (p.ang && p.next) {
    if (!d.eff_rec || !d.eff_n || !d.angtab_dev) throw LammpsError("internal: fused angle step without angle records");
    S.angle_rec = d.eff_rec; S.angle_n = d.eff_n; S.angles = d.angtab_dev;
  }
  if (p.ef) S.partial = d.partial;     // a thermo step: block totals of energies and virial
  const int grid = xcd_grid(A.nblocks);
  // velocities a rebuild left in the old order: this launch hands them over if it is the shape that can, else they are
  // permuted first.  (a launch that stores nothing - a list overflowed - is undone as a whole: undo_step_swap)
  const bool lazy_v = d.v_pending && takes_pending_v(p, d.dd != 0);
  if (!lazy_v) settle_velocities(d);
  const int key = step_plan_key(p, lazy_v);
  const StepKernel kernel = p.fused ? step_kernel(key) : nullptr;
  if (!kernel) throw LammpsError("internal: the step plan names a variant of the step kernel that does not exist");
  S.indents = itab;
  d.step_census[key]++;      // (host memory: the launch census, DeviceState::step_census)
  hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), p.lds_pad, d.stream, ev_start, ev_stop, 0, A, *a.bt, d.box, *a.tt, S,
                        d.f[0], d.f[1], d.f[2], d.pos_tmp, d.xhold);
  d.step_took_v = lazy_v;
  if (lazy_v) { for (int k = 0; k < 3; k++) std::swap(d.v[k], d.v_tmp[k]); d.v_pending = false; }
}
void launch_step(DeviceState &d, const StepPlan &p, const StepArgs &a) {
  ForceArgs A = force_args(d, a.special_lj);
  if (d.dd && p.next && d.sendslot) {
    A.sendslot = d.sendslot;
    if (d.fast_halo && d.direct_recv && p.which < 0) {
      // the neighbours' windows, in their sorted ghost order: what I send down arrives there "from above" and vice versa
      const int parity = (int)((d.halo_seq + 1u) & 1u);
      A.send_dn = d.peer_win[0] + (size_t)(parity * 2 + 1) * d.halo_cap;
      A.send_up = d.peer_win[1] + (size_t)(parity * 2 + 0) * d.halo_cap;
      d.packed_peer = parity + 1;
      d.packed_ahead = false;
    } else {
      A.send_dn = d.sendbuf; A.send_up = d.sendbuf + d.nsend[0];
      d.packed_ahead = true;
      d.packed_peer = 0;
    }
  }
  if (p.lpb == 4) { A.nblocks = (d.n + BLOCK / 4 - 1) / (BLOCK / 4); A.maxrow = (d.maxneigh - 4) / 4; }
  if (p.bin) {
    // the counts are zero unless an earlier launch binned and no rebuild consumed them (the scan zeroes what it reads)
    if (d.cell_count_dirty) HIP_CHECK(hipMemsetAsync(d.cell_count, 0, (size_t)(d.ncells + 1) * sizeof(int), d.stream));
    A.bin = 1;
  }
  note_step_binned(d, p.bin);
  // LAMMPS_LE_DIAG_STEP=bits: the same kernel is launched once more BEFORE the real launch with parts switched off
  // (1 bonds, 2 pair loop, 4 draws, 8 pair gathers replaced by coalesced loads, 128 nothing); it writes only the second position buffer, which the real launch
  // overwrites, so the run is physically unchanged and a kernel trace shows what each part costs
  if (p.diag_bits) {
    StepPlan q;
    q.fused = q.langevin = q.next = q.ident = q.pair = q.diag = true;
    q.check = p.check; q.which = p.which; q.lds_pad = p.lds_pad;
    ForceArgs R = A;
    R.diag = p.diag_bits | 64; R.bin = 0;
    launch_step_kernel(d, q, R, a, nullptr, nullptr);
  }
  launch_step_kernel(d, p, A, a, a.ev_start, a.ev_stop);
  if (p.next && a.swap_buffers) note_step_swapped(d);
}
// test hooks (not part of the reference surface, not declared in include/lammps_le.h): the plan for a request under the
// environment switches as they stand at this call.  Five exported names, one per layout the request and the answer have had;
// each reads the first `nreq` numbers of the request (the rest: none) and gets the first `nout` of the answer.
// req = langevin, next, ident, pair, angles, thermo, nvebit, lgbit, which, check, cells, [11] walls (StepRequest::walls),
// [12] pair_style soft, [13] fix spring/self | addforce | setforce, [14] indenters (StepRequest::indents)
// out = fused, langevin, next, ident, pair, lpb, diag, ahead, ang, ef, grp, bin, member_ranks, diag_bits, lds_pad, [15] whether
// the launcher's table holds the instantiation the plan names (its own look-up, nothing is launched), [16] StepPlan::wall,
// [17] the plan takes velocities a rebuild left pending, [18] StepPlan::soft, [19] StepPlan::ext, [20] the number of
// instantiations without the indent variants, [21] StepPlan::indent, [22] the number of instantiations
static void test_step_plan(int n_owned, int decomposed, const int *req, int nreq, int nout, int *out) {
  int q[15] = {};
  std::copy(req, req + nreq, q);
  StepRequest r;
  r.langevin = q[0]; r.next = q[1]; r.ident = q[2]; r.pair = q[3]; r.angles = q[4]; r.thermo = q[5];
  r.nvebit = q[6]; r.lgbit = q[7]; r.which = q[8]; r.check = q[9]; r.cells = q[10];
  r.walls = q[11]; r.soft = q[12] != 0; r.ext = q[13] != 0; r.indents = q[14];
  const StepPlan p = plan_step(n_owned, decomposed != 0, r, StepKnobs());
  const bool known = p.fused && step_kernel(step_plan_key(p, false));
  constexpr int variants = count_step_variants(SK_INDENT), all_variants = count_step_variants();   // (at compile time: the sweeps of the host tests call this a million times)
  const int v[23] = {p.fused, p.langevin, p.next, p.ident, p.pair, p.lpb, p.diag, p.ahead, p.ang, p.ef, p.grp, p.bin, p.member_ranks,
                     p.diag_bits, (int)p.lds_pad, known, p.wall, takes_pending_v(p, decomposed != 0), p.soft, p.ext, variants,
                     p.indent, all_variants};
  std::copy(v, v + nout, out);
}
extern "C" void lammps_le_test_step_plan(int n_owned, int decomposed, const int *req, int *out) { test_step_plan(n_owned, decomposed, req, 11, 16, out); }
extern "C" void lammps_le_test_step_plan_walls(int n_owned, int decomposed, const int *req, int *out) { test_step_plan(n_owned, decomposed, req, 12, 18, out); }
extern "C" void lammps_le_test_step_plan_soft(int n_owned, int decomposed, const int *req, int *out) { test_step_plan(n_owned, decomposed, req, 13, 19, out); }
extern "C" void lammps_le_test_step_plan_ext(int n_owned, int decomposed, const int *req, int *out) { test_step_plan(n_owned, decomposed, req, 14, 21, out); }
extern "C" void lammps_le_test_step_plan_indent(int n_owned, int decomposed, const int *req, int *out) { test_step_plan(n_owned, decomposed, req, 15, 23, out); }
// 1: the launcher's table holds this key (the look-up launch_step_kernel makes; launches nothing, needs no device)
extern "C" int lammps_le_test_step_dispatch(int key) { return step_kernel(key) != nullptr; }

// ------------------------------------------------------------------------------------------
// Angle forces (angle_style harmonic | cosine): AngleHarmonic::compute / AngleCosine::compute (src/MOLECULE/
// angle_harmonic.cpp:53-147, angle_cosine.cpp:49-121) as one thread per bead over the LISTED angles the bead is part of
// (k_angle_list above).  A bead evaluates every such angle and keeps
// only its own share - f1 as atom 1, -(f1 + f3) as the centre, f3 as atom 3 - so no atomics are needed and the order of
// a bead's sum is fixed; the two other atoms are found through map[] (tag -> index).  Energy and virial: a third of each
// per stored copy, which is Angle::ev_tally with newton_bond off (src/angle.cpp:164-250).  The two arms are taken by
// minimum image (they are a bond long; the reference uses the images closest to the listing atom at the last reneighbor).
// The angle list (NTopoAngleAll::build with newton_bond off, src/ntopo_angle_all.cpp:55-76): the copy atom i stores is
// listed iff i has the lowest local index of the three atoms, and a listed angle moves all three.  One thread per atom
// appends its listed copies to the three atoms' records; a second kernel sorts each atom's records (central atom, ends,
// type), so that what a bead sums, and in which order, depends on nothing but the topology.  An angle across a periodic
// face: seen from the listing atom i the atoms on the other side are ghost images (Domain::closest_image, index >= nlocal),
// which never block a listing and which the listing does not move (newton_bond off: forces go to owned atoms only,
// angle_harmonic.cpp:121-137) - so the copy on i is listed iff i has the lowest local index among the atoms on ITS side, and
// its record goes to those atoms only; the atoms on the other side are moved by the listings of their own copies.  With all
// copies in place that adds up to one evaluation per atom, with copies out of step it is what the reference computes
// (found by the mixed sweep, tests/test_gpu_fuzz2.py seeds 17, 74, 125).
// (type, a1, a2, a3) of the first ANGLE_PACK_COLS stored angles of every atom, column-major by tag (empty slots: type 0)
__global__ __launch_bounds__(BLOCK) void k_angle_pack(int T, int apa, int stride, const int *__restrict__ num_angle,
                                                      const int *__restrict__ angle_type, const int *__restrict__ a1,
                                                      const int *__restrict__ a2, const int *__restrict__ a3, int4 *__restrict__ pack) {
  const int i = blockIdx.x * BLOCK + threadIdx.x + 1;
  if (i > T) return;
  const int na = num_angle[i];
  for (int m = 0; m < ANGLE_PACK_COLS; m++) {
    const size_t c = (size_t)i * apa + m;
    pack[(size_t)m * stride + i] = m < na ? make_int4(angle_type[c], a1[c], a2[c], a3[c]) : make_int4(0, 0, 0, 0);
  }
}
__global__ __launch_bounds__(BLOCK) void k_angle_list(int T, int apa, int ecap, int npad, const int *__restrict__ crank,
                                                      const int *__restrict__ map, const float4 *__restrict__ pos, Box box, int n_owned,
                                                      const int *__restrict__ num_angle, const int *__restrict__ angle_type,
                                                      const int *__restrict__ a1, const int *__restrict__ a2,
                                                      const int *__restrict__ a3, int *__restrict__ eff_n,
                                                      int4 *__restrict__ eff_rec, int *__restrict__ flags,
                                                      const int4 *__restrict__ pack, int pack_stride) {
  const int i = blockIdx.x * BLOCK + threadIdx.x + 1;
  if (i > T) return;
  const int na = num_angle[i];
  const int li = crank ? crank[i] : i;
  for (int m = 0; m < na; m++) {
    const size_t c = (size_t)i * apa + m;
    // (the first columns come from the packed records - coalesced 16-byte loads -, the tables of stride apa only beyond them)
    int4 src;
    if (m < ANGLE_PACK_COLS) src = pack[(size_t)m * pack_stride + i];
    else src = make_int4(angle_type[c], a1[c], a2[c], a3[c]);
    const int t[3] = {src.y, src.z, src.w};
    if (n_owned < 0) {
      // one GPU: two of an angle's three stored copies are not listed (the listing atom must have the lowest local index among
      // the atoms on its side), and which ones is known from the ranks alone unless an atom with a lower rank sits across a
      // periodic face - so only those atoms are looked up before the copy is dropped (the kernel is bound by its gathers)
      int rk[3];
      bool lower = false;
      for (int q = 0; q < 3; q++) { rk[q] = crank ? crank[t[q]] : t[q]; lower = lower || li > rk[q]; }
      const int pi = map[i];
      if (pi < 0) { flags[FLAG_ERROR] = ERR_BOND_MISSING; continue; }
      const float4 ri = pos[pi];
      int p[3] = {-1, -1, -1};
      bool ghost[3] = {false, false, false}, known[3] = {false, false, false}, listed = true;
      auto look = [&](int q) {
        p[q] = (t[q] == i) ? pi : map[t[q]];
        known[q] = true;
        if (p[q] < 0) return false;
        const float4 rq = pos[p[q]];
        ghost[q] = fabs((double)ri.x - (double)rq.x) > box.half[0] || fabs((double)ri.y - (double)rq.y) > box.half[1] ||
                   fabs((double)ri.z - (double)rq.z) > box.half[2];
        return true;
      };
      bool missing = false;
      if (lower)
        for (int q = 0; q < 3 && listed; q++)
          if (li > rk[q]) { if (!look(q)) { missing = true; break; } listed = ghost[q]; }
      if (missing) { flags[FLAG_ERROR] = ERR_BOND_MISSING; continue; }
      if (!listed) continue;
      for (int q = 0; q < 3; q++) if (!known[q] && !look(q)) missing = true;
      if (missing) { flags[FLAG_ERROR] = ERR_BOND_MISSING; continue; }
      const int4 rec = make_int4(src.x, p[0], p[1], p[2]);
      for (int q = 0; q < 3; q++) {
        if (ghost[q]) continue;
        const int slot = atomicAdd(&eff_n[p[q]], 1);
        if (slot >= ecap) { flags[FLAG_ERROR] = ERR_ANGLES; continue; }
        eff_rec[(size_t)slot * npad + p[q]] = rec;
      }
      continue;
    }
    // records hold PHYSICAL indices (this list lives until the next reneighbor, like the indices) and sit column-major by
    // the bead's own index: the force kernel reads them coalesced and gathers positions without a tag -> index lookup
    const int p[3] = {map[t[0]], map[t[1]], map[t[2]]};
    const int pi = map[i];
    // decomposed runs (n_owned >= 0; the angle tables are replicated): only angles that move a bead this rank OWNS matter here;
    // all three atoms of such an angle must be present (owned or ghost: the ghost shell of a run with angles holds every bead
    // within the ghost cutoff of a face, k_dd_borders)
    if (n_owned >= 0 && !((p[0] >= 0 && p[0] < n_owned) || (p[1] >= 0 && p[1] < n_owned) || (p[2] >= 0 && p[2] < n_owned))) continue;
    if (p[0] < 0 || p[1] < 0 || p[2] < 0 || pi < 0) { flags[FLAG_ERROR] = ERR_BOND_MISSING; continue; }
    // (the float copy of the build-time positions decides "more than half a box away": an angle's arms are a few sigma long)
    const float4 ri = pos[pi];
    bool listed = true, ghost[3];
    for (int q = 0; q < 3; q++) {
      const float4 rq = pos[p[q]];
      ghost[q] = fabs((double)ri.x - (double)rq.x) > box.half[0] || fabs((double)ri.y - (double)rq.y) > box.half[1] ||
                 fabs((double)ri.z - (double)rq.z) > box.half[2];
      listed = listed && (ghost[q] || li <= (crank ? crank[t[q]] : t[q]));
    }
    if (!listed) continue;
    const int4 rec = make_int4(src.x, p[0], p[1], p[2]);
    for (int q = 0; q < 3; q++) {
      if (ghost[q] || (n_owned >= 0 && p[q] >= n_owned)) continue;
      const int slot = atomicAdd(&eff_n[p[q]], 1);
      if (slot >= ecap) { flags[FLAG_ERROR] = ERR_ANGLES; continue; }
      eff_rec[(size_t)slot * npad + p[q]] = rec;
    }
  }
}
__global__ __launch_bounds__(BLOCK) void k_angle_sort(int n, int ecap, int npad, int *__restrict__ eff_n, int4 *__restrict__ eff_rec) {
  const int p = blockIdx.x * BLOCK + threadIdx.x;
  if (p >= n) return;
  const int cnt = min(eff_n[p], ecap);
  eff_n[p] = cnt;
  if (cnt < 2) return;
  auto less = [](const int4 &x, const int4 &y) {       // (type, i1, i2, i3) = (x, y, z, w): centre, ends, type
    const int xl = min(x.y, x.w), xh = max(x.y, x.w), yl = min(y.y, y.w), yh = max(y.y, y.w);
    if (x.z != y.z) return x.z < y.z;
    if (xl != yl) return xl < yl;
    if (xh != yh) return xh < yh;
    return x.x < y.x;
  };
  for (int a = 1; a < cnt; a++) {
    const int4 key = eff_rec[(size_t)a * npad + p];
    int b = a - 1;
    while (b >= 0) {
      const int4 cur = eff_rec[(size_t)b * npad + p];
      if (!less(key, cur)) break;
      eff_rec[(size_t)(b + 1) * npad + p] = cur;
      b--;
    }
    eff_rec[(size_t)(b + 1) * npad + p] = key;
  }
}
void launch_angle_list(DeviceState &d) {
  if (d.apa <= 0) return;
  const int T = d.maxtag, nb = std::max(1, (T + BLOCK - 1) / BLOCK);
  HIP_CHECK(hipMemsetAsync(d.eff_n, 0, (size_t)d.npad * sizeof(int), d.stream));
  const int pack_stride = T + 2;
  if (d.angle_pack_dirty) {       // (the angle tables change at an LE firing with `atype` / angle breaking, not at a rebuild)
    hipLaunchKernelGGL(k_angle_pack, dim3(nb), dim3(BLOCK), 0, d.stream, T, d.apa, pack_stride, d.num_angle, d.angle_type, d.angle_a1,
                       d.angle_a2, d.angle_a3, (int4 *)d.angle_pack);
    d.angle_pack_dirty = false;
  }
  hipLaunchKernelGGL(k_angle_list, dim3(nb), dim3(BLOCK), 0, d.stream, T, d.apa, d.ecap, d.npad, d.ident_order ? (const int *)nullptr : d.crank,
                     d.map, d.posf, d.box, d.dd ? d.n : -1, d.num_angle, d.angle_type, d.angle_a1, d.angle_a2, d.angle_a3, d.eff_n, d.eff_rec, d.flags,
                     (const int4 *)d.angle_pack, pack_stride);
  hipLaunchKernelGGL(k_angle_sort, dim3(std::max(1, (d.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, d.stream, d.n, d.ecap, d.npad, d.eff_n,
                     d.eff_rec);
}

template <bool EFLAG, bool OVERWRITE = false>
__global__ __launch_bounds__(BLOCK) void k_angle(int n, int ecap, Box box, AngleTable at, const double4 *__restrict__ pos,
                                                 int npad, const int *__restrict__ num_angle, const int4 *__restrict__ rec,
                                                 double *__restrict__ fx,
                                                 double *__restrict__ fy, double *__restrict__ fz,
                                                 double *__restrict__ partial_a, int *__restrict__ flags) {
  const int p = blockIdx.x * BLOCK + threadIdx.x;
  double acc[8];
#pragma unroll
  for (int k = 0; k < 8; k++) acc[k] = 0.0;
  if (p < n) {
    const int na = num_angle[p];
    const double4 rp = pos[p];
    double f0 = 0.0, f1v = 0.0, f2 = 0.0;
    bead_angles<EFLAG>(p, rp, na, rec, npad, pos, box, at, f0, f1v, f2, acc);
    if (OVERWRITE) { fx[p] = f0; fy[p] = f1v; fz[p] = f2; }      // the fused step kernel adds them to its own sums
    else { fx[p] += f0; fy[p] += f1v; fz[p] += f2; }
  }
  if (EFLAG) {
    __shared__ double red[BLOCK / 64][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      double v = acc[k];
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < 8) {
      double v = 0.0;
      for (int w = 0; w < BLOCK / 64; w++) v += red[w][threadIdx.x];
      partial_a[(size_t)blockIdx.x * 8 + threadIdx.x] = v;
    }
  }
}
// the coefficient table in device memory, for the fused step (kernel arguments of k_step are not to be touched)
void upload_angle_table(DeviceState &d, const AngleTable &at) {
  DEV_RESERVE(d.mem, d.angtab_dev, 1);
  HIP_CHECK(hipMemcpyAsync(d.angtab_dev, &at, sizeof(AngleTable), hipMemcpyHostToDevice, d.stream));
  HIP_CHECK(hipStreamSynchronize(d.stream));      // (`at` is the caller's object)
}
void launch_angle(DeviceState &d, const AngleTable &at, bool eflag, bool overwrite) {
  if (d.apa <= 0) return;
  const int nb = std::max(1, (d.n + BLOCK - 1) / BLOCK);
  with_flags([&](auto E, auto O) {      // (the fused step kernel adds the forces of an `overwrite` launch to its own sums; no energies then)
    if constexpr (!(E && O))
      hipLaunchKernelGGL((k_angle<E, O>), dim3(nb), dim3(BLOCK), 0, d.stream, d.n, d.ecap, d.box, at, d.pos, d.npad, d.eff_n,
                         d.eff_rec, d.f[0], d.f[1], d.f[2], d.partial_a, d.flags);
  }, eflag && !overwrite, overwrite);
}
void reduce_angle_partials(DeviceState &d, double *out8) {
  const int nb = std::max(1, (d.n + BLOCK - 1) / BLOCK);
  hipLaunchKernelGGL((k_colsum<8>), dim3(1), dim3(BLOCK), 0, d.stream, nb, d.partial_a, d.partial_a + (size_t)nb * 8);
  HIP_CHECK(hipMemcpyAsync(d.partial_h, d.partial_a + (size_t)nb * 8, 8 * sizeof(double), hipMemcpyDeviceToHost, d.stream));
  stream_sync(d);
  for (int k = 0; k < 8; k++) out8[k] = d.partial_h[k];
}

void upload_wall_table(DeviceState &d, const WallTable &wt) {
  DEV_RESERVE(d.mem, d.walltab_dev, 1);
  DEV_RESERVE(d.mem, d.wall_partial, (size_t)WALL_MAX * (d.nred_blocks + 1) * 16);
  HIP_CHECK(hipMemsetAsync(d.wall_partial, 0, (size_t)WALL_MAX * (d.nred_blocks + 1) * 16 * sizeof(double), d.stream));
  HIP_CHECK(hipMemcpyAsync(d.walltab_dev, &wt, sizeof(WallTable), hipMemcpyHostToDevice, d.stream));
  HIP_CHECK(hipStreamSynchronize(d.stream));      // (`wt` is the caller's object)
}
void launch_wall(DeviceState &d, const WallTable &wt, int phase, bool eflag) {
  bool any = false, grouped = false;
  for (int k = 0; k < wt.n; k++) if (wt.w[k].after_langevin == phase) { any = true; grouped = grouped || wt.w[k].groupbit != 1; }
  if (!any) return;
  if (!d.walltab_dev || !d.wall_partial) throw LammpsError("internal: fix wall/region without its table on the device");
  if (grouped && !d.gmask) throw LammpsError("internal: fix wall/region on a group without group masks");
  const int nb = std::max(1, (d.n + BLOCK - 1) / BLOCK);
  if (nb > d.nred_blocks) throw LammpsError("internal: more blocks than rows of block sums");
  with_flags([&](auto E) {
    hipLaunchKernelGGL((k_wall<E>), dim3(nb), dim3(BLOCK), 0, d.stream, d.n, d.pos, d.tag, grouped ? d.gmask : (const int *)nullptr,
                       d.walltab_dev, phase, d.f[0], d.f[1], d.f[2], d.wall_partial, d.nred_blocks + 1, d.flags);
  }, eflag);
}
// the totals of n rows of block sums of one family (wall_partial | forceop_partial | indent_partial): rows of 16 into out
void reduce_rows(DeviceState &d, double *partial, int n, double *out) {
  const int nb = std::max(1, (d.n + BLOCK - 1) / BLOCK);
  const size_t rows = (size_t)d.nred_blocks + 1;
  for (int k = 0; k < n; k++) {
    double *tab = partial + (size_t)k * rows * 16;
    hipLaunchKernelGGL((k_colsum<16>), dim3(1), dim3(BLOCK), 0, d.stream, nb, tab, tab + (size_t)nb * 16);
    HIP_CHECK(hipMemcpyAsync(d.partial_h + 16 * (size_t)k, tab + (size_t)nb * 16, 16 * sizeof(double), hipMemcpyDeviceToHost, d.stream));
  }
  stream_sync(d);
  for (int k = 0; k < 16 * n; k++) out[k] = d.partial_h[k];
}

// fix indent: the rows of block sums (the table itself travels with every launch)
void reserve_indent_partials(DeviceState &d) {
  const size_t np = (size_t)INDENT_MAX * (d.nred_blocks + 1) * 16;
  DEV_RESERVE(d.mem, d.indent_partial, np);
  HIP_CHECK(hipMemsetAsync(d.indent_partial, 0, np * sizeof(double), d.stream));
}
void launch_indent(DeviceState &d, const IndentTable &it, int phase, bool eflag) {
  bool any = false, grouped = false;
  if (it.n < 0 || it.n > INDENT_MAX) throw LammpsError("internal: fix indent table with a bad count");
  for (int k = 0; k < it.n; k++) if (it.e[k].phase == phase) { any = true; grouped = grouped || it.e[k].groupbit != 1; }
  if (!any) return;
  if (!d.indent_partial) throw LammpsError("internal: fix indent without its rows of block sums");
  if (grouped && !d.gmask) throw LammpsError("internal: fix indent on a group without group masks");
  const int nb = std::max(1, (d.n + BLOCK - 1) / BLOCK);
  if (nb > d.nred_blocks) throw LammpsError("internal: more blocks than rows of block sums");
  with_flags([&](auto E) {
    hipLaunchKernelGGL((k_indent<E>), dim3(nb), dim3(BLOCK), 0, d.stream, d.n, d.pos, d.tag, grouped ? d.gmask : (const int *)nullptr,
                       it, d.box, phase, d.f[0], d.f[1], d.f[2], d.indent_partial, d.nred_blocks + 1);
  }, eflag);
}
void upload_forceop_table(DeviceState &d, ForceOpTable &ft, const double *const *origins, int natoms) {
  const size_t stride = (size_t)natoms + 1;
  ft.stride = (int)stride;
  d.forceop_grouped = false;
  std::vector<double> block(3 * stride);
  for (int k = 0; k < ft.n; k++) {
    if (ft.e[k].groupbit != 1) d.forceop_grouped = true;
    ft.e[k].origin = nullptr;
    if (!origins[k]) continue;
    // [natoms][3] by tag - 1 on the host -> [3][natoms + 1] by tag here
    for (int c = 0; c < 3; c++) {
      block[c * stride] = 0.0;
      for (int i = 0; i < natoms; i++) block[c * stride + i + 1] = origins[k][3 * (size_t)i + c];
    }
    DEV_RESERVE(d.mem, d.forceop_origin[k], 3 * stride);
    HIP_CHECK(hipMemcpyAsync(d.forceop_origin[k], block.data(), 3 * stride * sizeof(double), hipMemcpyHostToDevice, d.stream));
    HIP_CHECK(hipStreamSynchronize(d.stream));      // (`block` is filled again for the next entry)
    ft.e[k].origin = d.forceop_origin[k];
  }
  DEV_RESERVE(d.mem, d.forceoptab_dev, 1);
  const size_t np = (size_t)FORCEOP_MAX * (d.nred_blocks + 1) * 16;
  // the rows of block sums outlive a `run` while they still mean the same: an addforce with `every N` that skips the setup step
  // of the next run reports the sums of the last step on which it acted, as the reference keeps foriginal.  Another table (the
  // origin addresses aside), another bead count or a new buffer starts from zero
  ForceOpTable same = ft;
  for (int k = 0; k < FORCEOP_MAX; k++) same.e[k].origin = nullptr;
  const bool fresh = DEV_RESERVE(d.mem, d.forceop_partial, np);
  if (fresh || d.forceop_rows_n != d.n || memcmp(&same, &d.forceoptab_last, sizeof(ForceOpTable)) != 0)
    HIP_CHECK(hipMemsetAsync(d.forceop_partial, 0, np * sizeof(double), d.stream));
  d.forceoptab_last = same;
  d.forceop_rows_n = d.n;
  HIP_CHECK(hipMemcpyAsync(d.forceoptab_dev, &ft, sizeof(ForceOpTable), hipMemcpyHostToDevice, d.stream));
  HIP_CHECK(hipStreamSynchronize(d.stream));      // (`ft` is the caller's object)
}
void launch_fixforce(DeviceState &d, const ForceOpTable &ft, int phase, unsigned active, bool eflag) {
  bool any = false;
  for (int k = 0; k < ft.n; k++) if (ft.e[k].phase == phase && ((active >> k) & 1u)) any = true;
  if (!any) return;
  if (!d.forceoptab_dev || !d.forceop_partial) throw LammpsError("internal: fix spring/self | addforce | setforce without the table on the device");
  if (d.forceop_grouped && !d.gmask) throw LammpsError("internal: fix spring/self | addforce | setforce on a group without group masks");
  if (ft.stride != d.maxtag + 1) throw LammpsError("internal: the origin blocks do not match the atom count");
  const int nb = std::max(1, (d.n + BLOCK - 1) / BLOCK);
  if (nb > d.nred_blocks) throw LammpsError("internal: more blocks than rows of block sums");
  with_flags([&](auto E) {
    hipLaunchKernelGGL((k_fixforce<E>), dim3(nb), dim3(BLOCK), 0, d.stream, d.n, d.npad, d.pos, d.tag,
                       d.forceop_grouped ? d.gmask : (const int *)nullptr, d.img, d.box, d.forceoptab_dev, phase, active,
                       d.f[0], d.f[1], d.f[2], d.forceop_partial, d.nred_blocks + 1);
  }, eflag);
}
// every sum of a thermo evaluation added up where it lies: the same k_colsum launches as the reduce_* functions above, no copy
void enqueue_thermo_sums(DeviceState &d, const PostForce &pf, bool angles, MinSources &src) {
  const int nb = std::max(1, (d.n + BLOCK - 1) / BLOCK);
  const size_t rows = (size_t)d.nred_blocks + 1;
  hipLaunchKernelGGL((k_colsum<16>), dim3(1), dim3(BLOCK), 0, d.stream, (d.n + BLOCK - 1) / BLOCK, d.partial, d.partial + (size_t)((d.n + BLOCK - 1) / BLOCK) * 16);
  src.add(d.partial + (size_t)((d.n + BLOCK - 1) / BLOCK) * 16, 16);
  if (angles) {
    hipLaunchKernelGGL((k_colsum<8>), dim3(1), dim3(BLOCK), 0, d.stream, nb, d.partial_a, d.partial_a + (size_t)nb * 8);
    src.add(d.partial_a + (size_t)nb * 8, 8);
  }
  auto family = [&](double *partial, int n, int cols) {
    for (int k = 0; k < n; k++) {
      double *tab = partial + (size_t)k * rows * 16;
      hipLaunchKernelGGL((k_colsum<16>), dim3(1), dim3(BLOCK), 0, d.stream, nb, tab, tab + (size_t)nb * 16);
      src.add(tab + (size_t)nb * 16, cols);
    }
  };
  family(d.wall_partial, pf.walltab.n, 16);
  family(d.forceop_partial, pf.forceoptab.n, 16);
  family(d.indent_partial, (int)pf.indent_fixes.size(), INDENT_COLS);      // (the four columns of an indenter)
}

// sum the per-block partials in a fixed order (deterministic); the totals land in the table's spare row nb
void reduce_partials(DeviceState &d, double *out16) {
  int nb = (d.n + BLOCK - 1) / BLOCK;
  hipLaunchKernelGGL((k_colsum<16>), dim3(1), dim3(BLOCK), 0, d.stream, nb, d.partial, d.partial + (size_t)nb * 16);
  HIP_CHECK(hipMemcpyAsync(d.partial_h, d.partial + (size_t)nb * 16, 16 * sizeof(double), hipMemcpyDeviceToHost, d.stream));
  stream_sync(d);
  for (int k = 0; k < 16; k++) out16[k] = d.partial_h[k];
}

}  // namespace lmp_le
