// kernels_local.hip — pair rows of the local computes: compute property/local (natom* / ntype*, patom* / ptype*) and
// compute pair/local (dist eng force fx fy fz), from the neighbor list the device already holds.
//
// Reference semantics restated here (one rank):
//   ComputePropertyLocal::count_pairs    src/compute_property_local.cpp:395-461   (NEIGH: every listed pair of the group;
//                                                                                  PAIR: rsq < cutsq[itype][jtype] as well)
//   ComputePairLocal::compute_pairs      src/compute_pair_local.cpp:160-290       (rows of the PAIR kind with values)
//   PairLJCut::single                    src/pair_lj_cut.cpp:657-673              (1.0 / rsq, factor_lj, the shift offset)
// The reference walks an occasional HALF list that is a copy of the pair style's list; the engine's list is FULL, so a pair
// is emitted from the end with the LOWER ID only (on the rank that owns that end; the partner may be a ghost).  Rows are
// ordered by (atom1, atom2): the count of every bead is stored by TAG, the exclusive scan of the counts over the tags is the
// row offset of every bead, and each bead orders its own short segment by the partner's ID.  The row count is exact: no
// atomics, no overflow path.
//
// Two launches around one scan:
//   k_local_count   one lane per owned bead in physical order; walks the bead's list column behind its bond entries (the list
//                   is column-major ELL: lanes of a wavefront read consecutive words, as in k_force) and counts the kept entries
//   k_local_fill    the same walk; writes (partner ID, list entry) of every kept entry at the bead's offset, orders the segment
//                   by partner ID (insertion sort on those two words), then completes each row: IDs, types and - PAIR kind -
//                   dist eng force fx fy fz in plain IEEE FP64 in the reference's operation order (compiled -ffp-contract=off)
// Algorithmic bytes per invocation at N beads with F list entries per bead and R rows, both passes together: 2 x 4 F N list
// words, a 4-byte tag gather per entry (2 x 4 F N), a 32-byte position gather per entry whose partner has the higher ID and is
// a member (PAIR kind: 2 x 16 F N, half the entries), 12 N for the counts and offsets by tag, and 16 R (IDs and types) + 48 R
// (values) for the rows, which then travel to the host once.
#include <algorithm>
#include <chrono>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "device.h"

namespace lmp_le {

constexpr int LOCAL_BLOCK = 256;

struct LocalArgs {
  int n, nall, npad, maxneigh, maxtag;   // owned beads, owned + ghosts, ELL stride, rows of the list table, highest ID
  int nt;                                // ntypes + 1: stride of the coefficient tables
  const double4 *pos;
  const int *tag, *neigh, *numneigh;
  const int *gmask;                      // group bits by tag (nullptr: group all)
  int bit;
  const double *pairtab;                 // cutsq lj1 lj2 lj3 lj4 offset, nt * nt each
  int zero;                              // pair_style zero: rows by zero_cutsq, eng and force 0
  double zero_cutsq;
  double sl0, sl1, sl2, sl3;             // special_lj by the special bits of an entry
  Box box;
};

__device__ __forceinline__ double local_rsq(const Box &box, const double4 &ri, const double4 &rj, double &dx, double &dy,
                                            double &dz) {
  dx = ri.x - rj.x; dy = ri.y - rj.y; dz = ri.z - rj.z;
  dx -= box.prd[0] * __builtin_rint(dx * box.iprd[0]);      // minimum image = the listed image (box >= 3 neighbor cutoffs)
  dy -= box.prd[1] * __builtin_rint(dy * box.iprd[1]);
  dz -= box.prd[2] * __builtin_rint(dz * box.iprd[2]);
  return dx * dx + dy * dy + dz * dz;
}
__device__ __forceinline__ double local_cutsq(const LocalArgs &A, int itype, int jtype) {
  return A.zero ? A.zero_cutsq : A.pairtab[itype * A.nt + jtype];
}

// is the list entry `jraw` of bead (tag t, position ri) a row?  tj := the partner's ID
template <bool PAIR>
__device__ __forceinline__ bool local_kept(const LocalArgs &A, int t, const double4 &ri, int jraw, int &tj) {
  const int j = jraw & NEIGH_MASK;
  if (j >= A.nall) return false;                            // (never, for a list that fits its table)
  tj = A.tag[j];
  if (tj <= t || tj > A.maxtag) return false;               // emitted from the lower ID
  if (A.gmask && !(A.gmask[tj] & A.bit)) return false;
  if (!PAIR) return true;
  double dx, dy, dz;
  const double4 rj = A.pos[j];
  return local_rsq(A.box, ri, rj, dx, dy, dz) < local_cutsq(A, (int)ri.w, (int)rj.w);
}

// the pair entries of bead p: rows [first, last) of its list column
__device__ __forceinline__ void local_span(const LocalArgs &A, int p, int &first, int &last) {
  const int word = A.numneigh[p];
  last = min(word & NN_COUNT_MASK, A.maxneigh);
  first = min((word >> NN_BOND_SHIFT) & NN_NBOND_MASK, last);
}

template <bool PAIR>
__global__ __launch_bounds__(LOCAL_BLOCK) void k_local_count(LocalArgs A, int *__restrict__ count) {
  const int p = blockIdx.x * LOCAL_BLOCK + threadIdx.x;
  if (p >= A.n) return;
  const int t = A.tag[p];
  if (t < 1 || t > A.maxtag) return;
  int c = 0;
  if (!A.gmask || (A.gmask[t] & A.bit)) {
    int first, last;
    local_span(A, p, first, last);
    const double4 ri = A.pos[p];
    const int *col = A.neigh + p;
    for (int k = first; k < last; k++) {
      int tj;
      if (local_kept<PAIR>(A, t, ri, col[(size_t)k * A.npad], tj)) c++;
    }
  }
  count[t] = c;
}

// ids: [R][4] = atom1 atom2 type1 type2; vals: [R][6] = dist eng force fx fy fz (PAIR kind)
template <bool PAIR>
__global__ __launch_bounds__(LOCAL_BLOCK) void k_local_fill(LocalArgs A, const int *__restrict__ offset, long nrows,
                                                            int *__restrict__ ids, double *__restrict__ vals) {
  const int p = blockIdx.x * LOCAL_BLOCK + threadIdx.x;
  if (p >= A.n) return;
  const int t = A.tag[p];
  if (t < 1 || t > A.maxtag) return;
  if (A.gmask && !(A.gmask[t] & A.bit)) return;
  const long base = offset[t];
  const int room = (int)(min((long)offset[t + 1], nrows) - base);     // = the count pass' answer for this bead
  if (room <= 0) return;
  int first, last;
  local_span(A, p, first, last);
  const double4 ri = A.pos[p];
  const int *col = A.neigh + p;
  int *seg = ids + 4 * base;
  int m = 0;
  for (int k = first; k < last && m < room; k++) {
    int tj;
    const int jraw = col[(size_t)k * A.npad];
    if (!local_kept<PAIR>(A, t, ri, jraw, tj)) continue;
    // insertion into the segment ordered by partner ID: words 1 and 2 of a row hold (partner ID, list entry) for now
    int b = m - 1;
    while (b >= 0 && seg[4 * b + 1] > tj) { seg[4 * (b + 1) + 1] = seg[4 * b + 1]; seg[4 * (b + 1) + 2] = seg[4 * b + 2]; b--; }
    seg[4 * (b + 1) + 1] = tj; seg[4 * (b + 1) + 2] = jraw;
    m++;
  }
  for (int r = 0; r < m; r++) {
    const int jraw = seg[4 * r + 2];
    const double4 rj = A.pos[jraw & NEIGH_MASK];
    seg[4 * r] = t; seg[4 * r + 2] = (int)ri.w; seg[4 * r + 3] = (int)rj.w;
    if (PAIR) {
      double dx, dy, dz;
      const double rsq = local_rsq(A.box, ri, rj, dx, dy, dz);
      double eng = 0.0, fpair = 0.0;
      if (!A.zero) {      // PairLJCut::single
        const int nt2 = A.nt * A.nt, ij = (int)ri.w * A.nt + (int)rj.w;
        const int sb = (jraw >> NEIGH_SB_SHIFT) & 3;
        const double factor_lj = (sb == 0) ? A.sl0 : (sb == 1) ? A.sl1 : (sb == 2) ? A.sl2 : A.sl3;
        const double r2inv = 1.0 / rsq;
        const double r6inv = r2inv * r2inv * r2inv;
        const double forcelj = r6inv * (A.pairtab[nt2 + ij] * r6inv - A.pairtab[2 * nt2 + ij]);
        fpair = factor_lj * forcelj * r2inv;
        const double philj = r6inv * (A.pairtab[3 * nt2 + ij] * r6inv - A.pairtab[4 * nt2 + ij]) - A.pairtab[5 * nt2 + ij];
        eng = factor_lj * philj;
      }
      double *v = vals + 6 * (base + r);
      const double dist = sqrt(rsq);
      v[0] = dist; v[1] = eng; v[2] = dist * fpair; v[3] = dx * fpair; v[4] = dy * fpair; v[5] = dz * fpair;
    }
  }
}

static double local_now_ms() {
  return 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The rows of one (kind, group) on this rank, at the CURRENT positions, from the list of the last rebuild.  Returns the row
// count; ids / vals point into a pinned host block that the next call overwrites (vals: PAIR kind only).  ms[0]: count pass +
// scan + the read of the total; ms[1]: fill pass + the copy to the host (host wall clock around the two waits).
long local_pair_rows(DeviceState &d, const LocalRowsRequest &rq, const int *&ids, const double *&vals, double ms[2]) {
  if (!d.neigh || !d.numneigh || !d.pos || d.maxneigh <= 0) throw LammpsError("internal: pair rows without a neighbor list");
  if (rq.bit != 1 && !d.gmask) throw LammpsError("internal: pair rows of a group without group masks");
  if (d.dd) dd_halo_wait(d);     // ghost slots a halo on the second stream may still be filling
  const double t0 = local_now_ms();
  LocalArgs A;
  A.n = d.n; A.nall = d.n + (d.dd ? d.nghost : 0); A.npad = d.npad; A.maxneigh = d.maxneigh; A.maxtag = d.maxtag;
  A.nt = d.ntypes + 1;
  A.pos = d.pos; A.tag = d.tag; A.neigh = d.neigh; A.numneigh = d.numneigh;
  A.gmask = rq.bit != 1 ? d.gmask : nullptr; A.bit = rq.bit;
  A.pairtab = d.pairtab; A.zero = rq.zero ? 1 : 0; A.zero_cutsq = rq.zero_cutsq;
  A.sl0 = rq.special_lj[0]; A.sl1 = rq.special_lj[1]; A.sl2 = rq.special_lj[2]; A.sl3 = rq.special_lj[3];
  A.box = d.box;
  const size_t nt = (size_t)d.maxtag + 2;
  DEV_RESERVE(d.mem, d.local_count, nt);
  DEV_RESERVE(d.mem, d.local_offset, nt);
  HIP_CHECK(hipMemsetAsync(d.local_count, 0, nt * sizeof(int), d.stream));      // (tags this rank does not own: no rows)
  const int grid = std::max(1, (d.n + LOCAL_BLOCK - 1) / LOCAL_BLOCK);
  if (rq.pair) hipLaunchKernelGGL(k_local_count<true>, dim3(grid), dim3(LOCAL_BLOCK), 0, d.stream, A, d.local_count);
  else hipLaunchKernelGGL(k_local_count<false>, dim3(grid), dim3(LOCAL_BLOCK), 0, d.stream, A, d.local_count);
  HIP_CHECK(hipGetLastError());
  size_t need = 0;
  HIP_CHECK(rocprim::exclusive_scan(nullptr, need, d.local_count, d.local_offset, 0, nt, rocprim::plus<int>(), d.stream));
  DEV_RESERVE(d.mem, d.local_scan_tmp, std::max(need, (size_t)256));
  HIP_CHECK(rocprim::exclusive_scan(d.local_scan_tmp, need, d.local_count, d.local_offset, 0, nt, rocprim::plus<int>(), d.stream));
  // the host reads the total once (count[maxtag + 1] is 0: the last offset is the sum); the pinned block holds at least a row
  if (d.mem.capacity(d.local_rows_h) < 64) d.mem.alloc_host(d.local_rows_h, (size_t)1 << 16, "d.local_rows_h");
  HIP_CHECK(hipMemcpyAsync(d.local_rows_h, d.local_offset + (nt - 1), sizeof(int), hipMemcpyDeviceToHost, d.stream));
  stream_sync(d);
  int total = 0;
  memcpy(&total, d.local_rows_h, sizeof(int));
  if (total < 0) throw LammpsError("compute property/local: more than 2^31 pair rows on one rank");
  const double t1 = local_now_ms();
  const long R = total;
  // one block: [R][6] values (PAIR kind), then [R][4] IDs and types
  const size_t vbytes = rq.pair ? (size_t)R * 6 * sizeof(double) : 0, bytes = vbytes + (size_t)R * 4 * sizeof(int);
  ids = nullptr; vals = nullptr;
  if (R > 0) {
    if (bytes > d.mem.capacity(d.local_rows)) DEV_RESERVE(d.mem, d.local_rows, bytes + bytes / 4);
    if (bytes > d.mem.capacity(d.local_rows_h)) d.mem.alloc_host(d.local_rows_h, bytes + bytes / 4, "d.local_rows_h");
    double *dv = reinterpret_cast<double *>(d.local_rows);
    int *di = reinterpret_cast<int *>(d.local_rows + vbytes);
    if (rq.pair) hipLaunchKernelGGL(k_local_fill<true>, dim3(grid), dim3(LOCAL_BLOCK), 0, d.stream, A, d.local_offset, R, di, dv);
    else hipLaunchKernelGGL(k_local_fill<false>, dim3(grid), dim3(LOCAL_BLOCK), 0, d.stream, A, d.local_offset, R, di, dv);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(d.local_rows_h, d.local_rows, bytes, hipMemcpyDeviceToHost, d.stream));
    stream_sync(d);
    vals = rq.pair ? reinterpret_cast<const double *>(d.local_rows_h) : nullptr;
    ids = reinterpret_cast<const int *>(d.local_rows_h + vbytes);
  }
  const double t2 = local_now_ms();
  ms[0] = t1 - t0; ms[1] = t2 - t1;
  return R;
}

}  // namespace lmp_le
