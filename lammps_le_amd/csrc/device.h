// device.h — HBM layout of the engine and the kernel launchers (gfx950).
//
// Physical (p-indexed) arrays are kept in CELL order: every reneighbor re-sorts the atoms by
// neighbor cell (ties by tag), so a cell's atoms are one contiguous range and the neighbor
// gathers of the pair kernel stay inside a few L2-resident rows.  Topology (bonds, specials,
// extruder state) stays TAG-indexed and is never permuted; map[tag] -> p links the two.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <deque>
#include <string>
#include <vector>

#include <type_traits>

#include "engine.h"

namespace lmp_le {

#define HIP_CHECK(x)                                                                              \
  do {                                                                                            \
    hipError_t e_ = (x);                                                                          \
    if (e_ != hipSuccess)                                                                         \
      throw LammpsError(std::string("HIP error: ") + hipGetErrorString(e_) + " at " + __FILE__ + \
                        ":" + std::to_string(__LINE__));                                          \
  } while (0)

enum FlagSlot {
  FLAG_MOVED = 0,       // some atom moved more than skin/2 since the last build
  FLAG_ERROR = 1,       // device-side error code (see ERR_*)
  FLAG_NEIGH_OVERFLOW = 2,
  FLAG_FENE_WARN = 3,   // count of "FENE bond too long" warnings
  FLAG_TOPO_CHANGED = 4,
  FLAG_COUNT_A = 5,     // LE fix counters (created / broken)
  FLAG_COUNT_B = 6,
  FLAG_NDRAW = 7,       // number of RNG draws requested by an LE fix
  FLAG_NLIST = 8,       // number of extruder listings
  FLAG_MAXNEIGH = 9,    // largest neighbor count seen at the last build
  FLAG_AUX = 10,
  FLAG_SPECIAL_ASYM = 11,
  FLAG_RECV_UP = 12,    // decomposition: counts received from the upper / lower slab neighbour
  FLAG_RECV_DN = 13,
  FLAG_COUNT_BOTH = 14, // decomposition: beads of this rank in BOTH send lists at the last rebuild (slabs below two ghost cutoffs)
  FLAG_GHOST_MIXED = 15, // (unused)
  FLAG_RNG_MISS = 16,    // decomposition: an owned bead's Langevin draws lie in a stream segment this rank skipped (kernels_rng.hip)
  NFLAGS = 24
};
constexpr int FLAG_SEQ_SLOT = 32;   // the publish sequence number in the mapped host page: a 64-byte sector of its own
enum DevErr {
  ERR_NONE = 0, ERR_BAD_FENE = 1, ERR_BOND_MISSING = 2, ERR_EXT_MULTI = 3, ERR_BPA = 4,
  ERR_SPECIAL = 5, ERR_COUNT_MISMATCH = 6, ERR_NONFINITE = 7, ERR_SPECIAL_SCRATCH = 8, ERR_GHOST_ORDER = 9,
  ERR_HALO_TIMEOUT = 10, ERR_ANGLES = 11, ERR_WALL_OUTSIDE = 12,
  ERR_ONE_SIDED = 13     // fix extrusion: the higher end of a new bond has no free slot, the lower end has (kernels_le.hip k_ext_create)
};
// The one table code -> text (engine.cpp).  `style`: the fix that was firing when the code was raised - the reference's fixes
// each carry their own copy of the code that raises, and the copies end their texts in different names.
std::string device_error_text(int code, const std::string &style);

// z-slab decomposition: may `world` ranks share a box `prd_z` tall?  w = prd_z / world is a slab's width, cutghost =
// max(neighbor cutoff, comm_modify cutoff) the depth of a ghost shell.  Three conditions, in the order they are tested:
//   w >= cutghost                 every ghost of a rank lives on a DIRECT neighbour (thinner slabs would need multi-hop ghosts)
//   w >= 2 * cutneighmax          a bead within the pair shell (rc + skin) of one face is outside the pair shell of the other:
//                                 the two ranks that read it as a pair neighbor are distinct from each other and from its owner
//   w + 2 * cutghost <= prd_z     the shells [lo - cutghost, lo) and [hi, hi + cutghost) of a rank do not overlap around the
//                                 period (for two ranks this is w >= 2 * cutghost: thin slabs mean three or more ranks)
// Between one and two ghost cutoffs a bead can lie in the ghost shell of BOTH faces: it is then in both send lists
// (k_dd_borders, DeviceState::sendboth).  Host only; the one place the rule lives (Engine::upload, lammps_le_test_slab_rule).
enum SlabRule { SLAB_OK = 0, SLAB_BELOW_GHOST_CUTOFF = 1, SLAB_BELOW_PAIR_SHELLS = 2, SLAB_SHELLS_OVERLAP = 3 };
inline SlabRule slab_rule(double prd_z, int world, double cutneighmax, double comm_cutoff, std::string &msg) {
  const double w = prd_z / world, cutghost = std::max(cutneighmax, comm_cutoff);
  msg.clear();
  if (w < cutghost) {
    msg = "slab thinner than one ghost cutoff (slab width " + std::to_string(w) + ", ghost cutoff " + std::to_string(cutghost) +
          "): use fewer GPUs or a smaller comm_modify cutoff";
    return SLAB_BELOW_GHOST_CUTOFF;
  }
  if (w < 2.0 * cutneighmax) {
    msg = "slab thinner than two pair shells (slab width " + std::to_string(w) + ", neighbor cutoff " + std::to_string(cutneighmax) +
          "): use fewer GPUs";
    return SLAB_BELOW_PAIR_SHELLS;
  }
  if (w + 2.0 * cutghost > prd_z) {
    msg = "ghost shells of a slab overlap: box too small for this many GPUs";
    return SLAB_SHELLS_OVERLAP;
  }
  return SLAB_OK;
}

// Neighbor cells are cutneigh wide in y and z and cutneigh / CELL_XSPLIT wide in x (the fastest index of the cell
// order): the 2*CELL_XSPLIT+1 x-cells a bead has to look at are still ONE contiguous index range per (y,z) row, but
// cover 2.25 instead of 3 cutoffs -> 25 % fewer candidates in the list build.
constexpr int CELL_XSPLIT = 4;

constexpr int ANGLE_PACK_COLS = 4;
constexpr int PAIRTAB_RING = 8;
constexpr int LE_MAX_FIXES = 16;   // extrusion / ex_load / ex_unload / bond/create / bond/break instances with a device RanMars state each

// The one owner of what an instance holds on the device: device blocks, pinned host blocks, streams and events.  A record
// names the resource by the ADDRESS of the pointer field that holds it (so it follows std::swap(d.pos, d.pos_tmp) and the
// like), with its byte size (the capacity of a grow-only buffer), the field's name and its kind.  Allocating into a field
// that holds a block of this registry frees that block first; releasing nulls the field.  Not copyable, one thread at a time.
struct DevMem {
  enum Kind { DEVICE, HOST, STREAM, EVENT };
  struct Rec { void **field; size_t bytes; const char *name; Kind kind; };
  std::vector<Rec> recs;
  DevMem() = default;
  DevMem(const DevMem &) = delete;
  DevMem &operator=(const DevMem &) = delete;
  ~DevMem() { release_all(); }
  // `count` elements of device memory, zeroed unless told otherwise (null-stream memset + wait: see alloc_bytes)
  template <class T> void alloc(T *&p, size_t count, const char *name, bool zero = true) { alloc_bytes((void **)&p, count * sizeof(T), name, zero, 0); }
  // pinned host memory (`flags`: the runtime's, e.g. mapped | coherent), not zeroed
  template <class T> void alloc_host(T *&p, size_t count, const char *name, unsigned flags = 0) { alloc_bytes((void **)&p, count * sizeof(T), name, false, flags, HOST); }
  // grow-only: at least `count` elements, contents NOT kept and not zeroed; true when it (re-)allocated
  template <class T> bool reserve(T *&p, size_t count, const char *name) {
    if (count <= capacity(p)) return false;
    alloc_bytes((void **)&p, count * sizeof(T), name, false, 0);
    return true;
  }
  template <class T> size_t capacity(T *&p) const { const Rec *r = find((void **)&p); return r ? r->bytes / sizeof(T) : 0; }
  // a block allocated by other means (freed like any block of its kind)
  void adopt(void **field, size_t bytes, const char *name, Kind kind);
  void stream(hipStream_t &s, const char *name, unsigned flags, int priority = 0);
  void event(hipEvent_t &e, const char *name, unsigned flags);
  template <class T> void release(T *&p) { release_field((void **)&p); }
  void release_all(bool blocks_only = false);      // in reverse order of creation; every field is left null
  size_t device_bytes() const;
  void trace(const char *when, int rank) const;    // LAMMPS_LE_TRACE_ALLOC=1: every record to stderr
  static void live(long long out[3]);              // process-wide: live blocks, their bytes, live streams + events

 private:
  const Rec *find(void **field) const;
  void alloc_bytes(void **field, size_t bytes, const char *name, bool zero, unsigned host_flags, Kind kind = DEVICE);
  void release_field(void **field);
};
// (the record's name is the field as written at the call)
#define DEV_ALLOC(mem, field, count) (mem).alloc(field, count, #field)
#define DEV_ALLOC_RAW(mem, field, count) (mem).alloc(field, count, #field, false)      // not zeroed
#define DEV_RESERVE(mem, field, count) (mem).reserve(field, count, #field)

struct DeviceState {
  hipStream_t stream = nullptr;
  int n = 0;        // owned atoms
  int npad = 0;     // stride of the column-major (ELL) tables, multiple of 64
  int maxtag = 0;
  int ntypes = 0, bpa = 0, maxspecial = 0;
  Box box{};

  // ---- physical order ----
  double4 *pos = nullptr, *pos_tmp = nullptr;   // x y z type
  double4 *pos_hold = nullptr;                   // the third position buffer (see xhold)
  // positions at the last build (same order): a VIEW, the registry does not know it.  Decomposed runs, and every run under
  // LAMMPS_LE_NO_XHOLD_ALIAS=1: xhold == pos_hold, the rebuild stores a copy there.  One GPU otherwise (xhold_alias): the
  // buffer k_permute wrote IS the record - xhold names it, and the step kernels ping-pong between the other two, so
  // xhold == pos until the first step after a build and xhold == pos_hold from then on, never pos_tmp.  Whoever writes d.pos
  // in place goes through note_positions_replaced first, which moves d.pos off that buffer (detach_positions).  The one
  // exception: k_exload_create stores a bead's new TYPE into pos[p].w in the middle of a firing step, alias or not; under
  // the alias xhold[p].w follows it.  Nothing reads the w of xhold (the displacement tests and the LE fixes take x y z).
  double4 *xhold = nullptr;
  bool xhold_alias = false;
  bool step_rotated = false;                     // the last launch_step rotated three buffers, not two (undo_step_swap)
  float4 *posf = nullptr;                        // FP32 copy of the positions at the last reneighbor (list-build distance test)
  double *v[3] = {nullptr, nullptr, nullptr}, *v_tmp[3] = {nullptr, nullptr, nullptr};
  // velocities pending: a rebuild under RB_LAZY_V (rebuild_sort) moved every physical array but v.  d.v is then in the order
  // BEFORE that cell sort and d.perm translates - the bead in slot s has its velocity at v[k][perm[s]] - until the step
  // kernel that follows hands them over (launch_step: the LAZYV variant reads through perm, stores into v_tmp, the host
  // swaps).  The state belongs to rebuild_sort (raises it), launch_step (consumes it; undo_step_swap puts it back when the
  // launch stored nothing) and settle_velocities (permutes v with a kernel of its own).  Whoever else reads or writes d.v
  // calls settle_velocities first; inside Engine::iterate that never fires.
  bool v_pending = false;
  bool step_took_v = false;                      // the last launch_step consumed v_pending (undo_step_swap)
  long v_settled = 0;                            // launches of settle_velocities (lammps_le_stat("velocities_settled"))
  double *f[3] = {nullptr, nullptr, nullptr};
  int *tag = nullptr, *tag_tmp = nullptr;
  int *img = nullptr, *img_tmp = nullptr;        // [3][npad]
  // ---- tag order ----
  int *map = nullptr;                            // [maxtag+2] tag -> p
  int *type_t = nullptr;                         // [maxtag+2]
  int *crank = nullptr;                          // [maxtag+2] canonical (reference local) index
  int *num_bond = nullptr, *bond_type = nullptr, *bond_atom = nullptr;   // [(maxtag+2)], [*bpa]
  int *nspecial = nullptr, *special = nullptr;                            // [*3], [*maxspecial]
  // angles by tag (apa = 0: none): every atom holds a copy of each angle it is part of, atoms as IDs
  int apa = 0;
  int *num_angle = nullptr, *angle_type = nullptr, *angle_a1 = nullptr, *angle_a2 = nullptr, *angle_a3 = nullptr;
  double *partial_a = nullptr;     // [nblocks][8] angle energy + virial block sums
  int lg_bit = 1;                  // the group bit of fix langevin (DeviceState::gmask)
  bool lg_grouped = false;         // fix langevin acts on a group: its draws go by lgrank (rank among the members), not crank
  double *lgsum = nullptr;         // fix langevin `zero yes`: [nred_blocks + 1][16] block sums of the random forces + their mean
  // the angle LIST of the last reneighbor as every bead sees it (NTopoAngleAll::build, src/ntopo_angle_all.cpp:37-93): an
  // angle acts - on all three of its atoms - iff the one with the lowest local index holds a copy of it, whatever copies
  // the other two hold (copies go out of step when fix ex_unload's influence rule spares one atom).  eff_*[t]: the listed
  // angles bead t is part of, sorted, so that the force kernel is a per-bead gather with a fixed summation order.
  int ecap = 0;
  int *eff_n = nullptr;                          // [npad]
  int4 *eff_rec = nullptr;                       // [ecap][npad] = (type, i1, i2, i3) with PHYSICAL indices, column-major
  // bond tables as of the last reneighbor = the reference's neighbor->bondlist, which the LE fixes loop over
  // even when another LE fix changed the topology earlier in the same step (fix_ex_unload.cpp:223, fix_extrusion.cpp:368)
  int *num_bond0 = nullptr, *bond_type0 = nullptr, *bond_atom0 = nullptr;
  int le_snapshot = 0;             // keep the snapshot (set when an LE fix exists)
  bool topo_dirty = true;          // bond tables changed since the snapshot was taken
  // one record per tag {num_bond, (type << 26) | partner tag, ..} for the rebuild's bond-partner table: ONE line per bead
  // instead of three (num_bond, bond_type row, bond_atom row) when tag order is not memory order; refreshed when dirty
  int *bond_pack = nullptr;
  int bond_pack_stride = 0;
  bool bond_pack_dirty = true;
  // the first ANGLE_PACK_COLS stored angles of every atom as (type, a1, a2, a3) records, column-major by tag: what the angle
  // listing of every rebuild reads instead of three tables of stride apa (rebuilt after the angle tables changed)
  int *angle_pack = nullptr;
  bool angle_pack_dirty = true;
  // the same records by PHYSICAL index (one GPU, permute pass writes the bond-partner table): moved with the beads by
  // k_permute, so that the table pass reads them next to the bead's other data instead of gathering them by tag
  int *bond_pack_p[2] = {nullptr, nullptr};
  bool bond_pack_p_valid = false;
  // ---- cells / neighbor list ----
  int ncell[3] = {0, 0, 0}, ncells = 0;
  int row_tile = 0;          // (y, z) rows of cells numbered in tiles of this edge (bin_inl.h row_id); 0 = z-major (decomposed runs)
  double cellinv[3] = {0, 0, 0};
  int *cell_of = nullptr, *cell_count = nullptr, *cell_start = nullptr;
  int *scan_tmp = nullptr, *perm = nullptr;
  bool scan_two_pass = false;                    // LAMMPS_LE_SCAN_TWO_PASS=1: the cell scans one count per thread (k_scan_local + k_scan_add)
  int maxneigh = 0;
  int *neigh = nullptr;      // [maxneigh][npad] full list, special bits in the top 2 bits
  int *numneigh = nullptr;   // [npad]
  int *bpart = nullptr;      // [bpa][npad] (type << 26) | partner p ; -1 = none
  // [npad] frozen periodic image of each bond partner, BSHIFT_BITS per COMPACTED bond slot (= the bond's row in the bead's
  // list), written by k_bond_table from the positions of the build; 0 for nearly every bead (engine.h NN_SHIFTED_BIT)
  unsigned long long *bshift = nullptr;
  // 1: the minimum image of every step IS the frozen image, provably - every bond style is fene and 2 R0 < half the box,
  // so a bond component cannot reach half the box without `Bad FENE bond` ending the run at that very step (rlogarg <= -3
  // <=> r >= 2 R0); the force kernels then keep their three compares per bond and the rebuild skips the partner gathers
  // (k_bond_table: 25 instead of 56 us per rebuild at 1M beads).  0: images are frozen at the rebuild (bshift).
  int bond_minimg = 0;
  double *pairtab = nullptr; // 6 * nt*nt : cutsq lj1 lj2 lj3 lj4 offset
  int newton_pair = 0;           // `newton on [off]`: which end stores a pair in the reference's half list (ex_load's visit order)
  int ref_nbin[3] = {1, 1, 1};   // the reference's neighbor bins (cutneighmax / 2 fitted to the box, nbin_standard.cpp:53-186)
  double ref_bininv[3] = {1, 1, 1};
  bool ident_order = true;       // the reference's local index of a bead = its ID - 1 (no Atom::sort, data file in ID order)
  int sflag[4] = {1, 1, 1, 1};   // Engine::special_flag per level: 0 dropped from the list, 1 ordinary entry, 2 entry with level bits
  int pair_uniform = 0;      // every type pair has the same coefficients
  double pair_u[6] = {0, 0, 0, 0, 0, 0};
  // fix adapt, runs whose kernels read the table: PAIRTAB_RING pinned copies of it, written in turn; pairtab_ev[k] is recorded
  // behind the copy out of row k, and row k is written again only after that event (it passed long ago: the ring is deeper
  // than the host ever runs ahead of the stream between two waits of its own)
  double *pairtab_ring = nullptr;
  hipEvent_t pairtab_ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int pairtab_next = 0;
  double cutneigh = 0.0;
  // ---- thermo partial sums ----
  int nred_blocks = 0;
  double *partial = nullptr;     // [nblocks][16]
  double *partial_h = nullptr;   // pinned
  // ---- flags ----
  int *flags = nullptr;          // device
  int *flags_h = nullptr;        // pinned, mapped host copy
  int *flags_h_dev = nullptr;    // device-side address of flags_h
  bool cell_count_dirty = false; // cell_count holds counts that no scan has consumed (and zeroed) yet
  bool bins_ready = false;       // cell_of / cell_count / arrival ranks hold the bins of the CURRENT positions (written by k_step)
  int flags_seq = 0;             // sequence number of the last publish (flags_h[NFLAGS] echoes it)
  // ---- Langevin RNG (block-parallel RanMars) ----
  int rng_B = 0, rng_nblocks = 0;
  uint32_t *rng_state = nullptr;   // [nblocks][97]
  uint32_t *rng_jump = nullptr;    // coefficients of the jump polynomial(s): [97] block mode, [2][97] batch mode (full / last segment)
  uint32_t *rng_out = nullptr;     // [3N] 24-bit draws of the current call, canonical order
  uint32_t *rng_buf[2] = {nullptr, nullptr};   // double buffer: the next call's draws are generated on rng_stream
  int rng_cur = 0;
  hipStream_t rng_stream = nullptr;
  hipEvent_t rng_done[2] = {nullptr, nullptr}, rng_consumed[2] = {nullptr, nullptr};
  bool rng_ahead = false;          // rng_buf[rng_cur ^ 1] already holds the draws of the next call
  // batch generator (default): W whole calls per launch, one wavefront each, two pools alternating
  int rng_mode = 1;                // 1 = batch (k_rng_calls), 0 = block-parallel per call (k_rng_langevin)
  int rng_W = 0;
  long long rng_total = 0;         // draws per call = 3 * beads in the system
  int rng_nseg = 1;                // batch generator: segments per call (one wavefront each) and their length
  long long rng_seglen = 0;
  uint32_t *rng_wstate = nullptr;  // [3][W * S][97] windows in front of each (call, segment) of a batch: batch b reads copy b % 3, writes (b + 1) % 3
  long long rng_batch_no[2] = {0, 0};          // number of the batch each pool holds (selects the window copy it started from)
  // decomposed runs: a rank generates only the stream segments that hold draws of beads it owns or ghosts (kernels_rng.hip)
  int *rng_need = nullptr;         // [S] segments wanted by the batch about to be launched
  int *rng_gen[2] = {nullptr, nullptr};        // [S] segments each pool holds
  int *rng_late = nullptr;         // [2][S] segments the validation found missing (generated late, from the kept windows)
  bool rng_skip = false;           // segment skipping is on (decomposed, batch mode)
  uint32_t *rng_pool[2] = {nullptr, nullptr};   // [W][3N]
  uint64_t rng_batch_raw[2] = {0, 0};           // raw index of the first draw held by each pool (0 = empty)
  int rng_pool_cur = 0;
  RanMarsInt rng_origin;           // host generator at the position given to rng_langevin_setup
  // ---- LE fixes (tag order) ----
  double4 *xt = nullptr;           // [maxtag+2] stored coordinates by tag
  int *le_i[16] = {nullptr};       // integer scratch arrays [maxtag+2]
  double *le_d[2] = {nullptr};     // double scratch [maxtag+2]
  unsigned long long *le_bits = nullptr;
  uint32_t *le_rng_state = nullptr;   // [LE_MAX_FIXES][100]: w[97], n_lo, n_hi per LE fix slot
  uint32_t *le_draws = nullptr;       // [maxtag+2]
  int *le_list = nullptr;             // extruder listings [4][maxtag+2]
  int *le_scan = nullptr;
  // ---- spatial decomposition (z slabs; world > 1) ----
  int dd = 0;                      // 1 = this rank owns a z slab, ghosts at [n, n + nghost)
  int nghost = 0;
  int ntotal = 0;                  // beads in the whole system
  double slab_lo = 0.0, slab_hi = 0.0, cutghost = 0.0, zlo_ext = 0.0;
  int *gcell_start = nullptr, *gcell_count = nullptr;   // ghost ranges per cell (relative to n)
  int *sendlist[2] = {nullptr, nullptr};                // owned indices sent down / up every step
  int *sendlist_alt[2] = {nullptr, nullptr};            // ... and the buffers the next rebuild writes its reordered lists into
  int *gmask = nullptr;                                 // [maxtag+2] group bits by tag (bit 0 = all); only when a fix or a local compute acts on a group
                                                        // (uploaded with the system; refreshed in place by Engine::pair_rows for a compute defined since)
  int *lgrank = nullptr;                                // [maxtag+2] rank of a bead among the members of fix langevin's group (local order)
  WallTable *walltab_dev = nullptr;                     // fix wall/region: this run's table (k_wall, the wall variant of k_step)
  double *wall_partial = nullptr;                       // [WALL_MAX][nred_blocks + 1][16] block sums of k_wall<EFLAG> + their totals
  double *indent_partial = nullptr;                     // [INDENT_MAX][nred_blocks + 1][16] block sums of k_indent<EFLAG> + their totals
  int indent_count = 0;                                 // fix indent instances of this run : what a fused launch must carry
  // fix spring/self | addforce | setforce: this run's table (k_fixforce, the EXT variant of k_step); one block of unwrapped
  // origins per spring/self fix, [3][ntotal + 1] by tag, never permuted, whole on every rank of a decomposed run
  ForceOpTable *forceoptab_dev = nullptr;
  double *forceop_origin[FORCEOP_MAX] = {nullptr};
  bool forceop_grouped = false;                         // an entry of the table acts on a group other than all
  ForceOpTable forceoptab_last{};                       // the table those sums belong to (origin addresses nulled) and the bead count:
  int forceop_rows_n = -1;                              //   the rows are kept over a `run` command while both stay the same
  double *forceop_partial = nullptr;                    // [FORCEOP_MAX][nred_blocks + 1][16] block sums of k_fixforce<EFLAG> + their totals
  AngleTable *angtab_dev = nullptr;                     // this run's table in device memory (fused angle step)
  bool ghost_whole_shell = false;                       // every bead within the ghost cutoff of a face is sent (runs with an angle style)
  bool map_stale = true;                                // map[] was not left by a decomposed rebuild: fill it before the next one
  int nsend[2] = {0, 0}, nrecv[2] = {0, 0};
  double4 *sendbuf = nullptr, *recvbuf = nullptr;       // halo staging
  int *gone = nullptr;                                  // [npad] 1 = this bead has just left for another slab
  // halo / compute overlap: beads that are sent to a neighbour or read a ghost form phase 1 of a step, the rest
  // (phase 0) is computed while the ghost positions of the next step travel on comm_stream
  unsigned char *phase = nullptr;                       // [npad]
  int *sendslot = nullptr;                              // [npad] slot of a border bead in its send list (bit 30 = upper list), -1 = none,
                                                        // <= -2: in both lists, entry -2 - sendslot[p] of sendboth
  int *sendboth = nullptr;                              // [2 * npad] {slot in the lower list, slot in the upper list} of a bead in both:
                                                        // a view, sendslot + npad (the step kernel finds it without an argument of its own)
  int nsend_both = 0;                                   // ... and how many there are since the last rebuild (lammps_le_stat)
  long halo_pack_launches = 0;                          // k_dd_pack launches of dd_halo since the handle was opened (lammps_le_stat)
  bool direct_recv = false;                             // send lists are in the receiver's sorted ghost order: a halo lands in place
  bool packed_ahead = false;                            // the step kernel already wrote the border beads' new positions into sendbuf
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_phase1 = nullptr, ev_halo = nullptr;
  bool halo_inflight = false;                           // ev_halo guards ghost slots that comm_stream is filling
  bool halo_ahead = false;                              // ghosts of the coming step were already exchanged
  // Peer windows (kernels_dd.hip "fast halo"): the per-step halo as a side effect of the step kernel.  Every rank owns a
  // window [parity 2][side 2: from below, from above][halo_cap] of positions plus two arrival counters; the neighbours
  // map it (hipIpcOpenMemHandle, or the plain pointer when the ranks are threads of one process) and their step kernels
  // store the new positions of their border beads straight into it, in this rank's sorted ghost order.
  double4 *halo_win = nullptr;
  unsigned *halo_flag = nullptr;                        // [2] arrival counters: [0] written by the rank below, [1] by the rank above
  bool halo_fused = false;                              // counters + window copy in one launch (every neighbour is another GPU)
  size_t halo_cap = 0;
  double4 *peer_win[2] = {nullptr, nullptr};            // the windows of the rank below / above
  unsigned *peer_flag[2] = {nullptr, nullptr};          // ... and the counter of theirs that is mine to write
  void *peer_base[2] = {nullptr, nullptr};              // what hipIpcOpenMemHandle returned (to close), nullptr for plain pointers
  bool fast_halo = false;                               // windows mapped AND switched on for this run (Engine::run re-reads the switch)
  bool halo_mapped = false, halo_verify = false;
  unsigned halo_seq = 0;                                // completed window exchanges (same on every rank)
  int packed_peer = 0;                                  // the last step kernel stored into the neighbours' windows (parity + 1)
  double halo_timeout_s = 120.0;
  int *gdest = nullptr;                                 // arrival order -> sorted ghost slot
  int *gtag_in = nullptr;                               // ghost tags in arrival order
  double *migbuf[2] = {nullptr, nullptr}, *migin = nullptr;   // migrating beads (MIG_W doubles each)
  double4 *xht = nullptr;                               // [maxtag+2] xhold by tag (LE fixes)
  double *gather_send = nullptr, *gather_recv = nullptr;      // whole-system gathers (grow-only; gather_recv is a view into it)
  // kernels_sort.hip: key / value / temp buffers of the Atom::sort emulation (grow-only)
  unsigned long long *sort_keys[2] = {nullptr, nullptr};
  int *sort_vals[2] = {nullptr, nullptr};
  char *sort_temp = nullptr;
  double *respa_flevel[8] = {nullptr};   // run_style respa: the forces of each level, by tag (Engine::respa_setup)
  Comm *comm_watch = nullptr;     // decomposed runs: host waits on the stream go through Comm::wait_stream (time-out + abort)
  // ---- kernel timing (HIP events on the launch stream) ----
  std::deque<hipEvent_t> ev0, ev1;      // (a deque: the registry keeps the address of every element)
  size_t ev_used = 0;
  // ---- C-ABI subset calls (kernels_capi.hip): staging block of the K requested rows ----
  char *capi_buf = nullptr;     // grow-only
  // ---- pair rows of the local computes (kernels_local.hip): counts and row offsets by tag, the rows, their pinned host copy (grow-only) ----
  int *local_count = nullptr, *local_offset = nullptr;   // [maxtag+2]
  char *local_scan_tmp = nullptr;
  char *local_rows = nullptr;       // [R][6] doubles (PAIR kind), then [R][4] ints
  char *local_rows_h = nullptr;     // pinned
  // ---- minimize (kernels_min.hip): x0, g, h by tag [3][maxtag + 2], allocated by `minimize` and released at its end; the block
  // partials of the dot products; the record of one evaluation in mapped host memory (the last two also serve fmax / fnorm) ----
  double *min_x0 = nullptr, *min_g = nullptr, *min_h = nullptr;
  double *min_partial = nullptr;    // [blocks + 1][MIN_DOT_COLS]
  double *min_rec = nullptr;        // [MIN_REC_MAX] pinned, mapped
  double *min_rec_dev = nullptr;    // its device-side address (a view)
  // ---- launch census: launches of k_step<KEY> by KEY and of k_force by force_variant_key (step_plan.h), host memory,
  // over the life of the handle (the diagnostic launch and the relaunch behind regrow_lists count); read by the test hooks
  // lammps_le_test_step_census* (capi.cpp) and written out by ~Engine under LAMMPS_LE_STEP_CENSUS_FILE ----
  unsigned step_census[STEP_KEY_SPACE] = {0};
  unsigned force_census[FORCE_KEY_SPACE] = {0};
  long host_waits = 0;              // times the host waited for the stream or a flag publish (lammps_le_stat "min_host_waits" is a difference)
  // owns every pointer (but the mapped peer windows), stream and event above.  The LAST member: destroyed first, while the
  // fields its records point at are still there
  DevMem mem;
};

// minimize: the columns of a dots pass (the first MIN_NSUM are sums, the others maxima), the record's capacity and the
// totals of other reductions that travel with it (each `len` doubles in device memory, appended behind the dots)
enum MinDotCol { MIN_FF = 0, MIN_FH = 1, MIN_FG = 2, MIN_FMAX2 = 3, MIN_FMAXC = 4, MIN_HMAXC = 5 };
constexpr int MIN_NSUM = 3, MIN_DOT_USED = 6, MIN_DOT_COLS = 8, MIN_REC_MAX = 256, MIN_SRC_MAX = 20;
struct MinSources {
  int n = 0;
  const double *ptr[MIN_SRC_MAX] = {nullptr};
  int len[MIN_SRC_MAX] = {0};
  void add(const double *p, int l) { if (n >= MIN_SRC_MAX) throw LammpsError("internal: too many sources for the minimiser's record"); ptr[n] = p; len[n++] = l; }
};

// with_flags(f, a, b, ...) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}, ...): where the launchers turn run-time
// flags into template arguments.  f is a generic lambda; `if constexpr` inside it keeps combinations that do not exist
// from being instantiated.
template <class F> inline void with_flags(F &&f) { f(); }
template <class F, class... Rest> inline void with_flags(F &&f, bool b, Rest... rest) {
  if (b) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}

// ------------------------------- launchers (kernels_*.hip) -------------------------------------
void dev_alloc(DeviceState &d, int n, int maxtag, int ntypes, int bpa, int maxspecial, const Box &box,
               double cutneigh);
void dev_free(DeviceState &d);
// d.halo_win: `bytes` of device memory that a peer GPU may store into while kernels of this one run; false: none to be had
bool dev_alloc_halo_window(DeviceState &d, size_t bytes);
void dev_alloc_neigh(DeviceState &d, int maxneigh);

// integrate (kernels_md.hip)
void launch_initial_integrate(DeviceState &d, const TypeTables &tt, double dtv, double triggersq, bool check, int groupbit = 1);
void launch_force(DeviceState &d, const BondTable &bt, const double special_lj[4], bool eflag, bool has_pair, int parts = 3, bool soft = false);
void launch_flevel_copy(DeviceState &d, double *flevel, bool to_level, bool add);
// the fused step kernel: the variant `plan` names (step_plan.h), fused force + Langevin + final_integrate [+ the next
// initial_integrate]; what a launch needs beyond the plan and the device state:
struct StepArgs {
  const BondTable *bt = nullptr;
  const double *special_lj = nullptr;
  const TypeTables *tt = nullptr;
  double dtv = 0.0, triggersq = 0.0;
  hipEvent_t ev_start = nullptr, ev_stop = nullptr;   // sampled launches: the kernel's own begin / end timestamps
  bool swap_buffers = true;                           // a `next` launch leaves the new positions in d.pos
  unsigned ext_active = 0;                            // EXT: bit k - entry k of the force-op table acts on this step (addforce `every`)
  const IndentTable *indents = nullptr;               // INDENT: the indenters of the step whose forces the launch computes (copied into the launch)
};
void launch_step(DeviceState &d, const StepPlan &plan, const StepArgs &args);
void launch_langevin(DeviceState &d, const TypeTables &tt, bool identity_rank, bool fuse_final, int groupbit = 1);
// `zero yes`: after launch_langevin and before the draws are released - the members' mean random force off every member
void launch_langevin_zero(DeviceState &d, const TypeTables &tt, bool identity_rank, int groupbit, long members,
                          double *host_sum3 = nullptr);
void launch_langevin_zero_apply(DeviceState &d, int groupbit, const double *mean3);
void launch_final_integrate(DeviceState &d, const TypeTables &tt, int groupbit = 1);
void launch_ke(DeviceState &d, const TypeTables &tt);
// sum(m v_i v_j) over the owned beads, order xx yy zz xy xz yz (the kinetic part of the pressure tensor); synchronous
void ke_tensor(DeviceState &d, const TypeTables &tt, double *out6);
// angle forces added to f (after launch_force); eflag: energy / virial thirds into partial_a (reduce_angle_partials)
void launch_angle(DeviceState &d, const AngleTable &at, bool eflag, bool overwrite = false);
void launch_angle_list(DeviceState &d);       // at every reneighbor of a run with an angle style
void upload_angle_table(DeviceState &d, const AngleTable &at);   // before the first fused step of a run with an angle style
void reduce_angle_partials(DeviceState &d, double *out8);
// fix wall/region (kernels_md.hip): the table of a run; the walls of one place among the post-force fixes added to f (eflag:
// with the ten block sums per wall)
void upload_wall_table(DeviceState &d, const WallTable &wt);
void launch_wall(DeviceState &d, const WallTable &wt, int phase, bool eflag);
// fix indent (kernels_md.hip): the rows of block sums of a run; the indenters of one place among the post-force fixes added to f -
// the table goes by value with the launch (eflag: with the four block sums per indenter)
void reserve_indent_partials(DeviceState &d);
void launch_indent(DeviceState &d, const IndentTable &it, int phase, bool eflag);
// fix spring/self | addforce | setforce (kernels_md.hip): the table of a run with the origin blocks (`origins[k]`: the host
// block [natoms][3] of entry k, null for an entry that has none; the table's entries get the device addresses); the entries of
// one phase applied to f in table order (`active`: bit k - entry k acts on this step; eflag: with the ten block sums per entry)
void upload_forceop_table(DeviceState &d, ForceOpTable &ft, const double *const *origins, int natoms);
void launch_fixforce(DeviceState &d, const ForceOpTable &ft, int phase, unsigned active, bool eflag);
// the block sums of one of these families (wall_partial | indent_partial | forceop_partial) on the host: rows of 16 per wall,
// indenter or entry (synchronises the stream)
void reduce_rows(DeviceState &d, double *partial, int n, double *out);
// reductions: returns sums of `partial` columns on the host (synchronises the stream)
void reduce_partials(DeviceState &d, double *out16);

// the same sums left in device memory without a copy or a wait (the totals land in the spare row of each table): where they
// are, for a record that collects them (kernels_min.hip k_min_collect)
void enqueue_thermo_sums(DeviceState &d, const PostForce &pf, bool angles, MinSources &src);

// minimize (kernels_min.hip).  min_alloc: the partials and the record, with `vectors` also x0 g h; min_free releases the
// vectors and, with `all`, the rest.
// launch_min_move raises FLAG_MOVED by the rule of k_initial_integrate; launch_min_dots fills the block partials of a dots
// pass (with_g / with_h: the vectors exist and are read); launch_min_direction those of g.h and max |h| (cg) or sets h = f (sd);
// launch_min_collect adds the partials up (dots) and writes them and the sources into d.min_rec: valid after the next wait
void min_alloc(DeviceState &d, bool vectors);
void min_free(DeviceState &d, bool all);
void launch_min_store(DeviceState &d);
void launch_min_move(DeviceState &d, double alpha, double triggersq);
void launch_min_reset_coords(DeviceState &d);
void launch_min_dots(DeviceState &d, bool with_g, bool with_h);
void launch_min_direction(DeviceState &d, bool cg, double beta);
void launch_min_h_is_g(DeviceState &d);
void launch_min_collect(DeviceState &d, bool dots, const MinSources &src);

// neighbor (kernels_neigh.hip, kernels_dd.hip): the stages of a rebuild in the order Engine::reneighbor runs them; each
// launches what the plan says (rebuild_plan.h).  Decomposed runs: rebuild_migrate (ownership; returns the slots to bin and
// the beads that remain), rebuild_sort, rebuild_ghosts (borders, ghosts into cell order); one GPU: rebuild_sort alone.  Then
// the Atom::sort emulation where it is due, then rebuild_lists.
struct Comm;
void rebuild_migrate(DeviceState &d, Comm &comm, const RebuildPlan &plan, int &m_in, int &n_out);
void rebuild_sort(DeviceState &d, const RebuildPlan &plan, int m_in, int n_out, const int *gone);
void rebuild_ghosts(DeviceState &d, Comm &comm, const RebuildPlan &plan, double cutneighsq);
void rebuild_lists(DeviceState &d, const RebuildPlan &plan, double cutneighsq);
void scan_cells(DeviceState &d, int *count, int *start, int nc, int total);   // start[0..nc] := exclusive scan of count[0..nc), count := 0

// The flags of DeviceState a rebuild plans from (bins_ready, cell_count_dirty, bond_pack_dirty, bond_pack_p_valid, topo_dirty,
// map_stale) are raised from outside the rebuild through these and cleared by the rebuild's stages alone.
inline void note_topology_changed(DeviceState &d) { d.topo_dirty = d.bond_pack_dirty = d.angle_pack_dirty = true; }   // bond / angle tables edited
// xhold_alias: d.pos leaves the buffer that records the build (copy into the free buffer, on the stream) - before anything
// writes d.pos in place.  A no-op once a step kernel has run since the build, i.e. on every plain step.
void detach_positions(DeviceState &d);
// positions are about to be written in place, or replaced: bins a step kernel left behind belong to the old positions
inline void note_positions_replaced(DeviceState &d) { d.bins_ready = false; detach_positions(d); }
// a launch of the step kernel moved on to the other position buffer; the one that records the build is never the next target
inline void note_step_swapped(DeviceState &d) {
  std::swap(d.pos, d.pos_tmp);
  d.step_rotated = d.pos_tmp == d.xhold;
  if (d.step_rotated) std::swap(d.pos_tmp, d.pos_hold);
}
inline void undo_step_swap(DeviceState &d) {       // the launch stored nothing (a list had overflowed): back to the state before it
  if (d.step_rotated) std::swap(d.pos_tmp, d.pos_hold);
  std::swap(d.pos, d.pos_tmp);
  d.step_rotated = false;
  // (the velocities it was to hand over are where they were, perm[] too: the relaunch takes the same arguments)
  if (d.step_took_v) { for (int k = 0; k < 3; k++) std::swap(d.v[k], d.v_tmp[k]); d.v_pending = true; d.step_took_v = false; }
}
// d.v in the order of the other physical arrays: a no-op unless a rebuild left the velocities pending (DeviceState::v_pending)
// and no step kernel has taken them since; then one small kernel on the stream (kernels_neigh.hip)
void settle_velocities(DeviceState &d);
// Engine::run, once per `run` command: the mode of this run.  Leaving the alias mode gives xhold its own buffer back.
void set_xhold_alias(DeviceState &d, bool on);
inline void note_order_replaced(DeviceState &d) { d.bins_ready = false; d.bond_pack_p_valid = false; }   // the arrays are (about to be) refilled in another order
inline void note_arrays_allocated(DeviceState &d) {      // dev_alloc: zeroed cell counts, no packed records yet
  note_order_replaced(d);
  d.v_pending = d.step_took_v = false;
  d.cell_count_dirty = false;
  d.bond_pack_dirty = true;
}
inline void note_map_allocated(DeviceState &d) { d.map_stale = true; }            // dd_alloc: map[] may hold anything
inline void note_step_binned(DeviceState &d, bool binned) {                        // launch_step: the kernel bins (or not) what it moves
  if (binned) d.cell_count_dirty = true;
  d.bins_ready = binned;
}

// Atom::sort emulation (kernels_sort.hip): crank[tag] := rank in the reference's sorted local order
void launch_atom_sort(DeviceState &d, const int nb[3], const double binv[3], bool by_tag = false);

// rng (kernels_rng.hip)
void rng_langevin_setup(DeviceState &d, RanMarsInt &host_rng, int natoms);
void launch_rng_langevin(DeviceState &d, uint64_t first_raw);
void rng_langevin_consumed(DeviceState &d);
// decomposed runs, after every change of ownership or of the canonical ranks (rebuild with migration, Atom::sort): do the
// pools hold the draws of every owned bead?  Enqueues the check; rng_late_generate() (after the flags reached the host)
// produces what was missing before the next step consumes it
void rng_validate_owned(DeviceState &d);
// the same check as kernel arguments, for a kernel that walks the owned beads anyway (late == nullptr: nothing to check)
struct RngValidateArgs {
  const int *crank;
  long long seglen;
  int nseg;
  const int *gen0, *gen1;
  int live0, live1;
  int *late;
};
RngValidateArgs rng_validate_args(DeviceState &d);
__device__ __forceinline__ void rng_validate_bead(const RngValidateArgs &V, int t, int *__restrict__ flags) {
  const long long r = V.crank ? V.crank[t] : t - 1;
  const int sg = (int)((3 * r) / V.seglen);
  if (V.live0 && !V.gen0[sg]) { V.late[sg] = 1; flags[FLAG_RNG_MISS] = 1; }
  if (V.live1 && !V.gen1[sg]) { V.late[V.nseg + sg] = 1; flags[FLAG_RNG_MISS] = 1; }
}
void rng_late_generate(DeviceState &d);
int rng_segments_held(DeviceState &d);
void launch_ranmars_gen(DeviceState &d, int slot, const int *count_ptr, uint32_t *out, int maxout);

// LE fixes (kernels_le.hip)
struct ExLoadParams {
  int iatomtype, jatomtype, imaxbond, inewtype, jmaxbond, jnewtype, btype;
  double cutsq, fraction;
  int atype;        // angle type created around every new bond (0: none)
  int groupbit = 1; // both atoms of a candidate pair must be in the fix's group (fix_ex_load.cpp:435,450)
};
struct ExUnloadParams {
  int btype;
  double cutsq, fraction;
  int angleflag;    // angles exist: a broken bond takes the angles it is part of with it (fix_ex_unload.cpp:149-152)
  int groupbit = 1; // both ends of a bond must be in the fix's group (fix_ex_unload.cpp:228-229)
};
struct ExtrusionParams {
  int neutral, ctcf_left, ctcf_right, ctcf_lr, btype;
  double through_prob;
  int groupbit = 1; // both ends of an extruder bond must be in the fix's group (fix_extrusion.cpp:373-376)
};
void le_rng_upload(DeviceState &d, int slot, const RanMarsInt &r);
void le_rng_download(DeviceState &d, int slot, RanMarsInt &r);
// each returns after enqueueing; counters are read back by the caller through flags_h
void launch_topo_snapshot(DeviceState &d);   // num_bond0 / bond_type0 / bond_atom0 := current bond tables
struct Comm;
void launch_ex_load(DeviceState &d, const ExLoadParams &p, int rng_slot, Comm *comm);
// stock fix bond/create: `bondcount` (host, by tag, nt ints) goes up before the launch; bond_create_counts fetches it back
struct Comm;
void launch_bond_create(DeviceState &d, const ExLoadParams &p, int rng_slot, const int *bondcount, int nt, Comm *comm);
void bond_create_counts(DeviceState &d, int *bondcount, int nt);
void launch_ex_unload(DeviceState &d, const ExUnloadParams &p, int rng_slot);
void launch_extrusion(DeviceState &d, const ExtrusionParams &p, int rng_slot);
void dd_halo_wait(DeviceState &d);   // kernels_dd.hip: the main stream waits for a halo in flight on comm_stream
void stream_sync(DeviceState &d);    // wait for d.stream; with ranks: bounded (Comm::wait_stream)
void sync_flags(DeviceState &d, unsigned reset_mask = 0);   // copy flags to flags_h, zero the masked ones, wait
void publish_flags(DeviceState &d, unsigned reset_mask = 0);   // the same without waiting ...
void wait_flags(DeviceState &d);                               // ... and the wait for the last publish
void scan_exclusive(DeviceState &d, const int *in, int *out, int m, int total_flag);
void dd_alloc(DeviceState &d, int world);
// Decomposed runs, canonical visit order (local index = ID - 1, newton_pair off): the LE fixes work from owner-computed
// bits and O(extruders) position records instead of an all-gather of every bead's (tag, x, xhold) (kernels_dd.hip
// dd_gather_needed, kernels_le.hip launch_ex_load).  Other visit orders keep the whole-system gather.
inline bool dd_le_fast(const DeviceState &d) { return d.dd && d.ident_order && !d.newton_pair && !getenv("LAMMPS_LE_DD_FULL_GATHER"); }

// ID-addressed rows for the C-ABI subset calls (kernels_capi.hip).  ids: K tags in 1..natoms (host memory).
// SUBSET_X: x (double, 3); SUBSET_V3: v (which 0) or f (which 1) (double, 3); SUBSET_IMG3 / SUBSET_IMG1: image flags unpacked /
// packed (int, 3 / 1); SUBSET_TAGTAB: row t of the tag-indexed int table `tab` of width `count` (gather only); SUBSET_TYPE:
// type (scatter only).  Gather: `found[i]` = 1 where this rank holds row i (always, for a tag table); rows it does not hold
// are left unwritten.  Scatter writes the rows this rank owns.  Both synchronise the stream.
enum SubsetProp { SUBSET_X = 0, SUBSET_V3 = 1, SUBSET_IMG3 = 2, SUBSET_IMG1 = 3, SUBSET_TAGTAB = 4, SUBSET_TYPE = 5 };
void subset_gather(DeviceState &d, int prop, int which, const int *tab, int count, int K, const int *ids, void *out_rows,
                   int *found);
void subset_scatter(DeviceState &d, int prop, int which, int count, int K, const int *ids, const void *rows);

// pair rows of compute property/local (NEIGH / PAIR kind) and compute pair/local on this rank (kernels_local.hip): `pair` = the
// PAIR kind (rsq < cutsq at the current positions, with values), `bit` = the compute's group, `zero` = pair_style zero
struct LocalRowsRequest {
  bool pair = false, zero = false;
  int bit = 1;
  double zero_cutsq = 0.0;
  double special_lj[4] = {1.0, 0.0, 0.0, 0.0};
};
long local_pair_rows(DeviceState &d, const LocalRowsRequest &rq, const int *&ids, const double *&vals, double ms[2]);

}  // namespace lmp_le
