// rebuild_plan.h — which launches a reneighbor takes.  Plain host code without a device in it: Engine::reneighbor states
// what it knows when the rebuild starts (RebuildFacts, gathered in Engine::rebuild_facts), plan_rebuild answers, the stages
// of the rebuild (kernels_dd.hip rebuild_migrate / rebuild_ghosts, kernels_neigh.hip rebuild_sort / rebuild_lists) launch
// what the plan says and test no flag of DeviceState themselves.  tests/test_rebuild_plan_cpu.py restates the rules and holds
// them against plan_rebuild and against the instantiations the build dispatcher holds (with_build_kernel).
//
// Not in the plan: launches whose guard is a count the host learns only in the middle of a decomposed rebuild - arrivals
// (k_dd_arrive: narr), send lists (k_dd_pack_xt, k_dd_reorder_sends: nsall), ghosts (k_dd_ghost_bin / _slot / _sort / _place:
// m).  They stay run-time guards beside their launch.  FLAG_SPECIAL_ASYM is a fact as the host last read it: the kernels that
// raise it (LE fixes) are followed by a flag hand-over before any rebuild, and none runs inside one.
#pragma once
#include "step_plan.h"

namespace lmp_le {

constexpr int BPART_EXCL_MAX = 4;   // bond partners the list build keeps in registers as exclusions (kernels_neigh.hip SPMAX)

// Environment switches of the rebuild (experiments and tests).  Constructing a RebuildKnobs reads them - the one place that
// does; Engine::run does it once per `run` command, before setup, and the values hold for that run.
// (LAMMPS_LE_NO_ROW_TILES is a setting of the allocation, device.cpp dev_alloc: the numbering of the cells is part of the layout)
struct RebuildKnobs {
  bool build_fp64 = env_set("LAMMPS_LE_BUILD_FP64");           // every candidate of the list build takes the FP64 distance test
  int diag_build = env_int("LAMMPS_LE_DIAG_BUILD", -1);        // >= 0: an extra build into scratch outputs with these parts switched off
  bool no_direct_recv = env_set("LAMMPS_LE_NO_DIRECT_RECV");   // decomposed: halos through the receive buffer + unpack kernel
  long overflow_at = env_set("LAMMPS_LE_TEST_OVERFLOW_AT") ? atol(getenv("LAMMPS_LE_TEST_OVERFLOW_AT")) : -1;   // test hook: shrink the table before this build
  bool freeze_images = env_set("LAMMPS_LE_FREEZE_IMAGES");     // bond partner images frozen at the rebuild even where bond_minimg would hold
  bool no_xhold_alias = env_set("LAMMPS_LE_NO_XHOLD_ALIAS");   // one GPU: the rebuild stores a copy of the build-time positions (as decomposed runs do)
  bool scan_two_pass = env_set("LAMMPS_LE_SCAN_TWO_PASS");     // the cell scans with one count per thread (k_scan_local + k_scan_add) instead of four
  bool permute_all = env_set("LAMMPS_LE_PERMUTE_ALL");         // k_permute moves the velocities at every rebuild (no hand-over to the step kernel)
};

// What the engine knows when a rebuild starts.
struct RebuildFacts {
  bool decomposed = false;
  bool bins_ready = false;       // the step kernel binned the current positions (DeviceState::bins_ready)
  bool counts_dirty = false;     // cell_count holds counts no scan has consumed
  bool bonds_dirty = false;      // the packed bond records are older than the bond tables
  bool phys_valid = false;       // the packed records by physical index are current
  bool bond_minimg = false;      // the minimum image of every step is the frozen image (DeviceState::bond_minimg)
  int bpa = 0, bond_pack_stride = 4;
  bool bpart = false;            // a bond-partner table exists
  bool pair = false;             // a pair style (pair_style zero included): the list is built
  int sf[4] = {1, 1, 1, 1};      // Engine::special_flag per level, [1..3]
  bool special_asym = false;     // FLAG_SPECIAL_ASYM as last read
  int row_tile = 0;
  bool angles = false;           // an angle style is active
  bool snapshot_due = false;     // an LE fix wants the bond tables of the rebuild and they changed since the last snapshot
  bool map_stale = false;        // decomposed: map[] was not left by a rebuild
  bool sort_due = false;         // an Atom::sort falls on this rebuild
  bool can_defer = false;        // the caller enqueues a whole fused step next and looks at the build's flags behind it
  bool regrow = false;           // a list overflowed: the table grew, the lists stage runs again for the same order
  bool lazy_v = false;           // the step kernel enqueued next is the throughput shape of k_step, which can take the velocities
                                 // in the old order (Engine::reneighbor: the step plan of the iteration; one launch, every bead)
  long builds = 0;               // list builds of this run so far
};

// One bit per conditional launch and per choice; lammps_le_stat("rebuild_plan_full") returns the bits of the last plan executed,
// lammps_le_stat("rebuild_plan") the same without RB_LAZY_V (the bits lammps_le_test_rebuild_plan knows).
enum RebuildBit : unsigned {
  RB_WRAP_BIN = 1u << 0,          // k_wrap_bin
  RB_COUNT_MEMSET = 1u << 1,      // cell_count zeroed first (bins nobody consumed)
  RB_MAP_FILL = 1u << 2,          // decomposed: k_fill_int of map[]
  RB_BOND_PACK = 1u << 3,         // k_bond_pack (before the cell sort when the permute writes the table, else before k_bond_table)
  RB_BOND_PACK_PHYS = 1u << 4,    // k_bond_pack_phys
  RB_SORT_WRITES_MAP = 1u << 5,   // k_sort_cells writes map[]
  RB_PERMUTE_BONDS = 1u << 6,     // k_permute writes the bond-partner table
  RB_PREBINNED = 1u << 7,         // k_permute applies Domain::pbc (the step kernel binned)
  RB_PERMUTE_PHYS = 1u << 8,      // k_permute moves the physical bond records
  RB_BOND_TABLE = 1u << 9,        // k_bond_table
  RB_FROZEN_IMAGES = 1u << 10,    // bond partner images frozen at this rebuild (bshift written and read)
  RB_BUILD = 1u << 11,            // a list build
  RB_NOSP = 1u << 12, RB_ASYM = 1u << 13, RB_FRAC = 1u << 14,   // its template arguments: k_build_neigh<NOSP, false, FRAC> | k_build_neigh_asym<FRAC>
  RB_EXCL_BPART = 1u << 15,       // exclusions from the bond-partner table (else from the special lists)
  RB_DDCODE = 3u << 16,           // build_body's `dd` (two bits): 0 tiled rows, 1 decomposed, 2 z-major rows on one GPU
  RB_FP64 = 1u << 18,             // FP64 band: every candidate is re-tested
  RB_DIAG_BUILD = 1u << 19,       // the diagnostic build follows (RebuildPlan::diag_bits)
  RB_DIRECT_RECV = 1u << 20,      // decomposed: the senders reorder their lists to the receiver's ghost order
  RB_ANGLE_LIST = 1u << 21,       // launch_angle_list
  RB_TOPO_SNAPSHOT = 1u << 22,    // launch_topo_snapshot
  RB_CHECK_DEFERRED = 1u << 23,   // flags published, not waited for (else the synchronous check)
  RB_FORCE_OVERFLOW = 1u << 24,   // test hook: the table shrinks to 4 rows before this rebuild
  RB_ATOM_SORT = 1u << 25,        // the Atom::sort emulation between the cell sort and the lists
  RB_LAZY_V = 1u << 26,           // k_permute leaves the velocities in the old order: the step kernel that follows reads them
                                  // through perm[] and stores them in the new one (DeviceState::v_pending)
};
constexpr int RB_DDCODE_SHIFT = 16;

struct RebuildPlan {
  unsigned bits = 0;
  int diag_bits = 0;             // RB_DIAG_BUILD: the parts the diagnostic build switches off (entry stores always)
  bool decomposed = false;      // the migration, border and ghost stages run
  bool has(unsigned b) const { return (bits & b) != 0; }
  int ddcode() const { return (int)((bits & RB_DDCODE) >> RB_DDCODE_SHIFT); }
};

inline RebuildPlan plan_rebuild(const RebuildFacts &f, const RebuildKnobs &k) {
  RebuildPlan p;
  p.decomposed = f.decomposed;
  auto set = [&](unsigned bit, bool on) { if (on) p.bits |= bit; };
  // one GPU, bonds that need no frozen image: the permute pass also writes the bond-partner table (k_permute), from records
  // that travel with the beads when one int4 holds them
  const bool minimg = f.bond_minimg && !k.freeze_images;      // (Engine::run folds the switch into the fact as well)
  const bool permute_bonds = !f.decomposed && minimg && f.bpa > 0 && f.bpart;
  const bool phys = permute_bonds && f.bond_pack_stride == 4;
  if (!f.regrow) {
    set(RB_FORCE_OVERFLOW, k.overflow_at >= 0 && f.builds == k.overflow_at);
    // bins: the migration pass of a decomposed rebuild bins what stays (k_dd_leave); on one GPU the step kernel may have
    const bool prebinned = f.bins_ready && !f.decomposed;
    set(RB_PREBINNED, prebinned);
    set(RB_WRAP_BIN, !prebinned && !f.decomposed);
    set(RB_COUNT_MEMSET, f.counts_dirty && !prebinned);
    set(RB_MAP_FILL, f.decomposed && f.map_stale);
    set(RB_BOND_PACK, f.bonds_dirty);
    set(RB_BOND_PACK_PHYS, phys && (!f.phys_valid || f.bonds_dirty));     // (k_bond_pack voids the physical records)
    set(RB_SORT_WRITES_MAP | RB_PERMUTE_BONDS, permute_bonds);
    set(RB_PERMUTE_PHYS, phys);
    set(RB_DIRECT_RECV, f.decomposed && !k.no_direct_recv);
    set(RB_ATOM_SORT, f.sort_due);
    set(RB_ANGLE_LIST, f.angles);
    set(RB_TOPO_SNAPSHOT, f.snapshot_due);
    // (an Atom::sort changes the order the build stores pairs in and, decomposed, waits for the device anyway)
    set(RB_CHECK_DEFERRED, f.can_defer && !f.sort_due && !f.decomposed);
    // the velocities stay behind only where that step kernel is certain to come next, on the order this rebuild leaves
    set(RB_LAZY_V, f.lazy_v && f.can_defer && !f.sort_due && !f.decomposed && !k.permute_all);
  }
  // the lists stage.  A regrow pass re-derives the same table for the same order (a launch of its own: folded into the
  // prologue of the list build it made that kernel 48 us slower to save 16)
  set(RB_BOND_TABLE, f.regrow || !permute_bonds);
  set(RB_FROZEN_IMAGES, !minimg);
  if (f.pair) {
    const int s1 = f.sf[1], s2 = f.sf[2], s3 = f.sf[3];
    const bool nosp = s1 == 1 && s2 == 1 && s3 == 1;             // no special list at all
    const bool frac = s1 == 2 || s2 == 2 || s3 == 2;             // some special weight is neither 0 nor 1
    set(RB_BUILD, true);
    set(RB_NOSP, nosp);
    set(RB_ASYM, !nosp && f.special_asym);                       // the build that follows the reference's pair order
    set(RB_FRAC, frac && !nosp);
    // exclusions = bond partners (`special_bonds fene`-like flags, symmetric lists): read from the bond-partner table
    set(RB_EXCL_BPART, s1 == 0 && s2 == 1 && s3 == 1 && f.bpa >= 1 && f.bpa <= BPART_EXCL_MAX && !f.special_asym);
    p.bits |= (unsigned)(f.decomposed ? 1 : (f.row_tile ? 0 : 2)) << RB_DDCODE_SHIFT;
    set(RB_FP64, k.build_fp64);
    set(RB_DIAG_BUILD, k.diag_build >= 0);
    if (k.diag_build >= 0) p.diag_bits = k.diag_build | 1;
  }
  return p;
}

}  // namespace lmp_le
