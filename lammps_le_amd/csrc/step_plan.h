// step_plan.h — which instantiation of the fused step kernel (k_step, kernels_md.hip) a time step takes, or that it takes
// the unfused kernels.  Plain host code without a device in it: Engine::iterate states what it knows about the step
// (StepRequest), plan_step answers, launch_step launches what the plan says.  The set of instantiations that exist is
// step_variant_exists (below), a rule on the one integer that names an instantiation; tests/test_step_plan_cpu.py holds the two
// against each other.
#pragma once
#include <cstdlib>

namespace lmp_le {

constexpr int AHEAD_MAX_BEADS = 64000;   // k_step: partner / first-stage loads issued ahead of their use up to this size
constexpr int LPB4_MAX_BEADS = 50000;    // k_step: four lanes per bead up to this many (owned) beads, see k_step

// Environment switches of the step kernel (experiments and tests).  Constructing a StepKnobs reads them - the one place
// that does; Engine::iterate does it once per `run` command and the values hold for that run.
inline int env_int(const char *name, int dflt) { const char *v = getenv(name); return v ? atoi(v) : dflt; }
inline bool env_set(const char *name) { return getenv(name) != nullptr; }
struct StepKnobs {
  int lpb = env_int("LAMMPS_LE_LPB", 0);                              // 1 | 4: lanes per bead whatever the size (0: by size)
  int lpb_max_n = env_int("LAMMPS_LE_LPB_MAX_N", LPB4_MAX_BEADS);     // four lanes per bead up to this many owned beads
  int ahead_max_n = env_int("LAMMPS_LE_AHEAD_MAX_N", AHEAD_MAX_BEADS);   // loads issued ahead of their use up to this size
  bool no_fuse = env_set("LAMMPS_LE_NO_FUSE");                        // unfused integrate / force / Langevin kernels
  bool no_fused_thermo = env_set("LAMMPS_LE_NO_FUSED_THERMO");        // thermo steps through k_force<EFLAG> + k_langevin
  bool no_fused_groups = env_set("LAMMPS_LE_NO_FUSED_GROUPS");        // fixes on groups through the unfused kernels
  bool no_fused_bin = env_set("LAMMPS_LE_NO_FUSED_BIN");              // k_wrap_bin instead of binning in the step kernel
  unsigned lds_pad = (unsigned)env_int("LAMMPS_LE_STEP_LDS_PAD", 0);  // bytes of unused dynamic LDS per workgroup, to lower the occupancy on purpose
  int diag_step = env_int("LAMMPS_LE_DIAG_STEP", 0);                  // bits: an extra launch with parts switched off before the real one (launch_step)
};

// What the engine knows about the step.  langevin: a fix langevin acts; next: another step follows, its initial_integrate rides
// along (no forces are stored); ident: the reference's local index of a bead is its ID - 1; pair: a pair style; angles: an
// angle style is active; thermo: thermo output after this step, energies and virial are wanted; check: the displacement test
// of Neighbor::check_distance is due; cells: the cell tables the binning writes are allocated; walls: fix wall/region - 0 none,
// 1 walls the step kernel can take (every one on group all), 2 walls that force the unfused kernels (one of them on a group);
// soft: the pair style is soft, not lj/cut (pair is set as well); ext: fix spring/self, addforce or setforce act (on any group);
// indents: fix indent, coded as walls - 0 none, 1 every one on group all, 2 one of them on a group
struct StepRequest {
  bool langevin = false, next = false, ident = false, pair = false, angles = false, thermo = false, check = false, cells = false;
  int nvebit = 1, lgbit = 1; // group bits of fix nve / fix langevin (1 = all)
  int which = -1;            // decomposed runs with halo / compute overlap: the phase this launch handles (-1: every bead)
  int walls = 0;
  int indents = 0;
  bool soft = false;
  bool ext = false;
};

struct StepPlan {
  bool fused = false;        // false: not covered by the step kernel, take the unfused kernels (nothing below means anything)
  // the bits of the instantiation's key (step_plan_key) but one: SK_LAZYV is decided at the launch (takes_pending_v)
  bool langevin = false, next = false, ident = false, pair = false;
  int lpb = 1;
  bool diag = false, ahead = false, ang = false, ef = false, grp = false;
  bool wall = false;         // fix wall/region evaluated inside the kernel (wall_force); also set with `indent`
  bool indent = false;       // fix indent evaluated inside the kernel (indent_force): the wall variant with the launch's indenters
  bool soft = false;         // pair_style soft: the soft functor of pair_term
  bool ext = false;          // fix spring/self | addforce | setforce evaluated inside the kernel (forceops_on_bead)
  bool bin = false;          // positions binned by this launch
  bool member_ranks = false; // the draws go by the rank among the members of fix langevin's group, not by the canonical rank
  int diag_bits = 0;         // != 0: the diagnostic launch (L N I P DIAG, key 47) goes first, with these parts switched off
  unsigned lds_pad = 0;
  int which = -1, nvebit = 1, lgbit = 1;     // run-time arguments that come with the request
  bool check = false;
};

inline StepPlan plan_step(int n_owned, bool decomposed, const StepRequest &r, const StepKnobs &k) {
  const StepPlan unfused;
  StepPlan p;
  if (k.no_fuse) return unfused;
  // lanes per bead: 4 while the launch is latency-bound (few wavefronts per SIMD), 1 once it is throughput-bound
  const bool want_lpb4 = k.lpb ? k.lpb == 4 : n_owned <= k.lpb_max_n;
  const bool want_ahead = n_owned <= k.ahead_max_n;
  p.langevin = r.langevin; p.next = r.next; p.ident = r.ident; p.pair = r.pair;
  p.which = r.which; p.nvebit = r.nvebit; p.lgbit = r.lgbit; p.check = r.check; p.lds_pad = k.lds_pad;
  p.grp = r.nvebit != 1 || r.lgbit != 1;
  const bool confined = r.walls || r.indents;
  if (confined) {
    // fix wall/region, fix indent: the wall variant covers the plain steps of a run whose walls and indenters all act on group
    // all, with a pair style, no angle style and no fix on a group; thermo steps (the fixes' sums) and everything else take
    // k_wall and k_indent
    if (r.walls == 2 || r.indents == 2 || p.grp || r.thermo || r.angles || !r.pair) return unfused;
    p.wall = true;
    p.indent = r.indents != 0;      // (a run with indenters alone carries a wall table with n = 0)
  }
  if (r.soft) {
    // pair_style soft: the soft variant covers what the wall variant covers - plain steps, no angle style, no fix on a group -
    // and not together with walls; thermo steps and everything else take k_force<.., SOFT>
    if (!r.pair || confined || p.grp || r.thermo || r.angles) return unfused;
    p.soft = true;
  }
  if (r.ext) {
    // fix spring/self | addforce | setforce: the EXT variant covers what the wall variant covers - plain steps with a pair style,
    // no angle style, no fix nve / langevin on a group - and not together with walls or pair_style soft; the fixes' own groups
    // are tested inside the kernel.  Thermo steps (the fixes' sums) and everything else take k_fixforce
    if (!r.pair || confined || r.soft || p.grp || r.thermo || r.angles) return unfused;
    p.ext = true;
  }
  if (p.grp) {
    // fix nve / fix langevin on a group: one lane per bead, ranks from a table; with an angle style only the throughput shape
    // (the look-ahead shape of small systems has no group + angle instantiation); thermo steps take the unfused kernels
    if (!r.pair || k.no_fused_groups || (r.angles && want_ahead) || r.thermo) return unfused;
    p.ident = false; p.ang = r.angles;
    p.member_ranks = r.lgbit != 1;
  } else if (r.thermo) {
    // a thermo step as ONE pass (the energy variant): one GPU, a pair style, the throughput shape of the kernel
    if (!r.pair || decomposed || want_lpb4 || want_ahead || r.angles || k.no_fused_thermo || r.which >= 0) return unfused;
    p.next = false; p.ef = true; p.check = false;
  } else if (r.angles) {
    if (!r.pair) return unfused;       // (no pair style: force kernel -> angle kernel -> integrate kernels)
    p.ang = true; p.ahead = want_ahead;
  } else if (want_lpb4) {
    p.lpb = 4; p.ahead = true;
  } else {
    p.ahead = want_ahead;
  }
  p.fused = true;
  // positions binned by this launch: single GPU, whole-step launch with a displacement test in it, one lane per bead (with
  // four lanes per bead - small systems - it was measured slower than the separate k_wrap_bin: 62.2k vs 64.5k steps/s at 32k)
  p.bin = p.check && p.next && !decomposed && r.which < 0 && p.lpb != 4 && !k.no_fused_bin && r.cells;
  if (k.diag_step && r.langevin && r.next && r.ident && r.pair && r.which < 0 && p.lpb != 4 && !p.ef && !p.wall && !p.soft && !p.ext) p.diag_bits = k.diag_step;
  return p;
}

// The identity of an instantiation of k_step: one integer, the template argument of k_step<KEY> and the key of the launch
// census (DeviceState::step_census).  The bits are named here and nowhere else; their values are recorded in profiles/ and in
// the tables of the tests, so they stay.  SK_LPB4: four lanes per bead (StepPlan::lpb == 4), clear: one
enum StepKeyBit : int {
  SK_LANGEVIN = 1 << 0, SK_NEXT = 1 << 1, SK_IDENT = 1 << 2, SK_PAIR = 1 << 3, SK_LPB4 = 1 << 4, SK_DIAG = 1 << 5, SK_AHEAD = 1 << 6,
  SK_ANG = 1 << 7, SK_EF = 1 << 8, SK_GRP = 1 << 9, SK_LAZYV = 1 << 10, SK_WALL = 1 << 11, SK_SOFT = 1 << 12, SK_EXT = 1 << 13,
  SK_INDENT = 1 << 14
};
constexpr int STEP_KEY_BITS = 15, STEP_KEY_SPACE = 1 << STEP_KEY_BITS;
// The key of the instantiation a plan names; lazy_v: the launch takes velocities a rebuild left pending (takes_pending_v)
inline int step_plan_key(const StepPlan &p, bool lazy_v) {
  return (p.langevin ? SK_LANGEVIN : 0) | (p.next ? SK_NEXT : 0) | (p.ident ? SK_IDENT : 0) | (p.pair ? SK_PAIR : 0) |
         (p.lpb == 4 ? SK_LPB4 : 0) | (p.diag ? SK_DIAG : 0) | (p.ahead ? SK_AHEAD : 0) | (p.ang ? SK_ANG : 0) | (p.ef ? SK_EF : 0) |
         (p.grp ? SK_GRP : 0) | (lazy_v ? SK_LAZYV : 0) | (p.wall ? SK_WALL : 0) | (p.soft ? SK_SOFT : 0) | (p.ext ? SK_EXT : 0) |
         (p.indent ? SK_INDENT : 0);
}

// The instantiations of k_step that exist, by key (what plan_step plans with; k_step asserts it of its own KEY):
// 24 + 24 + 24 + 24 + 4 + 1 + 8 + 4 + 16 + 48 = 177.  To exist is to be compiled and to be held by the launcher's table; it is
// NOT to be launched: Engine::iterate asks for a plan with next = false on a thermo step only, so 84 of the 177 are never the
// answer to a request of the engine ("Launch census"; the launches of a handle are counted by key,
// tests/test_step_census_cpu.py holds the set that can be launched)
constexpr bool step_variant_exists(int key) {
  if (key < 0 || key >= STEP_KEY_SPACE) return false;
  const auto on = [key](int bits) { return (key & bits) != 0; };      // one of `bits` is set
  const bool one_lane = !on(SK_LPB4), plain_shape = one_lane || on(SK_AHEAD);   // plain shapes: four lanes ahead, one lane ahead, one lane
  if (on(SK_INDENT)) return on(SK_WALL) && on(SK_PAIR) && !on(SK_DIAG | SK_ANG | SK_EF | SK_GRP | SK_LAZYV | SK_SOFT | SK_EXT) && plain_shape;   // fix indent inside the wall variant: L, N, I x three shapes = 24
  if (on(SK_EXT)) return on(SK_PAIR) && !on(SK_DIAG | SK_ANG | SK_EF | SK_GRP | SK_LAZYV | SK_WALL | SK_SOFT) && plain_shape;   // spring/self, addforce, setforce inside the step: L, N, I x three shapes = 24
  if (on(SK_SOFT)) return on(SK_PAIR) && !on(SK_DIAG | SK_ANG | SK_EF | SK_GRP | SK_LAZYV | SK_WALL) && plain_shape;   // pair_style soft inside the step: L, N, I x three shapes = 24
  if (on(SK_WALL)) return on(SK_PAIR) && !on(SK_DIAG | SK_ANG | SK_EF | SK_GRP | SK_LAZYV) && plain_shape;   // fix wall/region inside the step: L, N, I x three shapes = 24
  if (on(SK_LAZYV)) return on(SK_NEXT) && on(SK_PAIR) && one_lane && !on(SK_DIAG | SK_AHEAD | SK_ANG | SK_EF | SK_GRP);   // velocities handed over after a rebuild: L, I = 4
  if (on(SK_DIAG)) return on(SK_LANGEVIN) && on(SK_NEXT) && on(SK_IDENT) && on(SK_PAIR) && one_lane && !on(SK_AHEAD | SK_ANG | SK_EF | SK_GRP);   // the diagnostic launch: 1
  if (on(SK_GRP)) return !on(SK_IDENT) && on(SK_PAIR) && one_lane && !on(SK_AHEAD | SK_EF);   // fixes on groups, with or without angles: L, N, ANG = 8
  if (on(SK_EF)) return !on(SK_NEXT) && on(SK_PAIR) && one_lane && !on(SK_AHEAD | SK_ANG);    // thermo step in one pass: L, I = 4
  if (on(SK_ANG)) return on(SK_PAIR) && one_lane;                                             // angles inside the step: L, N, I, AHEAD = 16
  return plain_shape;                                                                         // L, N, I, P x three shapes = 48
}
// how many exist among the keys with none of `without` set.  153 without fix indent's bit (which is a flag of its own so that a
// wall variant without indenters is the code it was), 177 in all: the test hooks report both
constexpr int count_step_variants(int without = 0) {
  int c = 0;
  for (int key = 0; key < STEP_KEY_SPACE; key++) c += !(key & without) && step_variant_exists(key);
  return c;
}
static_assert(count_step_variants(SK_INDENT) == 153 && count_step_variants() == 177, "the set of k_step instantiations changed");
// The census key of k_force<E, P, NOBOND, SOFT> (launch_force, DeviceState::force_census): E 0, P 1, NOBOND 2, SOFT 3.  Pairs only and pair_style soft need the
// pair part: 8 + 2 = 10 instantiations
constexpr int FORCE_KEY_BITS = 4, FORCE_KEY_SPACE = 1 << FORCE_KEY_BITS;
constexpr bool force_variant_exists(bool E, bool P, bool NOBOND, bool SOFT) { return (void)E, (P || !NOBOND) && (P || !SOFT); }
constexpr int force_variant_key(bool E, bool P, bool NOBOND, bool SOFT) { return (int)E | (int)P << 1 | (int)NOBOND << 2 | (int)SOFT << 3; }
constexpr bool force_key_exists(int key) {
  return key >= 0 && key < FORCE_KEY_SPACE && force_variant_exists(key & 1, key & 2, key & 4, key & 8);
}

// The launch of this plan takes the velocities a rebuild left in the old order (DeviceState::v_pending): the throughput shape
// of the kernel, in one launch over every bead of one GPU, with no diagnostic launch in front of it.  Engine::iterate asks
// before it lets a rebuild leave them, launch_step when it picks the instantiation.
inline bool takes_pending_v(const StepPlan &p, bool decomposed) {
  return p.fused && step_variant_exists(step_plan_key(p, true)) && p.which < 0 && !p.diag_bits && !decomposed;
}

}  // namespace lmp_le
