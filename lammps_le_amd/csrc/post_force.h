// post_force.h — the fixes that act on the forces between the force computation and the final half-kick (fix wall/region, fix
// indent, fix spring/self | addforce | setforce): the tables the kernels read of them, and PostForce, the one owner of which of
// them act in a run, in what order, and on which side of fix langevin.  "Phase" means one thing throughout: 0 = the fix is defined
// ahead of fix langevin (or there is none), 1 = behind it.  The reference runs the post_force hooks in fix order
// (src/modify.cpp:463-466); the kernels run, within a phase, the walls, then the indenters, then the force fixes in fix order.
#pragma once
#include <memory>
#include <vector>

namespace lmp_le {

constexpr int FORCEOP_MAX = 8;    // fix spring/self | addforce | setforce instances one run can hold (ForceOpTable)
constexpr int WALL_MAX = 4;        // fix wall/region instances one run can hold (WallTable)
constexpr int INDENT_MAX = 4;      // fix indent instances one run can hold (IndentTable)

// fix wall/region (src/fix_wall_region.cpp): what the kernels need of every wall, built on the host at every `run`
enum WallStyle { WALL_LJ93 = 0, WALL_LJ126 = 1, WALL_LJ1043 = 2, WALL_HARMONIC = 3, WALL_MORSE = 4 };
enum WallRegionKind { WALL_BLOCK = 0, WALL_SPHERE = 1, WALL_CYLINDER = 2 };
struct WallEntry {
  int kind, interior, axis;   // region: WallRegionKind, side in (1) | out (0), the cylinder's axis (0 x, 1 y, 2 z)
  int style;                  // WallStyle
  int groupbit;               // the fix's group (1 = all)
  int after_langevin;         // the phase: the fix is defined behind fix langevin, its force is added after drag and noise
  double p[6];                // the region's parameters, as Engine::Region::p
  double coeff[8];            // coeff1 .. coeff7 of FixWallRegion::init at [1] .. [7]
  double offset, cutoff;
  double epsilon, sigma, alpha;   // harmonic: epsilon; morse: D0 (epsilon), r0 (sigma), alpha
};
struct WallTable {
  int n;
  WallEntry w[WALL_MAX];
};

// fix indent (src/fix_indent.cpp): what the kernels need of every indenter.  Filled on the host for every force evaluation - the
// geometry may be a formula of the step - and handed to the kernels by value, so a moving indenter costs no copy and no wait
enum IndentKind { INDENT_SPHERE = 0, INDENT_CYLINDER = 1, INDENT_PLANE = 2 };
struct IndentEntry {
  int kind;                   // IndentKind
  int axis;                   // cylinder: its axis; plane: its normal (0 x, 1 y, 2 z)
  int side;                   // sphere | cylinder: side in (1) | out (0); plane: planeside, lo (-1) | hi (+1)
  int groupbit;               // the fix's group (1 = all)
  int phase;                  // 0: before fix langevin or without one, 1: behind it
  int pad;
  double k, k3;               // K and K / 3
  double ctr[3];              // sphere | cylinder: the centre, remapped into the box as Domain::remap does
  double r;                   // sphere | cylinder: the radius; plane: its position
};
struct IndentTable {
  int n;
  int pad;
  IndentEntry e[INDENT_MAX];
};
constexpr int INDENT_COLS = 4;     // sums per entry: energy, force on the indenter x y z

// fix spring/self | addforce | setforce (src/fix_spring_self.cpp, fix_addforce.cpp, fix_setforce.cpp): the post-force fixes that
// act on chosen beads from outside, in the order the fixes were defined; built on the host at every `run`
enum ForceOpKind { FORCEOP_SPRING = 0, FORCEOP_ADD = 1, FORCEOP_SET = 2 };
struct ForceOpEntry {
  int kind;                   // ForceOpKind
  int groupbit;               // the fix's group (1 = all)
  int phase;                  // 0: before fix langevin or without one, 1: behind it
  int every;                  // addforce `every N`: acts on steps with ntimestep % N == 0 (the host states it per launch)
  int mask;                   // bit c: spring/self has a spring along c | setforce sets component c (addforce: 7)
  int pad;
  double k;                   // spring/self: the spring constant
  double v[3];                // addforce | setforce: the three values
  const double *origin;       // spring/self: [3][stride] unwrapped origins by tag, device memory (members only are read)
};
struct ForceOpTable {
  int n;
  int stride;                 // natoms + 1: the row length of every origin block
  ForceOpEntry e[FORCEOP_MAX];
};
constexpr int FORCEOP_COLS = 10;   // sums per entry: energy, foriginal x y z, virial xx yy zz xy xz yz

struct DeviceState;
struct Fix;
struct FixWallRegion;
struct FixIndent;
struct FixForceOp;

// The post-force fixes of one run.  Host only: build() needs no device, and what it refuses is refused before any device work.
struct PostForce {
  // the tables of this run and the fixes behind their rows, each in fix order
  WallTable walltab{};
  std::vector<FixWallRegion *> wall_fixes;
  std::vector<FixIndent *> indent_fixes;
  std::vector<int> indent_phase;
  IndentTable indent_now{};           // the indenters' geometry of the force evaluation under way
  ForceOpTable forceoptab{};
  std::vector<FixForceOp *> forceop_fixes;
  bool behind = false, walls_grouped = false, indents_grouped = false;   // some fix acts in phase 1; some wall | indenter on a group

  // The one walk over the fixes, at every `run` and `minimize` behind Engine::init(): the phase flips at fix langevin, every wall,
  // indenter and force fix joins its table with the phase it was met in.  An addforce or setforce ahead of a wall or an indenter on
  // its side of fix langevin would see the wrong force (the kernels run those first): refused.  spring/self may stand anywhere.
  void build(const std::vector<std::unique_ptr<Fix>> &fixes, int natoms);
  void clear() { *this = PostForce(); }      // the set of fixes changed: the next run builds again
  // the tables on the device: the wall table (with n = 0 for a run with indenters alone - the wall variant of the step kernel
  // reads it whenever it runs), the indenters' rows of block sums, the force fixes' table with the tethers' origins
  void upload(DeviceState &d);
  // k_wall, k_indent, k_fixforce for the fixes of one phase, in that order; the geometry of step `step` is evaluated at phase 0
  void run(DeviceState &d, long step, int phase, bool eflag);
  IndentTable indent_table() const;   // the geometry as the formulas stand: evaluated on the host, centres remapped

  bool any() const { return walltab.n || forceoptab.n || !indent_fixes.empty(); }
  bool behind_langevin() const { return behind; }        // then: no fused final half-kick in fix langevin's kernel
  static int request(size_t n, bool grouped) { return !n ? 0 : grouped ? 2 : 1; }   // 0 none, 1 all on group all, 2 one on a group
  int walls_request() const { return request(wall_fixes.size(), walls_grouped); }           // StepRequest::walls
  int indents_request() const { return request(indent_fixes.size(), indents_grouped); }     // StepRequest::indents
  bool ext() const { return forceoptab.n > 0; }          // StepRequest::ext
  unsigned forceop_active(long step) const;              // bit k: entry k acts on `step` (addforce `every`)
  // An addforce with `every N` reports, on a thermo step it skips, the sums of the last step on which it acted: that step takes
  // the unfused kernels with the block sums, like a thermo step.  True when `step` is such a step: an entry with N > 1 acts now
  // and the next thermo step (a multiple of `thermo`, or the end of the run) comes before it acts again
  bool forceop_sums_due(long step, long endstep, int thermo_every) const;

  // The sums of a thermo evaluation: the sixteen of the force kernel, then rows of 16 per wall, per force fix and per indenter
  static constexpr int SUMS_MAX = 16 + 16 * (WALL_MAX + FORCEOP_MAX + INDENT_MAX);
  int sum_rows() const { return walltab.n + forceoptab.n + (int)indent_fixes.size(); }
  void reduce(DeviceState &d, double *s) const;          // the rows behind s[16], each family's in one pass and one wait
  // the rows into the fixes that report them; adds what fix_modify energy / virial put into pe and the pressure
  void take_sums(const double *s, long step, double &efix, double vfix[6]);
  // the minimiser's record behind its force (and angle) sums - enqueue_thermo_sums: the walls' and force fixes' rows, then
  // INDENT_COLS per indenter - into the rows behind s[16]
  void unpack_min_record(const double *p, double *s) const;
};

}  // namespace lmp_le
