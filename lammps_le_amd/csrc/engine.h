// engine.h — MI355X-native bead-spring MD engine behind the reference's script / C-library boundary.
//
// Host side (C++17) mirrors the reference objects that the hot path talks to
// (/root/reference/src: input.cpp, read_data.cpp, modify.cpp, verlet.cpp, neighbor.cpp,
// pair_lj_cut.cpp, MOLECULE/bond_fene.cpp, fix_nve.cpp, fix_langevin.cpp, USER-LE/fix_*.cpp);
// all per-atom work runs as hand-written HIP kernels for gfx950 (kernels_*.hip).
#pragma once
#include <cstdint>
#include <cstdio>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "step_plan.h"
#include "rebuild_plan.h"
#include "post_force.h"

namespace lmp_le {

struct LammpsError : std::runtime_error {
  using std::runtime_error::runtime_error;
};

constexpr int MAXTYPES = 16;       // atom types and bond types handled by the by-value kernel tables
constexpr int MAXBPA = 8;          // bonds per atom the bond-partner table can hold
constexpr int MS_MAX = 32;         // max special neighbors per atom handled by the device rebuild
constexpr int NEIGH_SB_SHIFT = 30; // special-bond bits, as src/lmptype.h:61-62
constexpr int NEIGH_MASK = 0x3FFFFFFF;
constexpr int BOND_TYPE_SHIFT = 26; // bond partner table: (type << 26) | partner index
constexpr int BOND_IDX_MASK = (1 << BOND_TYPE_SHIFT) - 1;
// numneigh word of a bead: list entries in the low 16 bits (bonds + pairs), of which the first (word >> 16) are bond
// entries in the bond-partner table's encoding (kernels_md.hip pair_loop)
constexpr int NN_BOND_SHIFT = 16;
constexpr int NN_COUNT_MASK = (1 << NN_BOND_SHIFT) - 1;
constexpr int NN_NBOND_MASK = 0xFF;          // bond entries of the word: (word >> NN_BOND_SHIFT) & NN_NBOND_MASK
// bit 30 of the word: some bond of this bead reaches its partner through a periodic image.  The image of a bond partner is
// FROZEN at the reneighbor (src/ntopo_bond_all.cpp:52-73: domain->closest_image picks a ghost, whose shift then stays),
// two bits per dimension and bond slot in DeviceState::bshift (0 none, 1 partner at +prd, 2 partner at -prd)
constexpr int NN_SHIFTED_BIT = 1 << 30;
constexpr int BSHIFT_BITS = 6;
// ---------------------------------------------------------------------------------------------
// RanMars in exact integer arithmetic (src/random_mars.cpp:29-95; every value is k * 2^-24)
// ---------------------------------------------------------------------------------------------
struct RanMarsInt {
  // history window w[k] = y_{n-97+k}, k = 0..96, of the lagged-Fibonacci part
  //   y_n = y_{n-97} - y_{n-33}  (mod 2^24),  y_{-k} = u[k] of the reference's seed table
  uint32_t w[97];
  uint64_t n;  // raw index of the NEXT value to generate (the constructor's warm-up draw was n = 0)
  void seed(int seed);
  uint32_t next_raw();  // 24-bit integer of the next uniform(): uniform = value / 2^24
  double uniform() { return next_raw() * (1.0 / 16777216.0); }
  static uint32_t c_of(uint64_t n);  // arithmetic-sequence term used for raw index n
  void jump(uint64_t k);             // advance by k draws in O(97^2 log k)
};
// coefficients a[0..96] of x^k mod (x^97 + x^64 - 1) over Z/2^24: y_{n+k} = sum_j a[j] y_{n+j}
void ranmars_jump_poly(uint64_t k, uint32_t a[97]);

// ---------------------------------------------------------------------------------------------
// device-side views (plain pointers; filled by Engine, consumed by the kernel launchers)
// ---------------------------------------------------------------------------------------------
struct Box {
  double lo[3], hi[3], prd[3], half[3], iprd[3];
};

struct TypeTables {  // by-value kernel argument
  double dtfm[MAXTYPES + 1];   // dtf / mass[type]           (src/fix_nve.cpp:95)
  double g1[MAXTYPES + 1];     // gfactor1[type]             (src/fix_langevin.cpp:296-310)
  double g2[MAXTYPES + 1];     // gfactor2[type] * tsqrt     (src/fix_langevin.cpp:663)
  double mass[MAXTYPES + 1];
};

struct PairTable {  // lj/cut per type pair, row-major (ntypes+1)^2; lives in device memory
  int nt;           // ntypes + 1
  double special_lj[4];
};

struct BondTable {  // by-value kernel argument
  int style[MAXTYPES + 1];  // 0 none/zero, 1 fene, 2 harmonic, 3 morse (unfused force kernel only)
  double p0[MAXTYPES + 1], p1[MAXTYPES + 1], p2[MAXTYPES + 1], p3[MAXTYPES + 1];
};

struct AngleTable {  // by-value kernel argument: angle_style harmonic | cosine (src/MOLECULE/angle_harmonic.cpp, angle_cosine.cpp)
  int style[MAXTYPES + 1];     // 0 none/zero, 1 harmonic, 2 cosine
  double k[MAXTYPES + 1], theta0[MAXTYPES + 1];   // theta0 in radians
};

struct DeviceState;  // defined in device.h (HIP side)
struct Comm;         // defined in comm.h

// ---------------------------------------------------------------------------------------------
// fixes (style registry mirrors src/modify.cpp:93-99 / style names of the reference)
// ---------------------------------------------------------------------------------------------
class Engine;

struct Fix {
  std::string id, group, style;
  int groupbit = 1;          // bit of the fix's group in Engine::gmask (1 = all)
  Engine *eng = nullptr;
  bool force_reneighbor = false;
  virtual ~Fix() {}
  virtual void init() {}
  virtual void setup() {}
  // which hooks this fix has (src/fix.h:247-273 mask bits)
  bool has_initial_integrate = false, has_post_integrate = false, has_post_force = false,
       has_final_integrate = false;
  // POST_INTEGRATE_RESPA: set by ex_load / ex_unload and their src/MC parents; fix extrusion's setmask() leaves it out
  // (fix_extrusion.cpp:166-171), so under run_style respa the reference never calls it - and neither does respa_recurse
  bool has_post_integrate_respa = true;
  virtual void initial_integrate() {}
  virtual void post_integrate() {}
  virtual void post_force() {}
  virtual void final_integrate() {}
  virtual double compute_vector(int) { throw LammpsError("Fix does not compute a vector"); }
  virtual double compute_scalar() { return compute_vector(0); }     // `f_ID` without an index
  virtual int size_vector() const { return -1; }                     // length of the global vector (-1: not checked)
  virtual bool extensive() const { return false; }                   // extscalar / extvector: thermo divides by the atom count under `norm yes`
};

struct FixNVE : Fix {
  FixNVE(Engine *e, const std::vector<std::string> &arg);
};

struct FixLangevin : Fix {
  double t_start, t_stop, t_period;
  int seed;
  RanMarsInt rng;          // host mirror of the stream position (kept in sync by draw counting)
  uint64_t draws = 0;      // Langevin draws consumed so far (3 per atom per post_force call)
  bool dev_ready = false;  // device block states initialised
  std::vector<double> ratio;   // keyword `scale itype ratio`: per-type divisor of the damping time (src/fix_langevin.cpp:135-141)
  bool zeroflag = false;       // keyword `zero yes`: the mean random force of the group is taken off every member (:752-772)
  FixLangevin(Engine *e, const std::vector<std::string> &arg);
};

struct FixExtrusion : Fix {
  int nevery, neutral, ctcf_left, ctcf_right, ctcf_lr, btype;
  double through_prob;
  RanMarsInt rng;
  bool rng_on_device = false;
  int last_break = 0;
  FixExtrusion(Engine *e, const std::vector<std::string> &arg);
  void post_integrate() override;
  double compute_vector(int n) override;
};

struct FixExLoad : Fix {    // also the stock `bond/create` (src/MC/fix_bond_create.cpp), the style ex_load was derived from
  int nevery, iatomtype, jatomtype, btype, imaxbond = 0, inewtype, jmaxbond = 0, jnewtype;
  int atype = 0;             // `atype N`: angles of type N around every new bond, if an angle style is defined (fix_ex_load.cpp:236-254, :855-954)
  bool stock = false;        // bond/create: candidates = every pair of the pair list (not only (i, i+2)), fires at step % N == 0,
  int phase = 3;             //   bonds of btype per bead counted at the first setup and from then on only incremented
  std::vector<int> bondcount;   // [natoms + 2] by tag (stock only)
  bool counted = false;
  double cutsq, fraction = 1.0;
  int seed = 12345;
  RanMarsInt rng;
  bool rng_on_device = false;
  int last_create = 0;
  long total_create = 0;
  FixExLoad(Engine *e, const std::vector<std::string> &arg);
  void init() override;
  void setup() override;
  void post_integrate() override;
  double compute_vector(int n) override;
};

struct FixExUnload : Fix {   // also the stock `bond/break` (src/MC/fix_bond_break.cpp), which differs only in the firing step
  int nevery, btype;
  int angleflag = 0;         // set in init(): the system has angles, broken bonds take theirs along (fix_ex_unload.cpp:149-152)
  void init() override;
  int phase = 2;             // fires when ntimestep % nevery == phase: 2 for ex_unload, 0 for bond/break
  double cutsq, fraction = 1.0;
  int seed = 12345;
  RanMarsInt rng;
  bool rng_on_device = false;
  int last_break = 0;
  long total_break = 0;
  FixExUnload(Engine *e, const std::vector<std::string> &arg);
  void post_integrate() override;
  double compute_vector(int n) override;
};

// fix ID group wall/region region-ID style args cutoff (src/fix_wall_region.cpp).  The force lives in kernels_md.hip
// (wall_force); this object holds the script's numbers and the sums of the last evaluation
struct FixWallRegion : Fix {
  std::string idregion;
  int wstyle = WALL_LJ126;
  double epsilon = 0.0, sigma = 0.0, alpha = 0.0, cutoff = 0.0;
  bool thermo_energy = false, thermo_virial = false;     // fix_modify energy / virial (src/fix.cpp:63-64: both off)
  double ewall[4] = {0, 0, 0, 0};                        // energy and the force on the wall, of the last thermo evaluation
  double virial[6] = {0, 0, 0, 0, 0, 0};                 // xx yy zz xy xz yz
  FixWallRegion(Engine *e, const std::vector<std::string> &arg);
  void init() override;                                  // the region may have been deleted since the command
  WallEntry entry() const;                               // coefficients by the expressions of FixWallRegion::init
  double compute_scalar() override { return ewall[0]; }
  double compute_vector(int n) override { return ewall[n + 1]; }
  int size_vector() const override { return 3; }
  bool extensive() const override { return true; }       // (src/fix_wall_region.cpp:45-46)
};

// fix ID group indent K <sphere x y z R | cylinder dim c1 c2 R | plane dim pos lo|hi> [side in|out] [units box|lattice]
// (src/fix_indent.cpp).  The force lives in indent_inl.h (indent_force); this object holds the script's numbers and variable
// names and the sums of the last evaluation with sums
struct FixIndent : Fix {
  int istyle = INDENT_SPHERE, cdim = 0, side = 0, planeside = 0;
  double k = 0.0, k3 = 0.0;
  double value[5] = {0, 0, 0, 0, 0};                     // x y z R pos as numbers
  std::string vstr[5];                                   // ... or as the name of an equal-style variable ("": a number)
  bool thermo_energy = false;                            // fix_modify energy (THERMO_ENERGY; the fix has no virial)
  double indenter[4] = {0, 0, 0, 0};                     // energy and the force on the indenter
  FixIndent(Engine *e, const std::vector<std::string> &arg);
  void init() override;                                  // FixIndent::init: the variables exist and are equal-style, host-evaluable
  bool varflag() const { for (auto &v : vstr) if (!v.empty()) return true; return false; }
  IndentEntry entry();                                   // the geometry of step Engine::ntimestep (FixIndent::post_force's head)
  double compute_scalar() override { return indenter[0]; }
  double compute_vector(int n) override { return indenter[n + 1]; }
  int size_vector() const override { return 3; }
  bool extensive() const override { return true; }       // (src/fix_indent.cpp:51-52)
};

// fix ID group spring/self K [dir] | addforce fx fy fz [every N] | setforce fx|NULL fy|NULL fz|NULL.  The force lives in
// kernels_md.hip (forceops_on_bead); the objects hold the script's numbers, the origins and the sums of the last evaluation
struct FixForceOp : Fix {
  int kind = FORCEOP_SPRING;
  int every = 1, mask = 7;
  double k = 0.0, v[3] = {0, 0, 0};
  bool has_energy = false, has_virial = false;           // what fix_modify energy / virial may switch on for this style
  bool thermo_energy = false, thermo_virial = false;
  std::string estr;                                      // addforce `energy v_name`: refused at run, as the reference's init()
  std::vector<double> xorig;                             // spring/self: [natoms][3] unwrapped origins by tag - 1 (non-members 0)
  double sums[FORCEOP_COLS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // of the last thermo evaluation on which the fix acted
  void init() override;
  ForceOpEntry entry() const;
  int size_vector() const override { return kind == FORCEOP_SPRING ? 0 : 3; }
  bool extensive() const override { return true; }       // extscalar / extvector = 1 in all three
  double compute_scalar() override;
  double compute_vector(int n) override;
};
struct FixSpringSelf : FixForceOp { FixSpringSelf(Engine *e, const std::vector<std::string> &arg); };
struct FixAddForce : FixForceOp { FixAddForce(Engine *e, const std::vector<std::string> &arg); };
struct FixSetForce : FixForceOp { FixSetForce(Engine *e, const std::vector<std::string> &arg); };

// fix ID group adapt N pair soft a | lj/cut epsilon | lj/cut sigma I J v_name [pair ...] [reset yes|no] [scale yes|no]
// (src/fix_adapt.cpp).  Holds the script's words; the values are set by Engine::adapt_apply at setup of every run and before the
// force evaluation of every step with step % N == 0, and travel to the device as Engine::push_pair_table describes
struct FixAdapt : Fix {
  struct Clause {
    std::string pstyle, pparam, var;
    int ilo, ihi, jlo, jhi;
    std::vector<double> orig;        // [(ntypes+1)^2] the parameter as FixAdapt::init found it (array_orig)
  };
  int nevery = 0;
  bool resetflag = false, scaleflag = false;
  std::vector<Clause> clauses;
  FixAdapt(Engine *e, const std::vector<std::string> &arg);
  void init() override;              // the checks of FixAdapt::init (:316-491) and the copy of the original values
  std::vector<double> *target(const Clause &c) const;   // the array of Engine the clause sets (pc_eps | pc_sig)
};

// ---------------------------------------------------------------------------------------------
// Engine = the LAMMPS instance behind one C-API handle
// ---------------------------------------------------------------------------------------------
struct ThermoRow {
  long step;
  double temp, epair, emol, etotal, press, ke, pe;
  double evdwl, ebond, virial[6];      // (sums over the system; ebond = bonds only)
  long nbonds;
  double eangle = 0.0;                 // sum over the listed angles
  double ptensor[6] = {0, 0, 0, 0, 0, 0};   // pxx pyy pzz pxy pxz pyz (src/compute_pressure.cpp:244-290), when asked for
  bool has_ptensor = false;
  double fmax = 0.0, fnorm = 0.0;      // max |f_ic| and sqrt(f.f) (src/thermo.cpp compute_fmax / compute_fnorm), when asked for
};

class Engine {
 public:
  Engine(int argc, char **argv);
  ~Engine();

  // ---- script layer (src/input.cpp:181 file, :327 one, :689 execute_command) ----
  void file(const std::string &path);
  const char *one(const std::string &line);  // returns the command name (borrowed), like Input::one
  void execute(const std::string &cmd, std::vector<std::string> &arg);

  // ---- global state ----
  std::string units = "lj", atom_style = "atomic";
  double boltz = 1, mvv2e = 1, ftm2v = 1, nktv2p = 1, mv2d = 1, dt = 0.005;
  double skin = 0.3;
  int neigh_every = 1, neigh_delay = 10, neigh_check = 1;
  bool newton_pair = true, newton_bond = true;
  int sortfreq = 1000;
  long nextsort = 0;
  double special_lj[4] = {1.0, 0.0, 0.0, 0.0};
  double special_coul[4] = {1.0, 0.0, 0.0, 0.0};   // no Coulomb on this path, but the pair list's special flags depend on it
  // how the pair list treats a special level (src/neighbor.cpp:360-376 special_flag, src/npair.h:112-136 find_special):
  // 0 = pair dropped from the list (lj and coul weight both 0), 1 = stored as an ordinary entry, 2 = stored with the level
  // in its top bits.  The reference also takes 2 when lj == 1 but coul != 1; the factor such an entry carries is 1.0,
  // so it is stored as an ordinary entry here (same list membership, same forces).
  int special_flag(int level) const {
    if (special_lj[level] == 0.0 && special_coul[level] == 0.0) return 0;
    if (special_lj[level] == 1.0) return 1;
    return 2;
  }
  double comm_cutoff = 0.0;
  long ntimestep = 0, beginstep = 0, endstep = 0;
  int thermo_every = 0;
  bool thermo_norm = true;
  std::vector<std::string> thermo_keywords;
  bool box_exist = false;
  Box box{};

  // ---- atoms: host master copies in TAG order (tag t at index t-1) ----
  int natoms = 0, ntypes = 0, nbondtypes = 0;
  int extra_bond = 0, extra_special = 0, bpa = 0, maxspecial = 0;
  long nbonds = 0;
  std::vector<double> mass;                        // [ntypes+1]
  std::vector<int> mass_set;
  std::vector<double> x, v, f;                     // [natoms*3]
  std::vector<int> type, image, molecule;          // image: 3 ints per atom
  std::vector<int> num_bond, bond_type, bond_atom; // [natoms], [natoms*bpa]
  std::vector<int> nspecial, special;              // [natoms*3], [natoms*maxspecial]
  // angles: stored with all three atoms (newton_bond off, src/atom.cpp:1290-1353), atoms as IDs
  int nangletypes = 0, extra_angle = 0, apa = 0;   // apa = angles per atom (0: the system has no angle storage)
  long nangles = 0;
  std::vector<int> num_angle, angle_type, angle_a1, angle_a2, angle_a3;   // [natoms], [natoms*apa]
  std::string angle_style_name;                    // "", "harmonic", "cosine", "zero", "none"
  AngleTable angtab{};
  bool angles_active() const;                      // an angle style with coefficients and angle storage exist
  std::vector<int> crank;                          // canonical (reference local) index of tag t-1
  // the reference's local index of a bead is its ID - 1: true while no Atom::sort ran and the data file listed the atoms
  // in ID order.  Then the order-sensitive kernels index by tag directly instead of through crank[].
  bool local_order_is_tag_order() const;
  bool crank_on_device = false;                    // the device's crank[] is newer than this copy (Atom::sort emulation)
  bool special_built = false;
  bool host_current = true;    // host x/v/f/type/topology reflect the device state
  bool dev_current = false;    // device state reflects the host copies

  // ---- styles ----
  bool pair_lj = false, pair_zero = false;
  // pair_style soft (src/pair_soft.cpp): A lives in pc_eps, rc in pc_cut; the derived columns lj1 lj2 lj3 then hold A pi/rc, pi/rc
  // and A (soft_inl.h), lj4 and offset stay 0
  bool pair_soft = false;
  bool pair_force() const { return pair_lj || pair_soft; }       // a pair style that computes something
  const char *pair_style_name() const { return pair_lj ? "lj/cut" : pair_soft ? "soft" : pair_zero ? "zero" : "none"; }
  void init_pair_coeffs();          // Pair::init / Pair::reinit: every type pair's derived coefficients, mixing included
  // the table and the scalars of the force kernels from the derived coefficients.  The scalars are refreshed; the table is
  // copied on the run's stream from a ring of pinned rows that stay untouched until the copy has run - except `mid_run` (fix
  // adapt between two launches) when the force kernels read the scalars alone: then the copy is left out and pair_table_stale
  // says so, until someone who reads the table (Engine::pair_rows) or the end of the run asks for it
  void push_pair_table(bool mid_run);
  bool pair_table_stale = false;
  long pair_table_copies = 0;       // mid-run copies of the pair table by fix adapt (lammps_le_stat "pair_table_copies")
  std::string pair_sig;             // pair style and neighbor cutoff of the last upload
  bool in_run = false;              // Update::whichflag != 0: ramp() is legal
  std::string host_only_for;        // != "": a formula evaluated for this variable of a fix must not read the device
  std::string host_only_style = "adapt";   // ... the style of that fix (adapt | indent), for the message (HostOnlyScope sets both)
  void adapt_apply(bool setup);     // FixAdapt::setup_pre_force / pre_force of every fix adapt, then Pair::reinit + push
  void adapt_post_run();            // FixAdapt::post_run: reset yes
  bool adapt_set_values(bool setup);   // the host part of adapt_apply: true when a coefficient was set (and all derived again)
  bool adapt_restore_values();         // ... of adapt_post_run
  bool have_adapt() const;
  double pair_cut_global = 0.0;
  bool pair_shift = false;
  int pair_mix = 0;  // 0 geometric, 1 arithmetic
  std::vector<double> pc_eps, pc_sig, pc_cut;
  std::vector<int> pc_set;
  std::vector<double> lj1, lj2, lj3, lj4, offset, cutsq;
  double cutforcemax = 0.0, cutneighmax = 0.0;
  std::string bond_style_name;                    // "", "fene", "harmonic", "hybrid", "zero"
  std::vector<std::string> bond_hybrid_styles;
  BondTable bondtab{};

  std::vector<std::unique_ptr<Fix>> fixes;
  Fix *find_fix(const std::string &id);

  // ---- run control (src/run.cpp:38-188, src/verlet.cpp) ----
  void run(long nsteps);
  void init();          // lmp->init(): pair coefficients, neighbor cutoffs, fix init, special lists
  void setup();         // Verlet::setup
  void iterate(long n); // Verlet::run
  // run_style respa N loop_1 .. loop_{N-1} [bond L] [pair L] (src/respa.cpp); respa_levels = 0: run_style verlet.  A slow
  // path of unfused kernels (round 3: also decomposed): what the LE fixes' post_integrate_respa hooks need
  int respa_levels = 0, respa_loop[8] = {1, 1, 1, 1, 1, 1, 1, 1}, respa_level_bond = 0, respa_level_pair = 0, respa_level_angle = 0;
  double respa_step[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  void respa_setup();                          // Respa::setup
  void respa_iterate(long n);                  // Respa::run
  void respa_recurse(int ilevel, bool last);   // Respa::recurse
  void respa_level_forces(int ilevel);
  void compute_forces(bool eflag);
  ThermoRow eval_thermo(bool ke_summed = false);
  // the row from the sums of one evaluation: s = the sixteen of the force kernel, then rows of 16 per wall, per force fix and per indenter;
  // a8 = the angles' (null: none), k6 = the kinetic tensor (null: not asked for)
  ThermoRow thermo_from_sums(const double *s, const double *a8, const double *k6);
  std::string thermo_float_format;     // thermo_modify format float: a checked printf conversion ("": %12.8g)
  bool want_fnorm = false;            // fmax or fnorm was named: thermo steps also reduce the force norms
  void print_thermo_header();
  // what `run` and `minimize` do between init() and their setup: the tables of the post-force fixes (first: what they refuse
  // needs no device), upload or refresh of the device state, the modes of this run
  void begin_run_state();
  // ---- minimize (minimize.cpp; src/minimize.cpp, min.cpp, min_linesearch.cpp, min_cg.cpp, min_sd.cpp) ----
  std::string min_style = "cg";        // (src/update.cpp:60-62: cg without the command)
  double min_dmax = 0.1;               // min_modify (src/min.cpp:50-80 defaults)
  int min_linestyle = 1;               // 0 backtrack, 1 quadratic
  int min_normstyle = 0;               // 0 two, 1 max, 2 inf
  std::map<std::string, std::string> min_other;   // the keywords of fire / spin: stored, without effect on cg and sd
  void min_style_command(std::vector<std::string> &arg);
  void min_modify_command(std::vector<std::string> &arg);
  void minimize(double etol, double ftol, long maxiter, long maxeval);
  // of the last minimisation (lammps_le_stat min_*): iterations, evaluations, index into the stop strings, the last line
  // search's alpha, host waits, list builds, and the energies of the stats block
  long min_niter = 0, min_neval = 0, min_host_waits = 0, min_rebuilds = 0;
  int min_stop = 0;
  double min_alpha = 0.0, min_einitial = 0.0, min_eprevious = 0.0, min_efinal = 0.0;
  double min_fnorm2_init = 0.0, min_fnorminf_init = 0.0, min_fnorm2_final = 0.0, min_fnorminf_final = 0.0;
  static const char *min_stop_string(int n);
  // one thermo keyword (src/thermo.cpp:1572-2110 compute_*): false when the keyword is unknown.  `r` = the row the energies
  // come from; `isint` = printed with the integer format (BIGINT fields)
  bool thermo_keyword(const ThermoRow &r, const std::string &k, double &val, bool &isint);
  bool want_ptensor = false;           // a pressure-tensor keyword was named: thermo steps also reduce the kinetic tensor
  bool thermo_multi = false;           // thermo_style multi (src/thermo.cpp:115-119, 171-180, 361-366)
  bool thermo_first_line = true;       // the first line of a run prints CPU = 0 (Thermo::firststep)
  double run_wall0 = 0.0;              // wall clock at the start of the run's loop (Timer::TOTAL)
  double atime = 0.0;                  // Update::atime / atimestep: simulation time accumulated over runs with changing dt
  long atimestep = 0;
  void print_thermo(const ThermoRow &);
  ThermoRow last_thermo{};
  std::vector<ThermoRow> thermo_log;
  double loop_time = 0.0;
  long neigh_builds = 0, neigh_dangerous = 0;
  long lazy_rebuilds = 0;      // rebuilds of this run that left the velocities to the step kernel (RB_LAZY_V), lammps_le_stat("lazy_rebuilds")
  // time steps of the current run by the path they took (lammps_le_stat "steps_*"): the step kernel - of which its group, wall,
  // soft and EXT (spring/self, addforce, setforce inside the kernel) variants and the launches that carried an indenter -, the
  // step kernel's energy variant on a thermo step, the unfused kernels
  struct StepCounters {
    long fused = 0, fused_group = 0, fused_wall = 0, fused_soft = 0, fused_ext = 0, fused_indent = 0, fused_thermo = 0, unfused = 0;
    void reset() { *this = StepCounters(); }
  } steps;
  // fix wall/region, fix indent, fix spring/self | addforce | setforce: the tables of this run, built by begin_run_state() (post_force.h)
  PostForce postforce;
  // the post-force fixes of phase 0, fix langevin if there is one (`fuse_final`: with the final half-kick in its kernel), the
  // post-force fixes of phase 1 - the order of Modify::post_force, the same for every integrator and the minimiser
  void post_force_sequence(FixLangevin *lg, bool eflag, bool fuse_final);
  StepKnobs step_knobs;        // the step kernel's environment switches as they stood when the current run began
  RebuildKnobs rebuild_knobs;  // ... and the rebuild's
  unsigned rebuild_plan_bits = 0;   // the plan the last rebuild (or regrow pass) executed, lammps_le_stat("rebuild_plan_full")
  long rng_late_count = 0;     // decomposed runs: late generations of skipped Langevin stream segments (lammps_le_stat)
  int ago = 0;
  // Timer sections of the loop (src/timer.h:25-28); wall clock between stamps as src/timer.cpp:100-135.  The GPU runs
  // asynchronously behind the host, so without `timer sync` a section holds the time the HOST spent in it (waits for
  // the device land where the host first needs a result); `timer sync` drains the stream at every stamp.
  enum { T_PAIR = 0, T_BOND, T_NEIGH, T_COMM, T_OUTPUT, T_MODIFY, T_NSECT };
  double timers[8] = {0};
  int timer_level = 2;         // `timer off|loop|normal|full` (src/timer.cpp:230-300): 0 off, 1 loop, 2 normal, 3 full
  bool timer_sync = false;     // `timer sync|nosync`
  double timer_prev = 0.0;
  void stamp();                // Timer::stamp()      : restart the section clock
  void stamp(int which);       // Timer::stamp(which) : add the time since the previous stamp to a section
  void print_timing_breakdown(long nsteps);   // src/finish.cpp:318-370
  std::string census_file;     // LAMMPS_LE_STEP_CENSUS_FILE=path (read once, here): ~Engine appends this handle's launch census to it
  bool kernel_timing = false;  // LAMMPS_LE_KERNEL_TIMING=1: HIP events around sampled step-kernel launches
  double kstat_ms = 0.0;       // mean step-kernel duration of the last run (ms)
  long kstat_n = 0;
  long ktime_counter = 0;      // launches seen by the sampler in this run
  int ktime_every = 16;        // sample every n-th launch (1 for runs of <= 64 steps)
  double stat_neigh_pairs();   // stored full-list entries of the current neighbor list

  // ---- topology on the host (read_data path) ----
  void read_data(const std::string &path);
  void write_data(const std::string &path);
  void velocity(std::vector<std::string> &arg);
  // groups (src/group.cpp): static bit masks by atom; bit 0 = all.  fix nve / fix langevin act on them (unfused kernels)
  std::vector<std::string> group_names = {"all"};
  std::vector<int> gmask;                          // by atom index (ID - 1); empty until a group is defined
  std::string group_sig;                           // group_signature() of the last upload
  std::string group_signature() const;
  int langevin_members = 0;                        // atoms in fix langevin's group (its draws per call / 3); set by upload()
  int group_bit(const std::string &name) const;    // 1 << index, or 0 if there is no such group
  void group_command(std::vector<std::string> &arg);
  // `region ID block | sphere | cylinder | union | intersect ... [side in|out] [units box|lattice]` (src/region*.cpp): static
  // regions, for `group ID region R` and `set region R ...`.  match = !(inside ^ interior), closed boundaries
  struct Region {
    std::string style;
    bool interior = true;
    double p[6] = {0, 0, 0, 0, 0, 0};      // block: xlo xhi ylo yhi zlo zhi; sphere: x y z r; cylinder: c1 c2 r lo hi
    char axis = 'z';
    std::vector<std::string> sub;          // union / intersect
  };
  std::map<std::string, Region> regions;
  void region_command(std::vector<std::string> &arg);
  bool region_match(const Region &r, double x, double y, double z) const;
  void set_command(std::vector<std::string> &arg);   // set atom|type|mol|group ... (src/set.cpp)   // velocity all create|set|scale|zero (src/velocity.cpp)
  // ---- dumps (src/dump_custom.cpp, dump_atom.cpp, dump_local.cpp; compute_property_local.cpp) ----
  struct Dump {
    std::string id, style, path, label = "ENTRIES";
    long every = 0, last = -1;
    int groupbit = 1;              // rows = the members of the dump's group (`mask[i] & groupbit`: src/dump_custom.cpp:607-612,
                                   // dump_atom.cpp:356, dump_dcd.cpp:69,200); dump local takes its rows from the compute's group
    bool unwrap = false;           // dcd: coordinates unwrapped by the image flags (dump_modify unwrap yes)
    int nframes = 0;               // dcd: snapshots written so far (header fields are patched after each one)
    std::vector<std::string> cols;
    FILE *fp = nullptr;
  };
  std::vector<Dump> dumps;
  // what the rows of a local compute are (src/compute_property_local.cpp kindflag): the stored bonds, the pair entries of the
  // neighbor list (natom1 natom2 ntype1 ntype2), or of those the pairs within their cutoff at the current positions (patom1
  // patom2 ptype1 ptype2, and every value of compute pair/local: dist eng force fx fy fz)
  enum { LOCAL_BOND = 0, LOCAL_NEIGH = 1, LOCAL_PAIR = 2 };
  struct LocalCompute {
    std::string style;                 // "property/local" | "pair/local"
    int kind = LOCAL_BOND;             // LOCAL_*: what its rows are
    int bit = 1;                       // group bit: both atoms of a row must be members
    std::vector<std::string> attrs;    // its columns, as named in the command
  };
  std::map<std::string, LocalCompute> computes_local;               // by compute ID
  void compute_command(std::vector<std::string> &arg);
  // the checks of a compute's init(): at every run for every compute, and before a compute defined since answers
  void init_local_compute(const LocalCompute &c) const;
  void init_local_computes() const { for (auto &c : computes_local) init_local_compute(c.second); }
  // Pair rows (kernels_local.hip): one device pass per (kind, group) and state, shared by every compute and dump column that
  // asks for it.  A state is (timestep, thermo rows so far, edits of the device state through the C-ABI subset calls).
  struct PairRows {
    int kind = LOCAL_NEIGH, bit = 1;
    long step = -1, edits = -1;
    size_t stamp = 0;
    long nrows = 0;
    std::vector<int> ids;        // [nrows][4] atom1 atom2 type1 type2, ordered by (atom1, atom2)
    std::vector<double> vals;    // [nrows][6] dist eng force fx fy fz (LOCAL_PAIR)
  };
  std::vector<PairRows> pair_rows_cache;
  const PairRows &pair_rows(const LocalCompute &c);  // collective when decomposed: every rank ends with the whole table
  static int pair_row_column(const std::string &attr);
  static double pair_row_value(const PairRows &r, long row, int column) {
    return column < 4 ? (double)r.ids[4 * (size_t)row + column] : r.vals[6 * (size_t)row + (column - 4)];
  }
  bool pair_list_ready = false;  // the device holds a neighbor list built for the arrays it holds (set by reneighbor, cleared by upload)
  long dev_edits = 0;            // C-ABI subset scatters applied to the device state so far
  long dev_edits_at_run = 0;     // ... as of the end of the last run (decomposed: ghosts are current up to there)
  long group_version = 0, gmask_uploaded_version = -1;   // `group` commands so far; the version DeviceState::gmask holds
  long pair_row_passes = 0, pair_rows_last = 0;          // device passes so far, rows of the last one (lammps_le_stat)
  double pair_rows_ms[2] = {0.0, 0.0};                   // the last pass: count + scan, fill + copy (host wall clock)
  // ---- restart: own binary format, bit-continuous incl. the RNG streams of the fixes ----
  void write_restart(const std::string &path);
  void read_restart(const std::string &path);
  // `restart N root` | `restart N fileA fileB` | `restart 0` (src/output.cpp:603-700 create_restart, :360-420 write_restart)
  long restart_every = 0;
  std::string restart_a, restart_b;
  int restart_toggle = 0;
  void write_periodic_restart(long step);
  std::map<std::string, std::vector<unsigned char>> restart_fix_state;   // fix ID -> saved state, applied by `fix`
  std::map<std::string, std::vector<double>> restart_origins;            // fix ID -> origins of a fix spring/self in the file
  void apply_restart_state(Fix *f);
  bool dump_due(long step) const;
  bool dump_force_all = false;       // the last iteration of a minimisation that stopped early: every dump is due (src/min.cpp:446-449)
  void write_dumps(long step);       // downloads, then writes every dump that is due
  void build_special();               // src/special.cpp:55-
  void create_box_atoms_check();

  // ---- ranks (one process per GPU; world > 1 = z-slab spatial decomposition) ----
  Comm *comm = nullptr;
  int world = 1, rank = 0;
  void comm_init(const std::string &backend, int rank, int world, const void *unique_id, const std::string &session);
  void halo_exchange();
  void halo_exchange_once();          // ... unless this step's ghosts are already current (an LE fix asked first)
  long halo_step = -1;

  // ---- device ----
  DeviceState *dev = nullptr;
  void device_init();                 // throws LammpsError if no HIP device
  void upload();                      // host -> device (after read_data / scatter)
  void download();                    // device -> host (x, v, f, type, image, topology)
  long host_downloads = 0;            // whole-system downloads so far (lammps_le_stat "host_downloads")
  double subset_comm_bytes = 0.0;     // bytes this rank contributed to the collectives of the C-ABI subset calls
  bool timeout_forced = false;        // lammps_force_timeout: runs end at once, as after Timer::force_timeout
  void reneighbor(bool can_defer = false, bool sort_due = false, bool lazy_v = false);   // pbc + spatial sort + cell lists + neighbor list + bond table
  RebuildFacts rebuild_facts(bool can_defer, bool sort_due, bool regrow, bool lazy_v = false) const;   // what plan_rebuild is asked with
  bool reneigh_pending = false;       // the build's overflow / error flags are published but not yet looked at
  bool finish_reneighbor();           // waits for them; false = a list overflowed (nothing may depend on the lists yet)
  void regrow_lists();                // grow the table and rebuild until every list fits
  bool decide();                      // Neighbor::decide (src/neighbor.cpp:1933-1948)
  void emulate_atom_sort();           // keep `crank` equal to the reference's local order (Atom::sort)
  std::vector<long> le_reneigh_step;  // next_reneighbor per fix
  std::string le_style;               // style of the LE fix that fired last (device_error_text)

  // ---- output ----
  FILE *screen = stdout, *logfile = nullptr;
  bool echo_screen = false;
  void say(const std::string &s);
  void warning(const std::string &s);
  std::string last_cmd;
  std::map<std::string, std::string> variables;       // name -> current value (index / loop / string) or formula (equal)
  struct VarInfo { std::string style; std::vector<std::string> values; size_t which = 0; };
  std::map<std::string, VarInfo> var_info;            // style + value list of variables made by the `variable` command
  std::string substitute(const std::string &line);
  double evaluate(const std::string &expr);           // equal-style formulas, $(...) and `if` conditions
  double variable_value(const std::string &name);
  // script control flow (src/input.cpp: label :1057, jump :1011, next :1079, if :851, include :989)
  std::string jump_file, jump_label;                  // set by `jump`, consumed by file()
  bool jump_pending = false, jump_skip = false, quit_requested = false;
  int file_depth = 0;

  // error state for the C API (src/library.cpp LAMMPS_EXCEPTIONS behaviour)
  std::string last_error;
  bool has_error = false;

  // extract_* scratch (borrowed pointers handed to the caller)
  std::map<std::string, std::vector<double>> scratch_d;
  std::map<std::string, std::vector<int>> scratch_i;
  std::vector<double *> scratch_rows;
  double scratch_scalar = 0.0;
  int scratch_int = 0;
  // lammps_extract_compute: values of the thermo computes and the step they were evaluated on (Compute::invoked_*)
  struct ComputeCache {
    long invoked = -1;                 // ntimestep of the evaluation ...
    size_t stamp = 0;                  // ... and thermo_log.size() then (a run in between re-evaluates)
    long edits = -1;                   // ... and Engine::dev_edits then (a subset scatter in between re-evaluates)
    double scalar = 0.0;
    std::vector<double> vector;        // global vector, or property/local values (rows x cols)
    std::vector<double *> rows;        // property/local with several attributes: row pointers (array_local)
    int size_vector = 0, size_rows = 0, size_cols = 0;
  };
  std::map<std::string, ComputeCache> compute_cache;
};

// helpers
double numeric(const std::string &s);
int inumeric(const std::string &s);
std::vector<std::string> split_words(const std::string &line);
void bounds(const std::string &s, int nmax, int &lo, int &hi);   // "*", "n*", "*m", "n*m" type ranges (src/utils.cpp bounds)

// While it lives, formulas are evaluated for variable `var` of a fix of style `style` and may read nothing that lives on the
// device (Parser, input.cpp); what was set before comes back when it goes, also on an exception
struct HostOnlyScope {
  Engine *e;
  std::string was_for, was_style;
  HostOnlyScope(Engine *en, const std::string &var, const std::string &style) : e(en), was_for(en->host_only_for), was_style(en->host_only_style) {
    e->host_only_for = var; e->host_only_style = style;
  }
  ~HostOnlyScope() { e->host_only_for = was_for; e->host_only_style = was_style; }
  HostOnlyScope(const HostOnlyScope &) = delete;
  HostOnlyScope &operator=(const HostOnlyScope &) = delete;
};

}  // namespace lmp_le
