// fixes.cpp — fix styles of the hot path, registered under the reference's style names
// (src/fix_nve.h, src/fix_langevin.h, src/USER-LE/fix_extrusion.h:14-18, fix_ex_load.h, fix_ex_unload.h).
// Argument grammars and error strings follow the reference constructors.
#include <cmath>
#include <cstring>

#include "comm.h"
#include "device.h"
#include "indent_inl.h"

namespace lmp_le {

void dd_gather_positions(DeviceState &d, Comm &comm);
void dd_gather_needed(DeviceState &d, Comm &comm, int btype, bool with_nbrs);

static int fix_group(Engine *e, const std::vector<std::string> &arg) {      // src/fix.cpp:67-69
  const int bit = e->group_bit(arg[1]);
  if (!bit) throw LammpsError("Could not find fix group ID");
  return bit;
}

// The LE fixes count on every bond being stored with BOTH of its atoms (`num_bond == 2` for a free backbone bead,
// fix_ex_load.cpp:481-483; bondcount per owned end, fix_extrusion.cpp:281-295).  With newton_bond on the reference stores a
// bond once, those tests never pass and nothing is ever loaded; this engine always stores both copies, so it would NOT
// reproduce that run: refuse instead of silently differing.
static void need_newton_bond_off(Engine *e, const std::string &style) {
  if (e->newton_bond)
    throw LammpsError("fix " + style + " needs newton_bond off (`newton off` or `newton on off`): with newton_bond on the "
                      "reference stores each bond on one atom only and the fix's bond counts never match");
}
// fix ID group nve  (src/fix_nve.cpp:33-45)
FixNVE::FixNVE(Engine *e, const std::vector<std::string> &arg) {
  eng = e; id = arg[0]; group = arg[1]; style = arg[2];
  if (arg.size() < 3) throw LammpsError("Illegal fix nve command");
  groupbit = fix_group(e, arg);
  has_initial_integrate = has_final_integrate = true;
}

// fix ID group langevin Tstart Tstop damp seed  (src/fix_langevin.cpp:54-196)
FixLangevin::FixLangevin(Engine *e, const std::vector<std::string> &arg) {
  eng = e; id = arg[0]; group = arg[1]; style = arg[2];
  if (arg.size() < 7) throw LammpsError("Illegal fix langevin command");
  groupbit = fix_group(e, arg);
  t_start = numeric(arg[3]);
  t_stop = numeric(arg[4]);
  t_period = numeric(arg[5]);
  seed = inumeric(arg[6]);
  if (t_period <= 0.0) throw LammpsError("Fix langevin period must be > 0.0");
  if (seed <= 0) throw LammpsError("Illegal fix langevin command");
  // optional keywords (src/fix_langevin.cpp:105-155): `scale` and `zero` are implemented, the others only at their defaults
  ratio.assign(e->ntypes + 1, 1.0);
  for (size_t k = 7; k < arg.size();) {
    const std::string &kw = arg[k];
    if (kw == "scale") {
      if (k + 3 > arg.size()) throw LammpsError("Illegal fix langevin command");
      int itype = inumeric(arg[k + 1]);
      double sc = numeric(arg[k + 2]);
      if (itype <= 0 || itype > e->ntypes) throw LammpsError("Illegal fix langevin command");
      ratio[itype] = sc;
      k += 3;
    } else if (kw == "zero" || kw == "tally" || kw == "omega" || kw == "angmom" || kw == "gjf") {
      if (k + 2 > arg.size()) throw LammpsError("Illegal fix langevin command");
      const std::string &val = arg[k + 1];
      if (kw == "zero") {
        if (val != "yes" && val != "no") throw LammpsError("Illegal fix langevin command");
        zeroflag = val == "yes";
      } else if (val != "no")
        throw LammpsError("MI355X engine: fix langevin " + kw + " " + val + " is not supported");
      k += 2;
    } else throw LammpsError("Illegal fix langevin command");
  }
  rng.seed(seed);   // seed + comm->me, me = 0
  has_post_force = true;
}

// fix ID group spring/self K [xyz|xy|xz|yz|x|y|z]  (src/fix_spring_self.cpp:34-91).  The origin of a member is its unwrapped
// position at this command (Domain::unmap: x + image * prd); when a run has left the newest state on the device it is fetched
// first - a whole-system download, the command is not on the hot path
FixSpringSelf::FixSpringSelf(Engine *e, const std::vector<std::string> &arg) {
  eng = e; id = arg[0]; group = arg[1]; style = arg[2];
  kind = FORCEOP_SPRING;
  const char *ill = "Illegal fix spring/self command";
  if (arg.size() < 4 || arg.size() > 5) throw LammpsError(ill);
  groupbit = fix_group(e, arg);
  k = numeric(arg[3]);
  if (k <= 0.0) throw LammpsError(ill);
  if (arg.size() == 5) {
    const std::string &w = arg[4];
    if (w == "xyz") mask = 7;
    else if (w == "xy") mask = 3;
    else if (w == "xz") mask = 5;
    else if (w == "yz") mask = 6;
    else if (w == "x") mask = 1;
    else if (w == "y") mask = 2;
    else if (w == "z") mask = 4;
    else throw LammpsError(ill);
  }
  e->download();
  const int n = e->natoms;
  xorig.assign(3 * (size_t)n, 0.0);
  for (int i = 0; i < n; i++) {
    if (groupbit != 1 && !(e->gmask[i] & groupbit)) continue;
    for (int c = 0; c < 3; c++) xorig[3 * (size_t)i + c] = e->x[3 * (size_t)i + c] + e->image[3 * (size_t)i + c] * e->box.prd[c];
  }
  has_energy = true;                 // THERMO_ENERGY in setmask(); no virial_flag
  has_post_force = true;
}

// one force word of addforce / setforce: a number, `v_name` (refused: the values would have to be evaluated per step, or per
// bead, between two launches), or - setforce - NULL
static bool force_word(const std::string &w, const std::string &style, bool null_ok, double &val) {
  if (w.rfind("v_", 0) == 0)
    throw LammpsError("MI355X engine: fix " + style + " with a variable force (" + w + ") is not supported, equal- or atom-style");
  if (null_ok && w == "NULL") return false;
  val = numeric(w);
  return true;
}

// fix ID group addforce fx fy fz [every N] [region R] [energy v_name]  (src/fix_addforce.cpp:36-119)
FixAddForce::FixAddForce(Engine *e, const std::vector<std::string> &arg) {
  eng = e; id = arg[0]; group = arg[1]; style = arg[2];
  kind = FORCEOP_ADD;
  const char *ill = "Illegal fix addforce command";
  if (arg.size() < 6) throw LammpsError(ill);
  groupbit = fix_group(e, arg);
  for (int c = 0; c < 3; c++) force_word(arg[3 + c], style, false, v[c]);
  for (size_t a = 6; a < arg.size(); a += 2) {
    if (arg[a] == "every") {
      if (a + 2 > arg.size()) throw LammpsError(ill);
      every = atoi(arg[a + 1].c_str());
      if (every <= 0) throw LammpsError(ill);
    } else if (arg[a] == "region") {
      if (a + 2 > arg.size()) throw LammpsError(ill);
      if (!e->regions.count(arg[a + 1])) throw LammpsError("Region ID for fix addforce does not exist");
      throw LammpsError("MI355X engine: fix addforce with the region keyword is not supported");
    } else if (arg[a] == "energy") {
      if (a + 2 > arg.size()) throw LammpsError(ill);
      if (arg[a + 1].rfind("v_", 0) != 0) throw LammpsError(ill);
      estr = arg[a + 1].substr(2);
    } else throw LammpsError(ill);
  }
  has_energy = has_virial = true;    // THERMO_ENERGY, virial_flag = 1
  has_post_force = true;
}

// fix ID group setforce fx|NULL fy|NULL fz|NULL [region R]  (src/fix_setforce.cpp:36-106)
FixSetForce::FixSetForce(Engine *e, const std::vector<std::string> &arg) {
  eng = e; id = arg[0]; group = arg[1]; style = arg[2];
  kind = FORCEOP_SET;
  const char *ill = "Illegal fix setforce command";
  if (arg.size() < 6) throw LammpsError(ill);
  groupbit = fix_group(e, arg);
  mask = 0;
  for (int c = 0; c < 3; c++) if (force_word(arg[3 + c], style, true, v[c])) mask |= 1 << c;
  for (size_t a = 6; a < arg.size(); a += 2) {
    if (arg[a] == "region") {
      if (a + 2 > arg.size()) throw LammpsError(ill);
      if (!e->regions.count(arg[a + 1])) throw LammpsError("Region ID for fix setforce does not exist");
      throw LammpsError("MI355X engine: fix setforce with the region keyword is not supported");
    } else throw LammpsError(ill);
  }
  has_post_force = true;
}

// init() of the three (src/fix_addforce.cpp:149-210, fix_setforce.cpp:134-197)
void FixForceOp::init() {
  if (kind == FORCEOP_ADD && !estr.empty()) {
    if (!eng->variables.count(estr)) throw LammpsError("Variable name for fix addforce does not exist");
    throw LammpsError("Cannot use variable energy with constant force in fix addforce");
  }
  // setforce under r-RESPA zeroes the members' force on every level but one: not carried by the per-level arrays here
  if (kind == FORCEOP_SET && eng->respa_levels > 0)
    throw LammpsError("MI355X engine: fix setforce under run_style respa is not supported (it acts on every level)");
  if (kind == FORCEOP_SPRING && xorig.size() != 3 * (size_t)eng->natoms)
    throw LammpsError("MI355X engine: the atom count changed since fix spring/self " + id + " stored its origins");
}
ForceOpEntry FixForceOp::entry() const {
  ForceOpEntry o{};
  o.kind = kind; o.groupbit = groupbit; o.every = every; o.mask = mask; o.k = k;
  for (int c = 0; c < 3; c++) o.v[c] = v[c];
  return o;
}
// spring/self: the spring energy (fix_spring_self.cpp:176-179: the sum of k * d^2, halved); addforce: -sum f . x_unwrapped
double FixForceOp::compute_scalar() {
  if (kind == FORCEOP_SPRING) return 0.5 * sums[0];
  if (kind == FORCEOP_ADD) return sums[0];
  throw LammpsError("Fix does not compute a scalar");
}
// addforce | setforce: the members' total force before the fix acted (foriginal)
double FixForceOp::compute_vector(int n) {
  if (kind == FORCEOP_SPRING) throw LammpsError("Fix does not compute a vector");
  return sums[1 + n];
}

// fix ID group adapt N pair pstyle pparam I J v_name ... [reset yes|no] [scale yes|no]  (src/fix_adapt.cpp:45-215).  Pair
// parameters only, and of those the ones PairSoft::extract and PairLJCut::extract expose: soft a, lj/cut epsilon, lj/cut sigma.
// The group is parsed and, as in the reference, not used for pair parameters.
FixAdapt::FixAdapt(Engine *e, const std::vector<std::string> &arg) {
  eng = e; id = arg[0]; group = arg[1]; style = arg[2];
  const char *ill = "Illegal fix adapt command";
  if (arg.size() < 5) throw LammpsError(ill);
  groupbit = fix_group(e, arg);
  nevery = inumeric(arg[3]);
  if (nevery < 0) throw LammpsError(ill);
  size_t k = 4;
  while (k < arg.size()) {
    if (arg[k] == "pair") {
      if (k + 6 > arg.size()) throw LammpsError(ill);
      Clause c;
      c.pstyle = arg[k + 1]; c.pparam = arg[k + 2];
      bounds(arg[k + 3], e->ntypes, c.ilo, c.ihi);
      bounds(arg[k + 4], e->ntypes, c.jlo, c.jhi);
      if (arg[k + 5].rfind("v_", 0) != 0) throw LammpsError(ill);
      c.var = arg[k + 5].substr(2);
      if (c.pstyle != "soft" && c.pstyle != "lj/cut")
        throw LammpsError("MI355X engine: fix adapt pair style " + c.pstyle + " is not supported (soft a, lj/cut epsilon, lj/cut sigma)");
      if (!((c.pstyle == "soft" && c.pparam == "a") || (c.pstyle == "lj/cut" && (c.pparam == "epsilon" || c.pparam == "sigma"))))
        throw LammpsError("MI355X engine: Fix adapt pair style param not supported: " + c.pstyle + " " + c.pparam);
      clauses.push_back(c);
      k += 6;
    } else if (arg[k] == "bond" || arg[k] == "kspace" || arg[k] == "atom") {
      const size_t n = arg[k] == "bond" ? 5 : arg[k] == "kspace" ? 2 : 3;
      if (k + n > arg.size()) throw LammpsError(ill);
      throw LammpsError("MI355X engine: fix adapt " + arg[k] + " is not supported (pair soft a, pair lj/cut epsilon | sigma)");
    } else break;
  }
  if (clauses.empty()) throw LammpsError(ill);
  for (; k < arg.size(); k += 2) {
    if (k + 2 > arg.size()) throw LammpsError(ill);
    const std::string &kw = arg[k], &val = arg[k + 1];
    if (val != "yes" && val != "no") throw LammpsError(ill);
    if (kw == "reset") resetflag = val == "yes";
    else if (kw == "scale") scaleflag = val == "yes";
    else if (kw == "mass") {}                    // (atom diameter only)
    else throw LammpsError(ill);
  }
}
std::vector<double> *FixAdapt::target(const Clause &c) const { return c.pparam == "sigma" ? &eng->pc_sig : &eng->pc_eps; }
void FixAdapt::init() {
  const int nt = eng->ntypes + 1;
  for (auto &c : clauses) {
    auto vi = eng->var_info.find(c.var);
    if (eng->variables.find(c.var) == eng->variables.end()) throw LammpsError("Variable name for fix adapt does not exist");
    if (vi == eng->var_info.end() || vi->second.style != "equal") throw LammpsError("Variable for fix adapt is invalid style");
    if (c.pstyle != eng->pair_style_name()) throw LammpsError("Fix adapt pair style does not exist");
    const std::vector<double> &arr = *target(c);
    if ((int)arr.size() != nt * nt) throw LammpsError("All pair coeffs are not set");
    c.orig = arr;                                // (array_orig: the values as this run finds them, :460-466)
    // the formula is evaluated on the host between two launches of a run: one that reads an energy, a temperature, the
    // pressure or a fix is refused here, at the run command, with the name of what it reads (Parser, input.cpp)
    struct Dry { Engine *e; bool was; Dry(Engine *en, const std::string &v) : e(en), was(en->in_run) { e->in_run = true; e->host_only_for = v; }
                 ~Dry() { e->in_run = was; e->host_only_for.clear(); } } dry(eng, c.var);
    (void)eng->variable_value(c.var);
  }
}

// fix ID group indent K <sphere x y z R | cylinder dim c1 c2 R | plane dim pos lo|hi> [side in|out] [units box|lattice]
// (src/fix_indent.cpp:41-91, options :405-528): the keywords in any order, each geometric value a number or v_name.  There is no
// lattice command here, so both `units` values scale by 1 (as `region` treats them)
FixIndent::FixIndent(Engine *e, const std::vector<std::string> &arg) {
  eng = e; id = arg[0]; group = arg[1]; style = arg[2];
  const char *ill = "Illegal fix indent command";
  if (arg.size() < 4) throw LammpsError(ill);
  groupbit = fix_group(e, arg);
  k = numeric(arg[3]);
  k3 = k / 3.0;
  bool have = false;
  auto read = [&](const std::string &w, int slot) {
    if (w.rfind("v_", 0) == 0) vstr[slot] = w.substr(2);
    else value[slot] = numeric(w);
  };
  size_t i = 4;
  const size_t n = arg.size();
  while (i < n) {
    if (arg[i] == "sphere") {
      if (i + 5 > n) throw LammpsError(ill);
      for (int c = 0; c < 4; c++) read(arg[i + 1 + c], c);
      istyle = INDENT_SPHERE; have = true;
      i += 5;
    } else if (arg[i] == "cylinder") {
      if (i + 5 > n) throw LammpsError(ill);
      if (arg[i + 1] == "x") { cdim = 0; read(arg[i + 2], 1); read(arg[i + 3], 2); }
      else if (arg[i + 1] == "y") { cdim = 1; read(arg[i + 2], 0); read(arg[i + 3], 2); }
      else if (arg[i + 1] == "z") { cdim = 2; read(arg[i + 2], 0); read(arg[i + 3], 1); }
      else throw LammpsError(ill);
      read(arg[i + 4], 3);
      istyle = INDENT_CYLINDER; have = true;
      i += 5;
    } else if (arg[i] == "plane") {
      if (i + 4 > n) throw LammpsError(ill);
      if (arg[i + 1] == "x") cdim = 0;
      else if (arg[i + 1] == "y") cdim = 1;
      else if (arg[i + 1] == "z") cdim = 2;
      else throw LammpsError(ill);
      read(arg[i + 2], 4);
      if (arg[i + 3] == "lo") planeside = -1;
      else if (arg[i + 3] == "hi") planeside = 1;
      else throw LammpsError(ill);
      istyle = INDENT_PLANE; have = true;
      i += 4;
    } else if (arg[i] == "units") {
      if (i + 2 > n || (arg[i + 1] != "box" && arg[i + 1] != "lattice")) throw LammpsError(ill);
      i += 2;
    } else if (arg[i] == "side") {
      if (i + 2 > n) throw LammpsError(ill);
      if (arg[i + 1] == "in") side = 1;
      else if (arg[i + 1] == "out") side = 0;
      else throw LammpsError(ill);
      i += 2;
    } else throw LammpsError(ill);
  }
  if (!have) throw LammpsError(ill);
  has_post_force = true;
}
// FixIndent::init (:118-160): the variables exist and are equal-style (the x variable's text differs, as in the reference).  A
// formula is evaluated on the host between two launches of a run: one that reads what lives on the device is refused here, at
// the run command, with the name of what it reads (Parser, input.cpp)
void FixIndent::init() {
  for (int c = 0; c < 5; c++) {
    if (vstr[c].empty()) continue;
    if (eng->variables.find(vstr[c]) == eng->variables.end()) throw LammpsError("Variable name for fix indent does not exist");
    auto vi = eng->var_info.find(vstr[c]);
    if (vi == eng->var_info.end() || vi->second.style != "equal")
      throw LammpsError(c == 0 ? "Variable for fix indent is invalid style" : "Variable for fix indent is not equal style");
    struct Dry { Engine *e; bool was; Dry(Engine *en) : e(en), was(en->in_run) { e->in_run = true; } ~Dry() { e->in_run = was; } } dry(eng);
    HostOnlyScope scope(eng, vstr[c], "indent");
    (void)eng->variable_value(vstr[c]);
  }
}
// FixIndent::post_force's head (:196-212, :250-280, :332-334): the values of this step, the centre through Domain::remap (the
// box is periodic in every dimension: while below lo add a period, while at or above hi take one off, then max(coord, lo))
IndentEntry FixIndent::entry() {
  double v[5];
  for (int c = 0; c < 5; c++) {
    v[c] = value[c];
    if (vstr[c].empty()) continue;
    HostOnlyScope scope(eng, vstr[c], "indent");
    v[c] = eng->variable_value(vstr[c]);
  }
  IndentEntry e{};
  e.kind = istyle; e.axis = cdim; e.groupbit = groupbit;
  e.k = k; e.k3 = k3;
  if (istyle == INDENT_PLANE) {
    e.side = planeside;
    e.r = v[4];
    return e;
  }
  e.side = side;
  e.r = v[3];
  const Box &b = eng->box;
  for (int c = 0; c < 3; c++) {
    const double x = (istyle == INDENT_CYLINDER && c == cdim) ? b.lo[c] : v[c];      // (the axis coordinate is not used: "just near box")
    e.ctr[c] = indent_remap(x, b.lo[c], b.hi[c], b.prd[c]);
  }
  return e;
}

// fix ID group wall/region region-ID style args cutoff  (src/fix_wall_region.cpp:35-92): lj93 | lj126 | lj1043 | harmonic take
// epsilon sigma cutoff, morse takes D0 alpha r0 cutoff
FixWallRegion::FixWallRegion(Engine *e, const std::vector<std::string> &arg) {
  eng = e; id = arg[0]; group = arg[1]; style = arg[2];
  const char *ill = "Illegal fix wall/region command";
  if (arg.size() < 8) throw LammpsError(ill);
  groupbit = fix_group(e, arg);
  idregion = arg[3];
  auto it = e->regions.find(idregion);
  if (it == e->regions.end()) throw LammpsError("Region ID for fix wall/region does not exist");
  bool colloid = false;
  if (arg[4] == "lj93") wstyle = WALL_LJ93;
  else if (arg[4] == "lj126") wstyle = WALL_LJ126;
  else if (arg[4] == "lj1043") wstyle = WALL_LJ1043;
  else if (arg[4] == "colloid") colloid = true;
  else if (arg[4] == "harmonic") wstyle = WALL_HARMONIC;
  else if (arg[4] == "morse") wstyle = WALL_MORSE;
  else throw LammpsError(ill);
  if (wstyle == WALL_MORSE && !colloid) {
    if (arg.size() != 9) throw LammpsError(ill);
    epsilon = numeric(arg[5]); alpha = numeric(arg[6]); sigma = numeric(arg[7]); cutoff = numeric(arg[8]);
  } else {
    if (arg.size() != 8) throw LammpsError(ill);
    epsilon = numeric(arg[5]); sigma = numeric(arg[6]); cutoff = numeric(arg[7]);
  }
  if (cutoff <= 0.0) throw LammpsError("Fix wall/region cutoff <= 0.0");
  // (the reference says this at init(): no atom style of this engine has a radius, so the command is where it ends)
  if (colloid) throw LammpsError("Fix wall/region colloid requires atom style sphere");
  // the contact sets the kernels restate: sphere and block from both sides, cylinder from inside
  init();
  has_post_force = true;
}
void FixWallRegion::init() {      // :115-121 (a region can be deleted, and defined again, between the command and a run)
  auto it = eng->regions.find(idregion);
  if (it == eng->regions.end()) throw LammpsError("Region ID for fix wall/region does not exist");
  const Engine::Region &r = it->second;
  if (r.style == "union" || r.style == "intersect" || (r.style == "cylinder" && !r.interior))
    throw LammpsError("MI355X engine: fix wall/region does not support region style " + r.style +
                      (r.style == "cylinder" ? " with side out" : ""));
}
WallEntry FixWallRegion::entry() const {      // :145-190, expression by expression
  WallEntry w{};
  const Engine::Region &r = eng->regions.at(idregion);
  w.kind = r.style == "block" ? WALL_BLOCK : r.style == "sphere" ? WALL_SPHERE : WALL_CYLINDER;
  w.interior = r.interior ? 1 : 0;
  w.axis = r.axis - 'x';
  for (int k = 0; k < 6; k++) w.p[k] = r.p[k];
  w.style = wstyle; w.groupbit = groupbit;
  w.cutoff = cutoff; w.epsilon = epsilon; w.sigma = sigma; w.alpha = alpha;
  double *c = w.coeff;
  const double MY_2PI = 6.28318530717958647692;
  if (wstyle == WALL_LJ93) {
    c[1] = 6.0 / 5.0 * epsilon * pow(sigma, 9.0);
    c[2] = 3.0 * epsilon * pow(sigma, 3.0);
    c[3] = 2.0 / 15.0 * epsilon * pow(sigma, 9.0);
    c[4] = epsilon * pow(sigma, 3.0);
    double rinv = 1.0 / cutoff;
    double r2inv = rinv * rinv;
    double r4inv = r2inv * r2inv;
    w.offset = c[3] * r4inv * r4inv * rinv - c[4] * r2inv * rinv;
  } else if (wstyle == WALL_LJ126) {
    c[1] = 48.0 * epsilon * pow(sigma, 12.0);
    c[2] = 24.0 * epsilon * pow(sigma, 6.0);
    c[3] = 4.0 * epsilon * pow(sigma, 12.0);
    c[4] = 4.0 * epsilon * pow(sigma, 6.0);
    double r2inv = 1.0 / (cutoff * cutoff);
    double r6inv = r2inv * r2inv * r2inv;
    w.offset = r6inv * (c[3] * r6inv - c[4]);
  } else if (wstyle == WALL_LJ1043) {
    c[1] = MY_2PI * 2.0 / 5.0 * epsilon * pow(sigma, 10.0);
    c[2] = MY_2PI * epsilon * pow(sigma, 4.0);
    c[3] = MY_2PI * pow(2.0, 1 / 2.0) / 3 * epsilon * pow(sigma, 3.0);
    c[4] = 0.61 / pow(2.0, 1 / 2.0) * sigma;
    c[5] = c[1] * 10.0;
    c[6] = c[2] * 4.0;
    c[7] = c[3] * 3.0;
    double rinv = 1.0 / cutoff;
    double r2inv = rinv * rinv;
    double r4inv = r2inv * r2inv;
    w.offset = c[1] * r4inv * r4inv * r2inv - c[2] * r4inv - c[3] * pow(cutoff + c[4], -3.0);
  } else if (wstyle == WALL_MORSE) {
    c[1] = 2 * epsilon * alpha;
    double alpha_dr = -alpha * (cutoff - sigma);
    w.offset = epsilon * (exp(2.0 * alpha_dr) - 2.0 * exp(alpha_dr));
  }
  return w;
}

// fix ID group extrusion N1 neutral ctcf_left ctcf_right through_prob btype [ctcf_left_right]
// (src/USER-LE/fix_extrusion.cpp:38-142; narg < 8 is rejected but arg[8] is read, so 9 are needed)
FixExtrusion::FixExtrusion(Engine *e, const std::vector<std::string> &arg) {
  eng = e; id = arg[0]; group = arg[1]; style = arg[2];
  if (arg.size() < 9) throw LammpsError("Illegal fix extrusion command");
  groupbit = fix_group(e, arg);
  nevery = inumeric(arg[3]);
  if (nevery <= 0) throw LammpsError("Illegal fix extrusion command, n_steps <= 0");
  neutral = inumeric(arg[4]); ctcf_left = inumeric(arg[5]); ctcf_right = inumeric(arg[6]);
  if (neutral < 1 || neutral > e->ntypes || ctcf_left < 1 || ctcf_left > e->ntypes || ctcf_right < 1 ||
      ctcf_right > e->ntypes)
    throw LammpsError("Invalid atom type (CTCF) in fix extrusion command");
  through_prob = numeric(arg[7]);
  if (through_prob < 0 || through_prob > 1)
    throw LammpsError("Invalid probability to pass through CTCF in fix extrusion command");
  btype = inumeric(arg[8]);
  if (btype < 1 || btype > e->nbondtypes) throw LammpsError("Invalid atom type in fix extrusion command");
  ctcf_lr = (arg.size() == 10) ? inumeric(arg[9]) : -1;
  e->say("Attention! Type of bidirectional CTCF is " + std::to_string(ctcf_lr) + "\n");
  e->say("Amount of args in loop extrusion is " + std::to_string(arg.size()) + "\n");
  if (ctcf_lr > e->ntypes) throw LammpsError("Invalid atom type in fix extrusion command");
  if (e->atom_style == "atomic") throw LammpsError("Cannot use fix extrusion with non-molecular systems");
  need_newton_bond_off(e, style);
  rng.seed(12345);   // hard-coded 12345 + me (:98-99)
  e->say("Attention! maxspecial = " + std::to_string(e->maxspecial) + "\n");
  force_reneighbor = true;
  has_post_integrate = true;
  has_post_integrate_respa = false;      // :166-171
}
double FixExtrusion::compute_vector(int n) { return n == 0 ? (double)last_break : 0.0; }   // :1496-1501

// fix ID group ex_load Nevery itype jtype Rmin bondtype [iparam ..] [jparam ..] [prob f seed] (:39-176)
FixExLoad::FixExLoad(Engine *e, const std::vector<std::string> &arg) {
  eng = e; id = arg[0]; group = arg[1]; style = arg[2];
  stock = (style == "bond/create");
  phase = stock ? 0 : 3;                                  // src/MC/fix_bond_create.cpp:356 vs src/USER-LE/fix_ex_load.cpp:338
  const std::string ill = "Illegal fix " + style + " command";
  if (arg.size() < 8) throw LammpsError(ill);
  groupbit = fix_group(e, arg);
  nevery = inumeric(arg[3]);
  if (nevery <= 0) throw LammpsError(ill);
  iatomtype = inumeric(arg[4]); jatomtype = inumeric(arg[5]);
  double cutoff = numeric(arg[6]);
  btype = inumeric(arg[7]);
  if (iatomtype < 1 || iatomtype > e->ntypes || jatomtype < 1 || jatomtype > e->ntypes)
    throw LammpsError("Invalid atom type in fix " + style + " command");
  if (cutoff < 0.0) throw LammpsError(ill);
  if (btype < 1 || btype > e->nbondtypes) throw LammpsError("Invalid bond type in fix " + style + " command");
  cutsq = cutoff * cutoff;
  inewtype = iatomtype; jnewtype = jatomtype;
  size_t iarg = 8;
  while (iarg < arg.size()) {
    if (arg[iarg] == "iparam") {
      if (iarg + 3 > arg.size()) throw LammpsError(ill);
      imaxbond = inumeric(arg[iarg + 1]); inewtype = inumeric(arg[iarg + 2]);
      if (imaxbond < 0) throw LammpsError(ill);
      if (inewtype < 1 || inewtype > e->ntypes) throw LammpsError("Invalid atom type in fix " + style + " command");
      iarg += 3;
    } else if (arg[iarg] == "jparam") {
      if (iarg + 3 > arg.size()) throw LammpsError(ill);
      jmaxbond = inumeric(arg[iarg + 1]); jnewtype = inumeric(arg[iarg + 2]);
      if (jmaxbond < 0) throw LammpsError(ill);
      if (jnewtype < 1 || jnewtype > e->ntypes) throw LammpsError("Invalid atom type in fix " + style + " command");
      iarg += 3;
    } else if (arg[iarg] == "prob") {
      if (iarg + 3 > arg.size()) throw LammpsError(ill);
      fraction = numeric(arg[iarg + 1]); seed = inumeric(arg[iarg + 2]);
      if (fraction < 0.0 || fraction > 1.0) throw LammpsError(ill);
      if (seed <= 0) throw LammpsError(ill);
      iarg += 3;
    } else if (arg[iarg] == "atype" || arg[iarg] == "dtype" || arg[iarg] == "itype") {
      if (iarg + 2 > arg.size()) throw LammpsError(ill);
      // fix_ex_load.cpp:108-122 parse the type; :236-254 (and MC/fix_bond_create.cpp:256-270) switch the creation of angles /
      // dihedrals / impropers on only `if (atype && force->angle)`, i.e. when the script defined such a style.  Angles are
      // created (kernels_le.hip dev_create_angles); this engine has no dihedral / improper styles, so dtype / itype stay
      // without effect exactly as in the reference for a script without such styles.
      if (inumeric(arg[iarg + 1]) < 0) throw LammpsError(ill);
      if (arg[iarg] == "atype") atype = inumeric(arg[iarg + 1]);
      iarg += 2;
    } else throw LammpsError(ill);
  }
  if (e->atom_style == "atomic") throw LammpsError("Cannot use fix " + style + " with non-molecular systems");
  need_newton_bond_off(e, style);
  if (iatomtype == jatomtype && (imaxbond != jmaxbond || inewtype != jnewtype))
    throw LammpsError("Inconsistent iparam/jparam values in fix " + style + " command");
  rng.seed(seed);
  force_reneighbor = true;
  has_post_integrate = true;
}
void FixExLoad::init() {
  // src/USER-LE/fix_ex_load.cpp:217-218
  if (!eng->pair_force()) throw LammpsError("Fix " + style + " cutoff is longer than pairwise cutoff");      // (force->pair == nullptr)
  int nt = eng->ntypes + 1;
  if (cutsq > eng->cutsq[iatomtype * nt + jatomtype])
    throw LammpsError("Fix " + style + " cutoff is longer than pairwise cutoff");
}
// FixBondCreate::setup (src/MC/fix_bond_create.cpp:302-345): count the bonds of btype each bead stores, once
void FixExLoad::setup() {
  if (!stock || counted) return;
  counted = true;
  const bool was_current = eng->host_current;
  eng->download();                   // setup runs with the device already holding the newest state
  eng->host_current = was_current;   // ... and the run that follows will change it again
  bondcount.assign((size_t)eng->natoms + 2, 0);
  for (int i = 0; i < eng->natoms; i++)
    for (int m = 0; m < eng->num_bond[i]; m++)
      if (eng->bond_type[(size_t)i * eng->bpa + m] == btype) bondcount[i + 1]++;
}
double FixExLoad::compute_vector(int n) { return n == 0 ? (double)last_create : (double)total_create; }

// fix ID group ex_unload Nevery bondtype Rmax [prob fraction seed]  (src/USER-LE/fix_ex_unload.cpp:34-115)
FixExUnload::FixExUnload(Engine *e, const std::vector<std::string> &arg) {
  eng = e; id = arg[0]; group = arg[1]; style = arg[2];
  // the reference's two files are the same text but for the firing step (src/MC/fix_bond_break.cpp:178 `% nevery`,
  // src/USER-LE/fix_ex_unload.cpp:178 `% nevery - 2`)
  phase = (style == "bond/break") ? 0 : 2;
  const std::string ill = "Illegal fix " + style + " command";
  if (arg.size() < 6) throw LammpsError(ill);
  groupbit = fix_group(e, arg);
  nevery = inumeric(arg[3]);
  if (nevery <= 0) throw LammpsError(ill);
  btype = inumeric(arg[4]);
  double cutoff = numeric(arg[5]);
  if (btype < 1 || btype > e->nbondtypes) throw LammpsError("Invalid bond type in fix " + style + " command");
  if (cutoff < 0.0) throw LammpsError(ill);
  cutsq = cutoff * cutoff;
  size_t iarg = 6;
  while (iarg < arg.size()) {
    if (arg[iarg] == "prob") {
      if (iarg + 3 > arg.size()) throw LammpsError(ill);
      fraction = numeric(arg[iarg + 1]); seed = inumeric(arg[iarg + 2]);
      if (fraction < 0.0 || fraction > 1.0) throw LammpsError(ill);
      if (seed <= 0) throw LammpsError(ill);
      iarg += 3;
    } else throw LammpsError(ill);
  }
  need_newton_bond_off(e, style);
  rng.seed(seed);
  force_reneighbor = true;
  has_post_integrate = true;
}
void FixExUnload::init() { angleflag = (eng->apa > 0 && eng->nangles > 0) ? 1 : 0; }
double FixExUnload::compute_vector(int n) { return n == 0 ? (double)last_break : (double)total_break; }

// ---------------------------------------------------------------------------------------------
// post_integrate: firing rule + device launch + counter read-back (firing steps only)
// ---------------------------------------------------------------------------------------------
static int fix_index(Engine *e, Fix *f) {
  for (size_t k = 0; k < e->fixes.size(); k++) if (e->fixes[k].get() == f) return (int)k;
  return -1;
}
static int le_slot(Engine *e, Fix *f) {
  int s = 0;
  for (auto &g : e->fixes) {
    if (g.get() == f) return s;
    if (g->force_reneighbor) s++;
  }
  return s;
}
static void check_le_error(DeviceState &d, const std::string &style) {
  int code = d.flags_h[FLAG_ERROR];
  if (code) throw LammpsError(device_error_text(code, style));
}

void FixExtrusion::post_integrate() {
  if (eng->ntimestep % nevery - 1) return;               // src/USER-LE/fix_extrusion.cpp:265
  DeviceState &d = *eng->dev;
  int slot = le_slot(eng, this);
  if (slot >= LE_MAX_FIXES) throw LammpsError("MI355X engine supports at most " + std::to_string(LE_MAX_FIXES) + " extrusion/ex_load/ex_unload fixes");
  if (!rng_on_device) { le_rng_upload(d, slot, rng); rng_on_device = true; }
  eng->le_style = style;
  if (eng->world > 1) {
    // stored coordinates of the extruder ends and the beads they can step to: O(extruders) rows (dd_gather_needed); every
    // bead's (tag, x, xhold) only when the visit order is not the canonical one
    if (dd_le_fast(d)) dd_gather_needed(d, *eng->comm, btype, true); else dd_gather_positions(d, *eng->comm);
  }
  ExtrusionParams p{neutral, ctcf_left, ctcf_right, ctcf_lr, btype, through_prob, groupbit};
  launch_extrusion(d, p, slot);
  note_topology_changed(d);
  sync_flags(d);
  // the reference's order: the bondcount pass and the insert of a new bond stop it inside their loops (:292, :764), then the
  // two counts are compared (:808), and only then update_topology rebuilds special rows (:1081).  A bond that its higher end
  // cannot store leaves the counts equal and the reference running (ERR_ONE_SIDED: this engine stops)
  const int code = d.flags_h[FLAG_ERROR];
  if (code == ERR_EXT_MULTI || code == ERR_SPECIAL) check_le_error(d, style);
  last_break = d.flags_h[FLAG_COUNT_A];
  int created = d.flags_h[FLAG_COUNT_B];
  if (last_break != created) throw LammpsError(device_error_text(ERR_COUNT_MISMATCH, style));
  check_le_error(d, style);
  if (last_break) eng->le_reneigh_step[fix_index(eng, this)] = eng->ntimestep;
}

void FixExLoad::post_integrate() {
  if (eng->ntimestep % nevery - phase) return;           // src/USER-LE/fix_ex_load.cpp:338, src/MC/fix_bond_create.cpp:356
  DeviceState &d = *eng->dev;
  int slot = le_slot(eng, this);
  if (slot >= LE_MAX_FIXES) throw LammpsError("MI355X engine supports at most " + std::to_string(LE_MAX_FIXES) + " extrusion/ex_load/ex_unload fixes");
  if (!rng_on_device) { le_rng_upload(d, slot, rng); rng_on_device = true; }
  eng->le_style = style;
  // angles around new bonds only `if (atype && force->angle)` (fix_ex_load.cpp:236-240)
  const int angle_type_new = (atype > 0 && eng->angles_active()) ? atype : 0;
  if (angle_type_new > eng->nangletypes) throw LammpsError("Fix " + style + " angle type is invalid");
  ExLoadParams p{iatomtype, jatomtype, imaxbond, inewtype, jmaxbond, jnewtype, btype, cutsq, fraction, angle_type_new, groupbit};
  if (stock) {
    if (eng->world > 1) dd_gather_positions(d, *eng->comm);   // current positions by tag (ghost slots lag one step here)
    launch_bond_create(d, p, slot, bondcount.data(), (int)bondcount.size(), eng->comm);
  } else {
    if (eng->world > 1) {
      // canonical order: every rank decides the pairs whose storing bead it owns from its own list and (current) ghosts
      if (dd_le_fast(d)) eng->halo_exchange_once(); else dd_gather_positions(d, *eng->comm);
    }
    launch_ex_load(d, p, slot, eng->comm);
  }
  note_topology_changed(d);
  sync_flags(d);
  check_le_error(d, style);
  last_create = d.flags_h[FLAG_COUNT_A];
  total_create += last_create;
  eng->nbonds += last_create;
  if (angle_type_new) eng->nangles += d.flags_h[FLAG_COUNT_B] / 3;     // copies on three atoms each (fix_ex_load.cpp:760-765)
  if (last_create) eng->le_reneigh_step[fix_index(eng, this)] = eng->ntimestep;
  if (stock && last_create) bond_create_counts(d, bondcount.data(), (int)bondcount.size());
}

void FixExUnload::post_integrate() {
  if (eng->ntimestep % nevery - phase) return;           // src/USER-LE/fix_ex_unload.cpp:178, src/MC/fix_bond_break.cpp:178
  DeviceState &d = *eng->dev;
  int slot = le_slot(eng, this);
  if (slot >= LE_MAX_FIXES) throw LammpsError("MI355X engine supports at most " + std::to_string(LE_MAX_FIXES) + " extrusion/ex_load/ex_unload fixes");
  if (!rng_on_device) { le_rng_upload(d, slot, rng); rng_on_device = true; }
  eng->le_style = style;
  if (eng->world > 1) {
    if (dd_le_fast(d)) dd_gather_needed(d, *eng->comm, btype, false); else dd_gather_positions(d, *eng->comm);
  }
  ExUnloadParams p{btype, cutsq, fraction, angleflag, groupbit};
  launch_ex_unload(d, p, slot);
  note_topology_changed(d);
  sync_flags(d);
  check_le_error(d, style);
  last_break = d.flags_h[FLAG_COUNT_A];
  total_break += last_break;
  eng->nbonds -= last_break;
  if (angleflag) eng->nangles -= d.flags_h[FLAG_COUNT_B] / 3;
  if (last_break) eng->le_reneigh_step[fix_index(eng, this)] = eng->ntimestep;
}

}  // namespace lmp_le
