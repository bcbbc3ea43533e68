// minimize.cpp — `minimize`, `min_style cg | sd`, `min_modify` on the device.
//
// The host runs the reference's control flow in its operation order (src/minimize.cpp:31-72 Minimize::command, src/min.cpp:114-200
// Min::init, :206-341 setup, :428-464 run, :468-492 cleanup, :502-614 energy_force, src/min_cg.cpp:37-191, src/min_sd.cpp:37-114,
// src/min_linesearch.cpp:176-285 linemin_backtrack, :325-505 linemin_quadratic, :838-875 alpha_step, src/finish.cpp:194-218); every
// pass over the beads is a kernel of kernels_min.hip or one of the unfused force kernels.  One evaluation costs the host one wait:
// the energies, the dot products and the flags of the evaluation arrive together (DeviceState::min_rec, the flag page).
//
// Neighbor::decide under every 1 / delay 0 / check yes tests the displacement before every force evaluation.  Here the forces
// are enqueued on the present lists first and the test's answer arrives with them; when it says `moved`, the lists are rebuilt
// and the evaluation repeated, so the forces that are used are those on the rebuilt lists, as in the reference.  The force
// kernels are safe on lists the beads have outrun: entries stay valid indices, and what they compute is thrown away.
#include <chrono>
#include <cmath>
#include <cstring>

#include "comm.h"
#include "device.h"

namespace lmp_le {

namespace {
double wall_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// src/min.h:59-60
enum { MAXITER = 0, MAXEVAL, ETOL, FTOL, DOWNHILL, ZEROALPHA, ZEROFORCE, ZEROQUAD, TRSMALL, INTERROR, TIMEOUT, MAXVDOTF };
// src/min_linesearch.cpp:44-50, src/min.h EPS_ENERGY
constexpr double ALPHA_MAX = 1.0, ALPHA_REDUCE = 0.5, BACKTRACK_SLOPE = 0.4, QUADRATIC_TOL = 0.1, EMACH = 1.0e-8, EPS_QUAD = 1.0e-28;
constexpr double EPS_ENERGY = 1.0e-8;

struct Minimizer {
  Engine &e;
  DeviceState &d;
  const bool cg;
  double etol, ftol;
  long maxeval;
  const double triggersq;
  // Min's members
  double ecurrent = 0.0, eprevious = 0.0, einitial = 0.0, alpha_final = 0.0;
  long niter = 0, neval = 0, rebuilds = 0, ndanger = 0;
  // of the last evaluation: the dots, and the row of energies thermo prints
  double ff = 0.0, fh = 0.0, fg = 0.0, fmax2 = 0.0, fmaxc = 0.0;
  // f.h and max |h_ic| for the line search to come (known from the direction update: there f = g)
  double fdoth = 0.0, hmaxall = 0.0;
  double ke_sum = 0.0, k6[6] = {0, 0, 0, 0, 0, 0};
  ThermoRow row{};

  Minimizer(Engine &eng, double et, double ft, long me)
      : e(eng), d(*eng.dev), cg(eng.min_style == "cg"), etol(et), ftol(ft), maxeval(me), triggersq(0.25 * eng.skin * eng.skin) {}

  void wait() {                   // the one wait of an evaluation or a direction update: everything enqueued so far has run
    publish_flags(d, 1u << FLAG_MOVED);
    wait_flags(d);
    const int code = d.flags_h[FLAG_ERROR];
    if (code) throw LammpsError(device_error_text(code, e.le_style));
  }

  // forces, energies, the fixes with a min_post_force hook, the dots: enqueue, wait once, read the record
  void evaluate(bool with_ke) {
    e.compute_forces(true);
    e.post_force_sequence(nullptr, true, false);      // FixWallRegion | FixIndent | FixSpringSelf | FixAddForce | FixSetForce::min_post_force, in fix order; no thermostat
    if (with_ke) {
      TypeTables tt{};
      for (int t = 1; t <= e.ntypes; t++) tt.mass[t] = e.mass[t];
      launch_ke(d, tt);
    }
    launch_min_dots(d, cg, true);
    MinSources src;
    const bool ang = e.angles_active();
    enqueue_thermo_sums(d, e.postforce, ang, src);
    launch_min_collect(d, true, src);
    wait();
    const double *rec = d.min_rec;
    ff = rec[MIN_FF]; fh = rec[MIN_FH]; fg = rec[MIN_FG]; fmax2 = rec[MIN_FMAX2]; fmaxc = rec[MIN_FMAXC];
    double s[PostForce::SUMS_MAX], a8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const double *p = rec + MIN_DOT_COLS;
    for (int k = 0; k < 16; k++) s[k] = p[k];
    p += 16;
    if (ang) { for (int k = 0; k < 8; k++) a8[k] = p[k]; p += 8; }
    e.postforce.unpack_min_record(p, s);
    if (with_ke) ke_sum = s[14];      // (the velocities do not change in a minimisation)
    s[14] = ke_sum;
    row = e.thermo_from_sums(s, ang ? a8 : nullptr, e.want_ptensor ? k6 : nullptr);
    row.fnorm = std::sqrt(ff);
    row.fmax = fmaxc;
  }

  // Min::energy_force (src/min.cpp:502-614)
  double energy_force(int resetflag, bool with_ke = false) {
    evaluate(with_ke);
    e.ago++;
    if (d.flags_h[FLAG_MOVED]) {      // Neighbor::decide said yes: pbc, (Atom::sort), lists, then the forces that count
      if (e.ago == 1) { e.neigh_dangerous++; ndanger++; }     // (src/neighbor.cpp:1943: ago == max(every, delay))
      const bool sort_due = e.sortfreq > 0 && e.ntimestep >= e.nextsort;
      e.reneighbor(true, sort_due, false);
      rebuilds++;
      evaluate(with_ke);
      if (e.reneigh_pending) {        // the flags of the build came with the evaluation's
        e.reneigh_pending = false;
        if (d.flags_h[FLAG_NEIGH_OVERFLOW]) { e.regrow_lists(); evaluate(with_ke); }
      }
      if (resetflag) launch_min_reset_coords(d);      // FixMinimize::reset_coords
    }
    return row.pe;
  }

  // MinLineSearch::alpha_step
  double alpha_step(double alpha, int resetflag) {
    launch_min_move(d, alpha, triggersq);
    neval++;
    return energy_force(resetflag);
  }

  // the head both line searches share (src/min_linesearch.cpp:186-234, :338-387): 0, or the stop it ends the search with
  int linemin_head(double &fdothall, double &alphamax) {
    fdothall = fdoth;
    if (e.thermo_norm) fdothall /= (double)e.natoms;
    if (fdothall <= 0.0) return DOWNHILL;
    alphamax = std::min(ALPHA_MAX, e.min_dmax / hmaxall);
    if (hmaxall == 0.0) return ZEROFORCE;
    launch_min_store(d);
    return 0;
  }

  int linemin_backtrack(double eoriginal, double &alpha) {
    double fdothall, de_ideal, de;
    if (int stop = linemin_head(fdothall, alpha)) return stop;
    while (true) {
      ecurrent = alpha_step(alpha, 1);
      de_ideal = -BACKTRACK_SLOPE * alpha * fdothall;
      de = ecurrent - eoriginal;
      if (de <= de_ideal) return 0;
      alpha *= ALPHA_REDUCE;
      if (alpha <= 0.0 || de_ideal >= -EMACH) {
        ecurrent = alpha_step(0.0, 0);
        return de < 0.0 ? ETOL : ZEROALPHA;
      }
    }
  }

  int linemin_quadratic(double eoriginal, double &alpha) {
    double fdothall, alphamax, de_ideal, de;
    if (int stop = linemin_head(fdothall, alphamax)) return stop;
    alpha = alphamax;
    double fhprev = fdothall, engprev = eoriginal, alphaprev = 0.0;
    while (true) {
      ecurrent = alpha_step(alpha, 1);
      double fhn = fh;
      if (e.thermo_norm) fhn /= (double)e.natoms;      // (ff is divided too, :441-446, and not used)
      const double delfh = fhn - fhprev;
      if (std::fabs(fhn) < EPS_QUAD || std::fabs(delfh) < EPS_QUAD) {
        ecurrent = alpha_step(0.0, 0);
        return ZEROQUAD;
      }
      const double relerr = std::fabs(1.0 - (0.5 * (alpha - alphaprev) * (fhn + fhprev) + ecurrent) / engprev);
      const double alpha0 = alpha - (alpha - alphaprev) * fhn / delfh;
      if (relerr <= QUADRATIC_TOL && alpha0 > 0.0 && alpha0 < alphamax) {
        ecurrent = alpha_step(alpha0, 1);
        if (ecurrent - eoriginal < EMACH) return 0;
      }
      de_ideal = -BACKTRACK_SLOPE * alpha * fdothall;
      de = ecurrent - eoriginal;
      if (de <= de_ideal) return 0;
      fhprev = fhn;
      engprev = ecurrent;
      alphaprev = alpha;
      alpha *= ALPHA_REDUCE;
      if (alpha <= 0.0 || de_ideal >= -EMACH) {
        ecurrent = alpha_step(0.0, 0);
        return ZEROALPHA;
      }
    }
  }

  void output(bool last) {        // Output::write on an iteration that is due
    const long step = e.ntimestep;
    const bool thermo_due = last || step == e.endstep || (e.thermo_every > 0 && step % e.thermo_every == 0);
    if (thermo_due) {
      row.step = step;
      e.last_thermo = row;
      e.thermo_log.push_back(row);
      e.print_thermo(row);
    }
    const bool restart_due = e.restart_every > 0 && (last || step % e.restart_every == 0);
    e.dump_force_all = last;
    try { if (!e.dumps.empty()) e.write_dumps(step); } catch (...) { e.dump_force_all = false; throw; }
    e.dump_force_all = false;
    if (restart_due) e.write_periodic_restart(step);
  }

  // MinCG::iterate / MinSD::iterate
  int iterate(long maxiter) {
    const long ndoftotal = 3L * e.natoms;
    const long nlimit = std::min(2147483647L, ndoftotal);
    // h = g = f: the line search of the first iteration reads f.h = f.f and max |h| = max |f_ic| of the setup evaluation
    launch_min_direction(d, cg, 0.0);
    fdoth = ff; hmaxall = fmaxc;
    double gg = ff;
    for (long iter = 0; iter < maxiter; iter++) {
      if (e.timeout_forced) return TIMEOUT;
      e.ntimestep++;
      niter++;
      eprevious = ecurrent;
      const int fail = e.min_linestyle == 0 ? linemin_backtrack(ecurrent, alpha_final) : linemin_quadratic(ecurrent, alpha_final);
      if (fail) return fail;
      if (neval >= maxeval) return MAXEVAL;
      if (std::fabs(ecurrent - eprevious) < etol * 0.5 * (std::fabs(ecurrent) + std::fabs(eprevious) + EPS_ENERGY)) return ETOL;
      const double dot0 = ff, dot1 = fg;
      if (ftol > 0.0) {
        const double fdotf = e.min_normstyle == 1 ? fmax2 : e.min_normstyle == 2 ? fmaxc * fmaxc : ff;
        if (fdotf < ftol * ftol) return FTOL;
      }
      if (cg) {
        double beta = std::max(0.0, (dot0 - dot1) / gg);
        if ((niter + 1) % nlimit == 0) beta = 0.0;
        gg = dot0;
        launch_min_direction(d, true, beta);
        launch_min_collect(d, true, MinSources());
        wait();
        fdoth = d.min_rec[MIN_FH]; hmaxall = d.min_rec[MIN_HMAXC];
        if (fdoth <= 0.0) {          // not downhill: h = g
          launch_min_h_is_g(d);
          fdoth = dot0; hmaxall = fmaxc;
        }
      } else {
        launch_min_direction(d, false, 0.0);
        fdoth = ff; hmaxall = fmaxc;
      }
      const long step = e.ntimestep;
      const bool due = step == e.endstep || (e.thermo_every > 0 && step % e.thermo_every == 0) ||
                       (!e.dumps.empty() && e.dump_due(step)) || (e.restart_every > 0 && step % e.restart_every == 0);
      if (due) output(false);
    }
    return MAXITER;
  }
};
}  // namespace

const char *Engine::min_stop_string(int n) {      // Min::stopstrings (src/min.cpp:1058-1073)
  static const char *strings[] = {"max iterations", "max force evaluations", "energy tolerance", "force tolerance",
                                  "search direction is not downhill", "linesearch alpha is zero", "forces are zero",
                                  "quadratic factors are zero", "trust region too small", "HFTN minimizer error",
                                  "walltime limit reached", "max iterations with v.f negative"};
  return n >= 0 && n < 12 ? strings[n] : "";
}

// min_style (src/input.cpp:1575-1580, src/update.cpp:389-445): a new Min object, so min_modify's settings start over
void Engine::min_style_command(std::vector<std::string> &arg) {
  if (!box_exist) throw LammpsError("Min_style command before simulation box is defined");
  if (arg.empty()) throw LammpsError("Illegal run_style command");      // (sic, src/update.cpp:391)
  const std::string &s = arg[0];
  static const char *elsewhere[] = {"fire", "fire/old", "quickmin", "hftn", "spin", "spin/cg", "spin/lbfgs"};
  for (const char *o : elsewhere)
    if (s == o) throw LammpsError("MI355X engine: min_style " + s + " is not on the device (cg and sd are)");
  if (s != "cg" && s != "sd") throw LammpsError("Illegal minimize style");
  min_style = s;
  min_dmax = 0.1; min_linestyle = 1; min_normstyle = 0;
  min_other.clear();
}

// Min::modify_params (src/min.cpp:667-751)
void Engine::min_modify_command(std::vector<std::string> &arg) {
  static const char *illegal = "Illegal min_modify command";
  if (arg.empty()) throw LammpsError(illegal);
  size_t i = 0;
  while (i < arg.size()) {
    const std::string &k = arg[i];
    auto value = [&]() -> const std::string & { if (i + 2 > arg.size()) throw LammpsError(illegal); return arg[i + 1]; };
    if (k == "dmax") min_dmax = numeric(value());
    else if (k == "delaystep" || k == "dtgrow" || k == "dtshrink" || k == "alpha0" || k == "alphashrink" || k == "tmax" || k == "tmin" ||
             k == "vdfmax") { numeric(value()); min_other[k] = arg[i + 1]; }
    else if (k == "halfstepback" || k == "initialdelay") {
      if (value() != "yes" && value() != "no") throw LammpsError(illegal);
      min_other[k] = arg[i + 1];
    } else if (k == "integrator") {
      const std::string &v = value();
      if (v != "eulerimplicit" && v != "verlet" && v != "leapfrog" && v != "eulerexplicit") throw LammpsError(illegal);
      min_other[k] = v;
    } else if (k == "line") {
      const std::string &v = value();
      if (v == "backtrack") min_linestyle = 0;
      else if (v == "quadratic") min_linestyle = 1;
      else if (v == "forcezero" || v == "spin_cubic" || v == "spin_none")
        throw LammpsError("MI355X engine: min_modify line " + v + " is not on the device (backtrack and quadratic are)");
      else throw LammpsError(illegal);
    } else if (k == "norm") {
      const std::string &v = value();
      if (v == "two") min_normstyle = 0;
      else if (v == "max") min_normstyle = 1;
      else if (v == "inf") min_normstyle = 2;
      else throw LammpsError(illegal);
    } else throw LammpsError("Illegal fix_modify command");      // (sic, src/min.cpp:747: cg and sd have no keywords of their own)
    i += 2;
  }
}

// Minimize::command
void Engine::minimize(double etol, double ftol, long maxiter, long maxeval) {
  if (!box_exist) throw LammpsError("Minimize command before simulation box is defined");
  if (timeout_forced) return;
  if (etol < 0.0 || ftol < 0.0) throw LammpsError("Illegal minimize command");
  if (ntimestep + maxiter < 0 || maxiter < 0) throw LammpsError("Too many iterations");
  if (world > 1) throw LammpsError("MI355X engine: minimize is not supported on a decomposed handle (run it on one GPU)");
  for (int a = 1; a <= nangletypes && apa > 0 && nangles > 0 && !angle_style_name.empty() && angle_style_name != "none" && angle_style_name != "zero"; a++)
    if (!angtab.style[a]) throw LammpsError("All angle coeffs are not set");
  init();
  begin_run_state();
  beginstep = ntimestep;
  endstep = ntimestep + maxiter;
  // Min::init :181-193: the reneighboring criteria of a minimisation
  const int every0 = neigh_every, delay0 = neigh_delay, check0 = neigh_check;
  if (neigh_every != 1 || neigh_delay != 0 || neigh_check != 1) warning("Using 'neigh_modify every 1 delay 0 check yes' setting during minimization");
  neigh_every = 1; neigh_delay = 0; neigh_check = 1;
  DeviceState &d = *dev;
  const bool partial_before = d.min_partial != nullptr;
  const long waits0 = d.host_waits;
  min_niter = min_neval = min_rebuilds = min_host_waits = 0;
  min_stop = 0; min_alpha = 0.0;
  struct Guard {      // Min::cleanup's share that must also happen when the minimisation ends in an error
    Engine &e; int every, delay, check; bool keep_partial;
    ~Guard() {
      e.neigh_every = every; e.neigh_delay = delay; e.neigh_check = check;
      e.in_run = false;
      e.beginstep = e.endstep = 0;
      try { min_free(*e.dev, !keep_partial); } catch (...) {}
    }
  } guard{*this, every0, delay0, check0, partial_before};
  in_run = true;
  min_alloc(d, true);
  Minimizer m(*this, etol, ftol, maxeval);

  // Min::setup
  say("Setting up " + min_style + " style minimization ...\n  Unit style    : " + units + "\n  Current step  : " + std::to_string(ntimestep) + "\n");
  reneighbor(false, sortfreq > 0);
  neigh_builds = 0;
  lazy_rebuilds = 0;
  steps.reset();
  if (want_ptensor) {
    TypeTables tt{};
    for (int t = 1; t <= ntypes; t++) tt.mass[t] = mass[t];
    ke_tensor(d, tt, m.k6);
  }
  m.evaluate(true);
  m.row.step = ntimestep;
  last_thermo = m.row;
  thermo_log.push_back(last_thermo);
  print_thermo_header();
  print_thermo(last_thermo);
  write_dumps(ntimestep);
  m.ecurrent = m.einitial = m.row.pe;
  min_fnorm2_init = std::sqrt(m.ff);
  min_fnorminf_init = m.fmaxc;

  // Min::run
  for (int k = 0; k < 8; k++) timers[k] = 0.0;
  const double t0 = wall_now();
  run_wall0 = t0;
  const int stop = m.iterate(maxiter);
  long nsteps = maxiter;
  if (stop != MAXITER) {          // :443-463: thermo, every dump and the restart file on the iteration reached
    nsteps = m.niter;
    m.ecurrent = m.energy_force(0);
    m.output(true);
  }
  loop_time = wall_now() - t0;

  // Min::cleanup
  adapt_post_run();
  min_efinal = m.ecurrent;
  min_einitial = m.einitial; min_eprevious = m.eprevious;
  min_fnorm2_final = std::sqrt(m.ff);
  min_fnorminf_final = m.fmaxc;
  min_niter = m.niter; min_neval = m.neval; min_stop = stop; min_alpha = m.alpha_final; min_rebuilds = m.rebuilds;
  dev_edits_at_run = dev_edits;
  min_host_waits = d.host_waits - waits0;

  // Finish::end(1) (src/finish.cpp:122-126, :194-218)
  char buf[512];
  snprintf(buf, sizeof buf, "Loop time of %g on 1 procs for %ld steps with %d atoms\n\n", loop_time, nsteps, natoms);
  say(buf);
  auto g8 = [](double v) { char b[40]; snprintf(b, sizeof b, "%.8g", v); return std::string(b); };
  snprintf(buf, sizeof buf, "\nMinimization stats:\n  Stopping criterion = %s\n  Energy initial, next-to-last, final = \n    %18.15g %18.15g %18.15g\n",
           min_stop_string(stop), min_einitial, min_eprevious, min_efinal);
  std::string mesg = buf;
  mesg += "  Force two-norm initial, final = " + g8(min_fnorm2_init) + " " + g8(min_fnorm2_final) + "\n";
  mesg += "  Force max component initial, final = " + g8(min_fnorminf_init) + " " + g8(min_fnorminf_final) + "\n";
  mesg += "  Final line search alpha, max atom move = " + g8(min_alpha) + " " + g8(min_alpha * min_fnorminf_final) + "\n";
  mesg += "  Iterations, force evaluations = " + std::to_string(min_niter) + " " + std::to_string(min_neval) + "\n";
  say(mesg);
  print_timing_breakdown(nsteps);
  snprintf(buf, sizeof buf, "Neighbor list builds = %ld\nDangerous builds = %ld\n", neigh_builds, m.ndanger);
  say(buf);
}

}  // namespace lmp_le
