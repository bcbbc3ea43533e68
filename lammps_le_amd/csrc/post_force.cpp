// post_force.cpp — PostForce (post_force.h): the one walk over the fixes, the upload, the launches of a phase, the layout of the sums
#include "engine.h"
#include "device.h"

namespace lmp_le {

void PostForce::build(const std::vector<std::unique_ptr<Fix>> &fixes, int natoms) {
  clear();
  forceoptab.stride = natoms + 1;
  int phase = 0;
  bool order_matters[2] = {false, false};     // an addforce / setforce was seen in this phase
  for (auto &f : fixes) {
    if (dynamic_cast<FixLangevin *>(f.get())) phase = 1;
    if (auto *w = dynamic_cast<FixWallRegion *>(f.get())) {
      if (order_matters[phase])
        throw LammpsError("MI355X engine: fix " + f->id + " (wall/region) is defined behind a fix addforce or setforce on the same side of "
                          "fix langevin; define the wall first");
      WallEntry e = w->entry();
      e.after_langevin = phase;
      walltab.w[walltab.n++] = e;
      wall_fixes.push_back(w);
      walls_grouped = walls_grouped || w->groupbit != 1;
    } else if (auto *o = dynamic_cast<FixIndent *>(f.get())) {
      if (order_matters[phase])
        throw LammpsError("MI355X engine: fix " + f->id + " (indent) is defined behind a fix addforce or setforce on the same side of "
                          "fix langevin; define the indenter first");
      if ((int)indent_fixes.size() >= INDENT_MAX) throw LammpsError("internal: more than INDENT_MAX fix indent instances");
      indent_fixes.push_back(o);
      indent_phase.push_back(phase);
      indents_grouped = indents_grouped || o->groupbit != 1;
    } else if (auto *o = dynamic_cast<FixForceOp *>(f.get())) {
      if (forceoptab.n >= FORCEOP_MAX) throw LammpsError("internal: more than FORCEOP_MAX force fixes");
      ForceOpEntry e = o->entry();
      e.phase = phase;
      if (o->kind != FORCEOP_SPRING) order_matters[phase] = true;
      forceoptab.e[forceoptab.n++] = e;
      forceop_fixes.push_back(o);
    } else continue;
    behind = behind || phase == 1;
  }
}

void PostForce::upload(DeviceState &d) {
  d.indent_count = (int)indent_fixes.size();
  if (walltab.n || !indent_fixes.empty()) upload_wall_table(d, walltab);
  if (!indent_fixes.empty()) reserve_indent_partials(d);
  if (forceoptab.n) {      // the origin blocks of the tethers: by tag, whole on every rank
    const double *origins[FORCEOP_MAX];
    for (int k = 0; k < forceoptab.n; k++) origins[k] = forceop_fixes[k]->kind == FORCEOP_SPRING ? forceop_fixes[k]->xorig.data() : nullptr;
    upload_forceop_table(d, forceoptab, origins, forceoptab.stride - 1);
  }
}

void PostForce::run(DeviceState &d, long step, int phase, bool eflag) {
  if (walltab.n) launch_wall(d, walltab, phase, eflag);
  if (!indent_fixes.empty()) {      // the geometry of this force evaluation, once for both phases
    if (phase == 0) indent_now = indent_table();
    launch_indent(d, indent_now, phase, eflag);
  }
  if (forceoptab.n) launch_fixforce(d, forceoptab, phase, forceop_active(step), eflag);
}

// FixIndent::post_force's head for every indenter (the formulas at the engine's ntimestep, the centre remapped), between two launches
IndentTable PostForce::indent_table() const {
  IndentTable t{};
  for (size_t k = 0; k < indent_fixes.size(); k++) {
    IndentEntry e = indent_fixes[k]->entry();
    e.phase = indent_phase[k];
    t.e[t.n++] = e;
  }
  return t;
}

unsigned PostForce::forceop_active(long step) const {
  unsigned m = 0;
  for (int k = 0; k < forceoptab.n; k++) if (step % forceoptab.e[k].every == 0) m |= 1u << k;
  return m;
}

bool PostForce::forceop_sums_due(long step, long endstep, int thermo_every) const {
  for (int k = 0; k < forceoptab.n; k++) {
    const long every = forceoptab.e[k].every;
    if (every <= 1 || step % every) continue;
    long next = endstep;
    if (thermo_every > 0) next = std::min(next, (step / thermo_every + 1) * (long)thermo_every);
    if (next > step && next - step < every) return true;
  }
  return false;
}

void PostForce::reduce(DeviceState &d, double *s) const {
  const int nwall = walltab.n, nops = forceoptab.n, nind = (int)indent_fixes.size();
  if (nwall) reduce_rows(d, d.wall_partial, nwall, s + 16);
  if (nops) reduce_rows(d, d.forceop_partial, nops, s + 16 + 16 * nwall);
  if (nind) reduce_rows(d, d.indent_partial, nind, s + 16 + 16 * (nwall + nops));
}

void PostForce::take_sums(const double *s, long step, double &efix, double vfix[6]) {
  const double *row = s + 16;
  for (FixWallRegion *w : wall_fixes) {
    for (int c = 0; c < 4; c++) w->ewall[c] = row[c];
    for (int c = 0; c < 6; c++) w->virial[c] = row[4 + c];
    if (w->thermo_energy) efix += w->ewall[0];
    if (w->thermo_virial) for (int c = 0; c < 6; c++) vfix[c] += w->virial[c];
    row += 16;
  }
  const unsigned active = forceop_active(step);
  for (size_t k = 0; k < forceop_fixes.size(); k++, row += 16) {
    FixForceOp *o = forceop_fixes[k];
    // (an addforce that skipped this step - `every` - returned before it touched its sums, src/fix_addforce.cpp:243: the rows
    //  of block sums are then those of the last step on which it acted, which forceop_sums_due had evaluated with them)
    //  The six virial terms are different: v_tally runs only on a step that wants the virial, so after a skipped thermo step
    //  the reference's array still holds what the last thermo step on which the fix acted left (:247-248, :292-300)
    const bool acted = (active >> k) & 1u;
    for (int c = 0; c < FORCEOP_COLS; c++) if (c < 4 || acted) o->sums[c] = row[c];
    if (o->thermo_energy) efix += o->compute_scalar();
    if (o->thermo_virial) for (int c = 0; c < 6; c++) vfix[c] += o->sums[4 + c];
  }
  for (FixIndent *o : indent_fixes) {      // FixIndent::compute_scalar / compute_vector; no virial (virial_flag 0)
    for (int c = 0; c < INDENT_COLS; c++) o->indenter[c] = row[c];
    if (o->thermo_energy) efix += o->indenter[0];
    row += 16;
  }
}

void PostForce::unpack_min_record(const double *p, double *s) const {
  const int nrest = 16 * (walltab.n + forceoptab.n);
  for (int k = 0; k < nrest; k++) s[16 + k] = p[k];
  p += nrest;
  for (size_t k = 0; k < indent_fixes.size(); k++)
    for (int c = 0; c < 16; c++) s[16 + nrest + 16 * k + c] = c < INDENT_COLS ? p[INDENT_COLS * k + c] : 0.0;
}

}  // namespace lmp_le
