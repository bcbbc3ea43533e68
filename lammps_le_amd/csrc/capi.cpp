// capi.cpp — extern "C" boundary (include/lammps_le.h): the reference's library.h subset for this path.
// Behaviour follows src/library.cpp; every entry point catches LammpsError and records it
// (the reference does the same when built with LAMMPS_EXCEPTIONS, src/library.cpp BEGIN_CAPTURE/END_CAPTURE).
#include <sys/utsname.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "../../include/lammps_le.h"
#include "comm.h"
#include "device.h"
#include "soft_inl.h"
#include "indent_inl.h"

namespace lmp_le { unsigned dd_halo_mismatches(DeviceState &d); }
using namespace lmp_le;

#define BEGIN_CAPTURE Engine *e = (Engine *)handle; try {
#define END_CAPTURE } catch (const std::exception &ex) { e->last_error = ex.what(); e->has_error = true; \
    if (e->screen) { fprintf(e->screen, "ERROR: %s\n", ex.what()); fflush(e->screen); } \
    if (e->logfile) { fprintf(e->logfile, "ERROR: %s\n", ex.what()); fflush(e->logfile); } }

extern "C" {

void *lammps_open_no_mpi(int argc, char **argv, void **ptr) {
  Engine *e = nullptr;
  try { e = new Engine(argc, argv); } catch (const std::exception &ex) { fprintf(stderr, "LAMMPS Exception: %s\n", ex.what()); }
  if (ptr) *ptr = (void *)e;
  return (void *)e;
}
void lammps_close(void *handle) { delete (Engine *)handle; }

void lammps_file(void *handle, const char *file) { BEGIN_CAPTURE e->file(file); END_CAPTURE }
char *lammps_command(void *handle, const char *cmd) {
  char *result = nullptr;
  BEGIN_CAPTURE result = (char *)e->one(cmd); END_CAPTURE
  return result;
}
void lammps_commands_list(void *handle, int ncmd, const char **cmds) {
  for (int i = 0; i < ncmd; i++) {
    lammps_command(handle, cmds[i]);
    if (((Engine *)handle)->has_error) return;
  }
}
void lammps_commands_string(void *handle, const char *str) {
  std::string s(str), line;
  size_t pos = 0;
  while (pos <= s.size()) {
    size_t nl = s.find('\n', pos);
    line = s.substr(pos, nl == std::string::npos ? std::string::npos : nl - pos);
    lammps_command(handle, line.c_str());
    if (((Engine *)handle)->has_error || nl == std::string::npos) return;
    pos = nl + 1;
  }
}

double lammps_get_natoms(void *handle) { return (double)((Engine *)handle)->natoms; }

double lammps_get_thermo(void *handle, const char *keyword) {
  double val = 0.0;
  BEGIN_CAPTURE
    const ThermoRow &r = e->last_thermo;
    std::string k = keyword;
    bool isint;
    if (k == "step") val = (double)e->ntimestep;
    else if (k.rfind("f_", 0) == 0 || !e->thermo_keyword(r, k, val, isint))
      throw LammpsError("Unknown keyword in thermo_style custom command: " + k);
  END_CAPTURE
  return val;
}

void lammps_extract_box(void *handle, double *boxlo, double *boxhi, double *xy, double *yz, double *xz, int *pflags,
                        int *boxflag) {
  Engine *e = (Engine *)handle;
  for (int d = 0; d < 3; d++) {
    if (boxlo) boxlo[d] = e->box.lo[d];
    if (boxhi) boxhi[d] = e->box.hi[d];
    if (pflags) pflags[d] = 1;
  }
  if (xy) *xy = 0.0;
  if (yz) *yz = 0.0;
  if (xz) *xz = 0.0;
  if (boxflag) *boxflag = 0;
}

int lammps_extract_setting(void *handle, const char *keyword) {
  Engine *e = (Engine *)handle;
  std::string k = keyword;
  if (k == "bigint") return 8;
  if (k == "tagint" || k == "imageint") return 4;
  if (k == "nlocal" || k == "nall") return e->natoms;
  if (k == "ntypes") return e->ntypes;
  if (k == "nbondtypes") return e->nbondtypes;
  if (k == "bond_per_atom") return e->bpa;
  if (k == "angle_per_atom") return e->apa;
  if (k == "nangles") return (int)e->nangles;
  if (k == "nangletypes") return e->nangletypes;
  if (k == "maxspecial") return e->maxspecial;
  if (k == "newton_bond") return 0;
  if (k == "molecule_flag") return e->atom_style != "atomic";
  if (k == "dimension") return 3;
  if (k == "box_exist") return e->box_exist;
  return -1;
}

void *lammps_extract_global(void *handle, const char *name) {
  Engine *e = (Engine *)handle;
  std::string k = name;
  if (k == "dt") return &e->dt;
  if (k == "ntimestep") return &e->ntimestep;
  if (k == "atime") return &e->atime;              // src/library.cpp:1332-1333
  if (k == "atimestep") return &e->atimestep;
  if (k == "boxlo") return e->box.lo;
  if (k == "boxhi") return e->box.hi;
  if (k == "natoms") { e->scratch_scalar = e->natoms; return &e->scratch_scalar; }
  if (k == "nbonds") return &e->nbonds;
  if (k == "ntypes") return &e->ntypes;
  if (k == "boltz") return &e->boltz;
  if (k == "units") return (void *)e->units.c_str();
  return nullptr;
}

void *lammps_extract_atom(void *handle, const char *name) {
  void *result = nullptr;
  BEGIN_CAPTURE
    e->download();
    std::string k = name;
    auto rows = [&](std::vector<double> &a) {
      e->scratch_rows.resize(e->natoms);
      for (int i = 0; i < e->natoms; i++) e->scratch_rows[i] = &a[3 * (size_t)i];
      return (void *)e->scratch_rows.data();
    };
    if (k == "x") result = rows(e->x);
    else if (k == "v") result = rows(e->v);
    else if (k == "f") result = rows(e->f);
    else if (k == "type") result = e->type.data();
    else if (k == "mass") result = e->mass.data();
    else if (k == "id") {
      auto &a = e->scratch_i["id"]; a.resize(e->natoms);
      for (int i = 0; i < e->natoms; i++) a[i] = i + 1;
      result = a.data();
    } else if (k == "mask") {
      auto &a = e->scratch_i["mask"]; a.assign(e->natoms, 1);       // bit 0 = all; further bits = the groups in definition order
      if ((int)e->gmask.size() == e->natoms) for (int i = 0; i < e->natoms; i++) a[i] = e->gmask[i] | 1;
      result = a.data();
    } else if (k == "image") {
      auto &a = e->scratch_i["image"]; a.resize(e->natoms);
      for (int i = 0; i < e->natoms; i++) a[i] = lammps_encode_image_flags(e->image[3 * i], e->image[3 * i + 1], e->image[3 * i + 2]);
      result = a.data();
    } else if (k == "molecule") result = e->molecule.data();
  END_CAPTURE
  return result;
}

void *lammps_extract_fix(void *handle, char *id, int style, int type, int nrow, int /*ncol*/) {
  void *result = nullptr;
  BEGIN_CAPTURE
    Fix *f = e->find_fix(id);
    if (!f) throw LammpsError(std::string("Could not find fix ID ") + id);
    // (the fixes with a global scalar: wall/region, spring/self, addforce, indent)
    const bool scalar = style == 0 && type == 0 && (dynamic_cast<FixWallRegion *>(f) || dynamic_cast<FixSpringSelf *>(f) || dynamic_cast<FixAddForce *>(f) ||
                                                    dynamic_cast<FixIndent *>(f));
    if (!scalar && (style != 0 || type != 1)) throw LammpsError("MI355X engine: only global fix vectors can be extracted");
    if (!scalar && f->size_vector() >= 0 && (nrow < 0 || nrow >= f->size_vector()))
      throw LammpsError("MI355X engine: fix vector is accessed out-of-range");
    double *d = (double *)malloc(sizeof(double));
    *d = scalar ? f->compute_scalar() : f->compute_vector(nrow);
    result = d;
  END_CAPTURE
  return result;
}

static int topo_width(Engine *e, const std::string &k) {
  if (k == "num_bond") return 1;
  if (k == "bond_type" || k == "bond_atom") return e->bpa;
  if (k == "nspecial") return 3;
  if (k == "special") return e->maxspecial;
  if (k == "num_angle") return e->apa > 0 ? 1 : 0;
  if (k == "angle_type" || k == "angle_atom1" || k == "angle_atom2" || k == "angle_atom3") return e->apa;
  return 0;
}

// the whole-system forms, ordered by atom ID (fn: the entry point named in error messages)
static void gather_atoms_impl(Engine *e, const char *fn, const char *name, int type, int count, void *data) {
  e->download();
  std::string k = name;
  int n = e->natoms;
  if (type == 1) {
    std::vector<double> *src = (k == "x") ? &e->x : (k == "v") ? &e->v : (k == "f") ? &e->f : nullptr;
    if (!src || count != 3) throw LammpsError(std::string(fn) + ": unknown property name " + k);
    memcpy(data, src->data(), 3 * (size_t)n * sizeof(double));
  } else {
    int *out = (int *)data;
    if (k == "type" && count == 1) memcpy(out, e->type.data(), n * sizeof(int));
    else if (k == "id" && count == 1) for (int i = 0; i < n; i++) out[i] = i + 1;
    else if (k == "mask" && count == 1) for (int i = 0; i < n; i++) out[i] = (int)e->gmask.size() == n ? (e->gmask[i] | 1) : 1;
    else if (k == "molecule" && count == 1) memcpy(out, e->molecule.data(), n * sizeof(int));
    else if (k == "image" && count == 3) memcpy(out, e->image.data(), 3 * (size_t)n * sizeof(int));
    else if (k == "image" && count == 1)
      for (int i = 0; i < n; i++) out[i] = lammps_encode_image_flags(e->image[3 * i], e->image[3 * i + 1], e->image[3 * i + 2]);
    else if (topo_width(e, k) == count && count > 0) {
      const std::vector<int> &src = (k == "num_bond") ? e->num_bond : (k == "bond_type") ? e->bond_type :
                                    (k == "bond_atom") ? e->bond_atom : (k == "nspecial") ? e->nspecial :
                                    (k == "num_angle") ? e->num_angle : (k == "angle_type") ? e->angle_type :
                                    (k == "angle_atom1") ? e->angle_a1 : (k == "angle_atom2") ? e->angle_a2 :
                                    (k == "angle_atom3") ? e->angle_a3 : e->special;
      memcpy(out, src.data(), (size_t)n * count * sizeof(int));
    } else throw LammpsError(std::string(fn) + ": unknown property name " + k);
  }
}

static void scatter_atoms_impl(Engine *e, const char *fn, const char *name, int type, int count, void *data) {
  e->download();
  std::string k = name;
  int n = e->natoms;
  if (type == 1 && count == 3 && (k == "x" || k == "v" || k == "f")) {
    std::vector<double> &dst = (k == "x") ? e->x : (k == "v") ? e->v : e->f;
    memcpy(dst.data(), data, 3 * (size_t)n * sizeof(double));
  } else if (type == 0 && count == 1 && k == "type") memcpy(e->type.data(), data, n * sizeof(int));
  else if (type == 0 && count == 3 && k == "image") memcpy(e->image.data(), data, 3 * (size_t)n * sizeof(int));
  else throw LammpsError(std::string(fn) + ": unknown property name " + k);
  e->dev_current = false;   // next run re-uploads
}
void lammps_gather_atoms(void *handle, char *name, int type, int count, void *data) {
  BEGIN_CAPTURE gather_atoms_impl(e, "lammps_gather_atoms", name, type, count, data); END_CAPTURE
}
void lammps_scatter_atoms(void *handle, char *name, int type, int count, void *data) {
  BEGIN_CAPTURE scatter_atoms_impl(e, "lammps_scatter_atoms", name, type, count, data); END_CAPTURE
}


// ---- ID-addressed subsets (src/library.cpp:2225-2363 gather_atoms_subset, :2482-2614 scatter_atoms_subset) ----
// While the device holds the newer state, the K requested rows move through kernels_capi.hip and nothing downloads the system;
// otherwise (before the first run, after a whole-system scatter) the host copies in tag order are the state and serve the call.
static bool device_is_newer(Engine *e) { return e->dev && e->dev_current && e->dev->pos && !e->host_current; }

static void check_ids(Engine *e, const char *fn, int ndata, const int *ids) {
  if (ndata < 0) throw LammpsError(std::string(fn) + ": invalid number of atoms");
  for (int i = 0; i < ndata; i++)
    if (ids[i] < 1 || ids[i] > e->natoms) throw LammpsError(std::string(fn) + ": unknown atom ID " + std::to_string(ids[i]));
}

// the int table a subset row of a topology name comes from (host copy or device table, both row t-1 / t of width count)
static const std::vector<int> *host_topo(Engine *e, const std::string &k) {
  return (k == "num_bond") ? &e->num_bond : (k == "bond_type") ? &e->bond_type : (k == "bond_atom") ? &e->bond_atom :
         (k == "nspecial") ? &e->nspecial : (k == "special") ? &e->special : (k == "num_angle") ? &e->num_angle :
         (k == "angle_type") ? &e->angle_type : (k == "angle_atom1") ? &e->angle_a1 : (k == "angle_atom2") ? &e->angle_a2 :
         (k == "angle_atom3") ? &e->angle_a3 : nullptr;
}
static const int *dev_topo(DeviceState &d, const std::string &k) {
  return (k == "num_bond") ? d.num_bond : (k == "bond_type") ? d.bond_type : (k == "bond_atom") ? d.bond_atom :
         (k == "nspecial") ? d.nspecial : (k == "special") ? d.special : (k == "num_angle") ? d.num_angle :
         (k == "angle_type") ? d.angle_type : (k == "angle_atom1") ? d.angle_a1 : (k == "angle_atom2") ? d.angle_a2 :
         (k == "angle_atom3") ? d.angle_a3 : (k == "type") ? d.type_t : nullptr;
}

static void gather_subset_impl(Engine *e, const char *fn, const char *name, int type, int count, int ndata, const int *ids,
                               void *data) {
  const std::string k = name;
  const bool dbl3 = type == 1 && count == 3 && (k == "x" || k == "v" || k == "f");
  const bool img = type == 0 && k == "image" && (count == 1 || count == 3);
  const bool host_only = type == 0 && count == 1 && (k == "id" || k == "mask" || k == "molecule");   // static per atom
  const bool tagtab = type == 0 && ((k == "type" && count == 1) || (topo_width(e, k) == count && count > 0));
  if (!dbl3 && !img && !host_only && !tagtab) throw LammpsError(std::string(fn) + ": unknown property name " + k);
  check_ids(e, fn, ndata, ids);
  const int K = ndata;
  if (K == 0) return;
  if (host_only || !device_is_newer(e)) {
    double *od = (double *)data;
    int *oi = (int *)data;
    const int n = e->natoms;
    for (int r = 0; r < K; r++) {
      const int i = ids[r] - 1;
      if (dbl3) {
        const std::vector<double> &src = (k == "x") ? e->x : (k == "v") ? e->v : e->f;
        for (int c = 0; c < 3; c++) od[3 * (size_t)r + c] = src[3 * (size_t)i + c];
      } else if (k == "id") oi[r] = i + 1;
      else if (k == "mask") oi[r] = (int)e->gmask.size() == n ? (e->gmask[i] | 1) : 1;
      else if (k == "molecule") oi[r] = e->molecule[i];
      else if (k == "type") oi[r] = e->type[i];
      else if (img && count == 3) for (int c = 0; c < 3; c++) oi[3 * (size_t)r + c] = e->image[3 * (size_t)i + c];
      else if (img) oi[r] = lammps_encode_image_flags(e->image[3 * i], e->image[3 * i + 1], e->image[3 * i + 2]);
      else {
        const std::vector<int> &src = *host_topo(e, k);
        for (int c = 0; c < count; c++) oi[(size_t)r * count + c] = src[(size_t)i * count + c];
      }
    }
    return;
  }
  DeviceState &d = *e->dev;
  const int prop = dbl3 ? (k == "x" ? SUBSET_X : SUBSET_V3) : img ? (count == 3 ? SUBSET_IMG3 : SUBSET_IMG1) : SUBSET_TAGTAB;
  const size_t rowb = (size_t)count * (dbl3 ? sizeof(double) : sizeof(int));
  std::vector<int> found(K);
  std::vector<char> rows((size_t)K * rowb);
  subset_gather(d, prop, k == "f" ? 1 : 0, tagtab ? dev_topo(d, k) : nullptr, count, K, ids, rows.data(), found.data());
  if (d.dd && prop != SUBSET_TAGTAB) {
    // every rank packed the rows it owns: one K-row all-gather completes them (found column included)
    const int W = e->world;
    const size_t per = (size_t)K * rowb + (size_t)K * sizeof(int);
    std::vector<char> mine(per), all(per * W);
    memcpy(mine.data(), rows.data(), (size_t)K * rowb);
    memcpy(mine.data() + (size_t)K * rowb, found.data(), (size_t)K * sizeof(int));
    e->comm->allgather_host(mine.data(), all.data(), per);
    e->subset_comm_bytes += (double)per;
    for (int r = 0; r < K; r++) {
      int owner = -1;
      for (int q = 0; q < W && owner < 0; q++) {
        int fl;
        memcpy(&fl, all.data() + per * q + (size_t)K * rowb + (size_t)r * sizeof(int), sizeof(int));
        if (fl) owner = q;
      }
      if (owner < 0) throw LammpsError(std::string(fn) + ": atom ID " + std::to_string(ids[r]) + " is owned by no rank");
      memcpy((char *)data + (size_t)r * rowb, all.data() + per * owner + (size_t)r * rowb, rowb);
    }
    return;
  }
  for (int r = 0; r < K; r++)
    if (!found[r]) throw LammpsError(std::string(fn) + ": atom ID " + std::to_string(ids[r]) + " has no slot on the device");
  memcpy(data, rows.data(), (size_t)K * rowb);
}

static bool fixes_on_groups(Engine *e) {
  for (auto &f : e->fixes) if (f->groupbit != 1) return true;
  return false;
}

static void scatter_subset_impl(Engine *e, const char *fn, const char *name, int type, int count, int ndata, const int *ids,
                                void *data) {
  const std::string k = name;
  const bool dbl3 = type == 1 && count == 3 && (k == "x" || k == "v" || k == "f");
  const bool img = type == 0 && k == "image" && (count == 1 || count == 3);
  const bool typ = type == 0 && count == 1 && k == "type";
  if (!dbl3 && !img && !typ) throw LammpsError(std::string(fn) + ": unknown property name " + k);
  check_ids(e, fn, ndata, ids);
  // a type outside 1 .. ntypes: the reference writes it and fails later in its pair style; here it would index the per-type
  // tables out of range on the device, so it is refused before anything is written, on the host copies and on the device alike
  // (every row sent is read, ahead of the last-row-wins of a repeated ID: an invalid row that a later valid one would have
  // overwritten is refused too, where the reference would end with the valid value - stricter, never less safe)
  if (typ)
    for (int r = 0; r < ndata; r++) {
      const int t = ((const int *)data)[r];
      if (t < 1 || t > e->ntypes)
        throw LammpsError(std::string(fn) + ": invalid atom type " + std::to_string(t) + " for atom ID " + std::to_string(ids[r]));
    }
  // a repeated ID takes its last row, as the reference's sequential loop leaves it
  const size_t rowb = (size_t)count * (dbl3 ? sizeof(double) : sizeof(int));
  std::vector<int> uid;
  std::vector<char> urows;
  {
    std::vector<char> seen((size_t)e->natoms + 1, 0);
    for (int r = ndata - 1; r >= 0; r--) {
      if (seen[ids[r]]) continue;
      seen[ids[r]] = 1;
      uid.push_back(ids[r]);
      urows.insert(urows.end(), (const char *)data + (size_t)r * rowb, (const char *)data + (size_t)(r + 1) * rowb);
    }
  }
  const int K = (int)uid.size();
  if (K == 0) return;
  auto apply_host = [&]() {
    for (int r = 0; r < K; r++) {
      const int i = uid[r] - 1;
      const char *src = urows.data() + (size_t)r * rowb;
      if (dbl3) {
        std::vector<double> &dst = (k == "x") ? e->x : (k == "v") ? e->v : e->f;
        memcpy(&dst[3 * (size_t)i], src, rowb);
      } else if (typ) memcpy(&e->type[i], src, sizeof(int));
      else if (count == 3) memcpy(&e->image[3 * (size_t)i], src, rowb);
      else { int im; memcpy(&im, src, sizeof(int)); lammps_decode_image_flags(im, &e->image[3 * (size_t)i]); }
    }
  };
  if (!(e->dev && e->dev_current && e->dev->pos)) { apply_host(); return; }   // the host copies are the state
  DeviceState &d = *e->dev;
  // what cannot stay on the device takes the whole-system path (download, edit, re-upload at the next run):
  //  - a new type for a bead while some fix acts on a group (its members' draws and masks travel with an upload);
  //  - decomposed runs: moved beads that land beyond a neighbouring slab, or more of them than k_dd_leave can migrate
  bool fallback = typ && fixes_on_groups(e);
  if (d.dd && k == "x") {
    std::vector<int> found(K);
    std::vector<double> cur(3 * (size_t)K);
    subset_gather(d, SUBSET_X, 0, nullptr, 3, K, uid.data(), cur.data(), found.data());
    const int W = e->world, me = e->rank;
    long leave = 0, far = 0;
    for (int r = 0; r < K; r++) {
      if (!found[r]) continue;
      double z;
      memcpy(&z, urows.data() + (size_t)r * rowb + 2 * sizeof(double), sizeof(double));
      if (z < e->box.lo[2]) z += e->box.prd[2];          // the owner expression of Engine::upload / k_dd_classify
      if (z >= e->box.hi[2]) z -= e->box.prd[2];
      int owner = (int)((z - e->box.lo[2]) / (e->box.prd[2] / W));
      owner = std::min(std::max(owner, 0), W - 1);
      if (owner == me) continue;
      leave++;
      if (owner != (me + 1) % W && owner != (me + W - 1) % W) far++;
    }
    const long migcap = (long)d.npad / 4;                  // kernels_dd.hip rebuild_migrate: slots per direction
    fallback = e->comm->allreduce_host_max((far > 0 || leave > migcap / 2) ? 1L : 0L) != 0;
    e->subset_comm_bytes += (double)sizeof(long);
  }
  if (fallback) {
    e->download();
    apply_host();
    e->dev_current = false;    // next run re-uploads
    return;
  }
  const int prop = dbl3 ? (k == "x" ? SUBSET_X : SUBSET_V3) : typ ? SUBSET_TYPE : (count == 3 ? SUBSET_IMG3 : SUBSET_IMG1);
  // (before the rows land: d.pos may have to leave the buffer that records the build - a new type is written into pos.w)
  if (k == "x") note_positions_replaced(d);
  else if (typ) detach_positions(d);
  subset_scatter(d, prop, k == "f" ? 1 : 0, count, K, uid.data(), urows.data());
  e->dev_edits++;          // (what was computed from the device state at this timestep is no longer current)
  if (e->host_current) apply_host();       // keep a current host copy current
}

// local order of the engine's one-rank reference (crank): order[r] = tag - 1 of the atom with local index r
static std::vector<int> local_order(Engine *e) {
  const int n = e->natoms;
  std::vector<int> cr(e->crank.begin(), e->crank.begin() + n);
  if (e->crank_on_device && e->dev && e->dev->crank) {
    std::vector<int> c((size_t)n + 2);
    HIP_CHECK(hipMemcpy(c.data(), e->dev->crank, c.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++) cr[i] = c[i + 1];
  }
  std::vector<int> order(n, -1);
  for (int i = 0; i < n; i++) {
    if (cr[i] < 0 || cr[i] >= n || order[cr[i]] >= 0) throw LammpsError("internal: local order is not a permutation");
    order[cr[i]] = i;
  }
  return order;
}

// gather_atoms_concat / gather_concat (src/library.cpp:2076-2224, :2834-3075): every atom, in local order
static void gather_concat_impl(Engine *e, const char *fn, const char *name, int type, int count, void *data) {
  const int n = e->natoms;
  const size_t rowb = (size_t)count * (type == 1 ? sizeof(double) : sizeof(int));
  std::vector<char> bytag((size_t)n * rowb);
  gather_atoms_impl(e, fn, name, type, count, bytag.data());
  const std::vector<int> order = local_order(e);
  for (int r = 0; r < n; r++) memcpy((char *)data + (size_t)r * rowb, bytag.data() + (size_t)order[r] * rowb, rowb);
}

// lammps_gather / lammps_scatter and their subset forms (src/library.cpp:2615-3509): per-atom properties only - fix,
// compute and custom per-atom names (f_, c_, d_, i_) have nothing per-atom to return on this path
static void no_custom(const char *fn, const char *name) {
  const std::string k = name;
  if (k.rfind("f_", 0) == 0 || k.rfind("c_", 0) == 0 || k.rfind("d_", 0) == 0 || k.rfind("i_", 0) == 0)
    throw LammpsError(std::string(fn) + ": unknown property name " + k);
}

void lammps_gather_atoms_subset(void *handle, char *name, int type, int count, int ndata, int *ids, void *data) {
  BEGIN_CAPTURE gather_subset_impl(e, "lammps_gather_atoms_subset", name, type, count, ndata, ids, data); END_CAPTURE
}
void lammps_scatter_atoms_subset(void *handle, char *name, int type, int count, int ndata, int *ids, void *data) {
  BEGIN_CAPTURE scatter_subset_impl(e, "lammps_scatter_atoms_subset", name, type, count, ndata, ids, data); END_CAPTURE
}
void lammps_gather_atoms_concat(void *handle, char *name, int type, int count, void *data) {
  BEGIN_CAPTURE gather_concat_impl(e, "lammps_gather_atoms_concat", name, type, count, data); END_CAPTURE
}
void lammps_gather(void *handle, char *name, int type, int count, void *data) {
  BEGIN_CAPTURE no_custom("lammps_gather", name); gather_atoms_impl(e, "lammps_gather", name, type, count, data); END_CAPTURE
}
void lammps_scatter(void *handle, char *name, int type, int count, void *data) {
  BEGIN_CAPTURE no_custom("lammps_scatter", name); scatter_atoms_impl(e, "lammps_scatter", name, type, count, data); END_CAPTURE
}
void lammps_gather_concat(void *handle, char *name, int type, int count, void *data) {
  BEGIN_CAPTURE no_custom("lammps_gather_concat", name); gather_concat_impl(e, "lammps_gather_concat", name, type, count, data); END_CAPTURE
}
void lammps_gather_subset(void *handle, char *name, int type, int count, int ndata, int *ids, void *data) {
  BEGIN_CAPTURE
    no_custom("lammps_gather_subset", name);
    gather_subset_impl(e, "lammps_gather_subset", name, type, count, ndata, ids, data);
  END_CAPTURE
}
void lammps_scatter_subset(void *handle, char *name, int type, int count, int ndata, int *ids, void *data) {
  BEGIN_CAPTURE
    no_custom("lammps_scatter_subset", name);
    scatter_subset_impl(e, "lammps_scatter_subset", name, type, count, ndata, ids, data);
  END_CAPTURE
}

// ---- computes (src/library.cpp:1555-1640).  The thermo computes the reference creates with every instance
// (thermo_temp, thermo_pe, thermo_press; src/output.cpp) take their values from the thermo evaluation of the current step -
// the device reductions thermo runs - and compute property/local from the bond tables ----
enum { LMP_STYLE_GLOBAL = 0, LMP_STYLE_ATOM = 1, LMP_STYLE_LOCAL = 2 };
enum { LMP_TYPE_SCALAR = 0, LMP_TYPE_VECTOR = 1, LMP_TYPE_ARRAY = 2, LMP_SIZE_VECTOR = 3, LMP_SIZE_ROWS = 4, LMP_SIZE_COLS = 5 };

// sum(m v_i v_j) over all atoms, order xx yy zz xy xz yz (compute temp's vector before the mvv2e factor)
static void ke_tensor_now(Engine *e, double k6[6]) {
  if (e->dev && e->dev_current && e->dev->pos) {      // the device holds the state (possibly the host as well)
    TypeTables tt{};
    for (int t = 1; t <= e->ntypes; t++) tt.mass[t] = e->mass[t];
    ke_tensor(*e->dev, tt, k6);
    if (e->world > 1) e->comm->allreduce_host_sum(k6, 6);
    return;
  }
  for (int c = 0; c < 6; c++) k6[c] = 0.0;
  for (int i = 0; i < e->natoms; i++) {
    const double m = e->mass[e->type[i]], *v = &e->v[3 * (size_t)i];
    k6[0] += m * v[0] * v[0]; k6[1] += m * v[1] * v[1]; k6[2] += m * v[2] * v[2];
    k6[3] += m * v[0] * v[1]; k6[4] += m * v[0] * v[2]; k6[5] += m * v[1] * v[2];
  }
}

void *lammps_extract_compute(void *handle, char *id, int style, int type) {
  void *result = nullptr;
  BEGIN_CAPTURE
    const std::string c = id;
    const bool thermo_c = c == "thermo_temp" || c == "thermo_pe" || c == "thermo_press";
    if (!thermo_c && !e->computes_local.count(c)) return nullptr;
    Engine::ComputeCache &cc = e->compute_cache[c];
    const bool fresh = cc.invoked == e->ntimestep && cc.stamp == e->thermo_log.size() && cc.edits == e->dev_edits;
    if (thermo_c) {
      if (style != LMP_STYLE_GLOBAL) return nullptr;                         // no per-atom / local data
      if (type == LMP_TYPE_ARRAY || type == LMP_SIZE_ROWS || type == LMP_SIZE_COLS) return nullptr;   // no array_flag
      if (c == "thermo_pe" && type != LMP_TYPE_SCALAR) return nullptr;       // compute pe: scalar only
      if (!fresh) {
        // energies and the virial exist for a step whose forces were computed with energy: the thermo row of this step
        const ThermoRow &r = e->last_thermo;
        const bool tallied = !e->thermo_log.empty() && r.step == e->ntimestep;
        const double dof = 3.0 * e->natoms - 3.0;
        const double vol = e->box.prd[0] * e->box.prd[1] * e->box.prd[2];
        double k6[6];
        if (c == "thermo_pe") {
          if (!tallied) throw LammpsError("Energy was not tallied on needed timestep");   // src/compute_pe.cpp
          cc.scalar = r.evdwl + (r.ebond + r.eangle);                       // compute pe is not normalized by natoms
        } else if (c == "thermo_temp") {
          ke_tensor_now(e, k6);
          cc.vector.assign(6, 0.0);
          for (int q = 0; q < 6; q++) cc.vector[q] = k6[q] * e->mvv2e;       // src/compute_temp.cpp compute_vector
          cc.scalar = tallied ? r.temp : (dof > 0 ? (k6[0] + k6[1] + k6[2]) * e->mvv2e / (dof * e->boltz) : 0.0);
        } else {
          if (!tallied) throw LammpsError("Virial was not tallied on needed timestep");   // src/compute_pressure.cpp
          cc.scalar = r.press;
          cc.vector.assign(6, 0.0);
          if (r.has_ptensor) for (int q = 0; q < 6; q++) cc.vector[q] = r.ptensor[q];
          else {
            ke_tensor_now(e, k6);     // the expression of Engine::eval_thermo (src/compute_pressure.cpp:244-290)
            for (int q = 0; q < 6; q++) cc.vector[q] = (k6[q] * e->mvv2e + r.virial[q]) / vol * e->nktv2p;
          }
        }
        cc.size_vector = (int)cc.vector.size();
        cc.invoked = e->ntimestep;
        cc.stamp = e->thermo_log.size();
        cc.edits = e->dev_edits;
      }
      if (type == LMP_TYPE_SCALAR) result = &cc.scalar;
      else if (type == LMP_TYPE_VECTOR) result = cc.vector.data();
      else if (type == LMP_SIZE_VECTOR) result = &cc.size_vector;
      return result;
    }
    // compute property/local (btype batom1 batom2): one row per bond, listed once from the lower ID, both atoms in the
    // compute's group (src/compute_property_local.cpp:420-480; the rows dump local writes)
    if (style != LMP_STYLE_LOCAL) return nullptr;
    const Engine::LocalCompute &lc = e->computes_local.at(c);
    if (lc.kind != Engine::LOCAL_BOND) {
      // pair rows: from the device list, shared with every compute of the same kind and group (Engine::pair_rows; nothing is
      // downloaded).  Asked when the list cannot serve, the call sets the error and answers NULL
      const std::vector<std::string> &attrs = lc.attrs;
      const Engine::PairRows &R = e->pair_rows(lc);
      if (!fresh) {
        const int nc = (int)attrs.size();
        std::vector<int> col(nc);
        for (int k = 0; k < nc; k++) col[k] = Engine::pair_row_column(attrs[k]);
        cc.vector.resize((size_t)R.nrows * nc);
        for (long r = 0; r < R.nrows; r++)
          for (int k = 0; k < nc; k++) cc.vector[(size_t)r * nc + k] = Engine::pair_row_value(R, r, col[k]);
        cc.size_rows = (int)R.nrows;
        cc.size_cols = nc > 1 ? nc : 0;
        cc.rows.resize(cc.size_rows);
        for (int r = 0; r < cc.size_rows; r++) cc.rows[r] = cc.vector.data() + (size_t)r * nc;
        cc.invoked = e->ntimestep;
        cc.stamp = e->thermo_log.size();
        cc.edits = e->dev_edits;
      }
    } else if (!fresh) {
      e->download();
      const std::vector<std::string> &attrs = lc.attrs;
      const int bit = lc.bit;
      auto member = [&](int i) { return bit == 1 || (!e->gmask.empty() && (e->gmask[i] & bit)); };
      const int nc = (int)attrs.size();
      cc.vector.clear();
      for (int i = 0; i < e->natoms; i++)
        for (int m = 0; m < e->num_bond[i]; m++) {
          const int bt = e->bond_type[(size_t)i * e->bpa + m], j = e->bond_atom[(size_t)i * e->bpa + m];
          if (bt == 0 || i + 1 > j || !member(i) || !member(j - 1)) continue;
          for (auto &a : attrs) cc.vector.push_back(a == "btype" ? bt : a == "batom1" ? i + 1 : j);
        }
      cc.size_rows = nc ? (int)(cc.vector.size() / nc) : 0;
      cc.size_cols = nc > 1 ? nc : 0;                  // one attribute: vector_local, size_local_cols = 0
      cc.rows.resize(cc.size_rows);
      for (int r = 0; r < cc.size_rows; r++) cc.rows[r] = cc.vector.data() + (size_t)r * nc;
      cc.invoked = e->ntimestep;
      cc.stamp = e->thermo_log.size();
      cc.edits = e->dev_edits;
    }
    if (type == LMP_TYPE_SCALAR || type == LMP_SIZE_ROWS) result = &cc.size_rows;
    else if (type == LMP_SIZE_COLS) result = &cc.size_cols;
    else if (type == LMP_TYPE_VECTOR && cc.size_cols == 0) result = cc.vector.data();
    else if (type == LMP_TYPE_ARRAY && cc.size_cols > 0) result = cc.rows.data();
  END_CAPTURE
  return result;
}

// ---- variables (src/library.cpp:1859-1940) ----
void *lammps_extract_variable(void *handle, char *name, char * /*group*/) {
  void *result = nullptr;
  BEGIN_CAPTURE
    auto it = e->variables.find(name);
    if (it == e->variables.end()) return nullptr;
    auto vi = e->var_info.find(name);
    if (vi != e->var_info.end() && vi->second.style == "equal") {
      double *d = (double *)malloc(sizeof(double));       // released by the caller with lammps_free
      *d = e->evaluate(it->second);
      result = d;
    } else result = (void *)it->second.c_str();           // index / loop / string (and -var): borrowed
  END_CAPTURE
  return result;
}
// the style of a variable as the later library.h's lammps_extract_variable_datatype reports it: LMP_VAR_EQUAL (0) or
// LMP_VAR_STRING (3, index / loop / string), -1 if there is no such variable; tells a caller which pointer to expect
int lammps_extract_variable_datatype(void *handle, const char *name) {
  Engine *e = (Engine *)handle;
  if (!e->variables.count(name)) return -1;
  auto vi = e->var_info.find(name);
  return (vi != e->var_info.end() && vi->second.style == "equal") ? 0 : 3;
}
int lammps_set_variable(void *handle, char *name, char *str) {
  int err = -1;
  BEGIN_CAPTURE
    auto vi = e->var_info.find(name);                     // Variable::set_string: string style only
    if (vi != e->var_info.end() && vi->second.style == "string") {
      vi->second.values = {str};
      e->variables[name] = str;
      err = 0;
    }
  END_CAPTURE
  return err;
}

// ---- introspection (src/library.cpp:973, :1407, :4241-4500) ----
enum { LAMMPS_INT = 0, LAMMPS_INT_2D = 1, LAMMPS_DOUBLE = 2, LAMMPS_DOUBLE_2D = 3, LAMMPS_INT64 = 4, LAMMPS_STRING = 6 };
int lammps_extract_global_datatype(void *, const char *name) {
  const std::string k = name;
  if (k == "dt" || k == "atime" || k == "boxlo" || k == "boxhi" || k == "boltz") return LAMMPS_DOUBLE;
  if (k == "ntimestep" || k == "atimestep" || k == "natoms" || k == "nbonds") return LAMMPS_INT64;
  if (k == "ntypes") return LAMMPS_INT;
  if (k == "units") return LAMMPS_STRING;
  return -1;
}
int lammps_extract_atom_datatype(void *, const char *name) {
  const std::string k = name;
  if (k == "x" || k == "v" || k == "f") return LAMMPS_DOUBLE_2D;
  if (k == "mass") return LAMMPS_DOUBLE;
  if (k == "type" || k == "id" || k == "mask" || k == "image" || k == "molecule") return LAMMPS_INT;
  return -1;
}

// styles: the ones lammps_has_style knows, in this order
static const std::vector<std::pair<std::string, std::vector<std::string>>> &style_table() {
  static const std::vector<std::pair<std::string, std::vector<std::string>>> t = {
      {"atom", {"angle", "atomic", "bond", "full", "molecular"}},
      {"bond", {"fene", "harmonic", "hybrid", "none", "zero"}},
      {"compute", {"pair/local", "property/local"}},
      {"dump", {"atom", "custom", "dcd", "local"}},
      {"fix", {"adapt", "addforce", "bond/break", "bond/create", "ex_load", "ex_unload", "extrusion", "indent", "langevin", "nve", "setforce", "spring/self", "wall/region"}},
      {"pair", {"lj/cut", "none", "soft", "zero"}},
  };
  return t;
}
static const std::vector<std::string> *styles_of(const char *category) {
  for (auto &c : style_table()) if (c.first == category) return &c.second;
  return nullptr;
}
int lammps_style_count(void *, const char *category) {
  const std::vector<std::string> *s = styles_of(category);
  return s ? (int)s->size() : 0;
}
int lammps_style_name(void *, const char *category, int idx, char *buffer, int buf_size) {
  const std::vector<std::string> *s = styles_of(category);
  if (!s || idx < 0 || idx >= (int)s->size()) { if (buf_size > 0) buffer[0] = '\0'; return 0; }
  snprintf(buffer, buf_size, "%s", (*s)[idx].c_str());
  return 1;
}

// IDs by category (src/library.cpp:4348-4500): compute, dump, fix, group, molecule, region, variable
static std::vector<std::string> ids_of(Engine *e, const std::string &c) {
  std::vector<std::string> out;
  if (c == "compute") {
    out = {"thermo_temp", "thermo_press", "thermo_pe"};        // created with every instance (src/output.cpp:60-80)
    for (auto &kv : e->computes_local) out.push_back(kv.first);
  } else if (c == "dump") for (auto &d : e->dumps) out.push_back(d.id);
  else if (c == "fix") for (auto &f : e->fixes) out.push_back(f->id);
  else if (c == "group") { for (auto &g : e->group_names) if (!g.empty()) out.push_back(g); }
  else if (c == "region") for (auto &kv : e->regions) out.push_back(kv.first);
  else if (c == "variable") for (auto &kv : e->variables) out.push_back(kv.first);
  return out;                                                   // molecule: this path has no molecule templates
}
int lammps_has_id(void *handle, const char *category, const char *name) {
  for (auto &s : ids_of((Engine *)handle, category)) if (s == name) return 1;
  return 0;
}
int lammps_id_count(void *handle, const char *category) { return (int)ids_of((Engine *)handle, category).size(); }
int lammps_id_name(void *handle, const char *category, int idx, char *buffer, int buf_size) {
  const std::vector<std::string> ids = ids_of((Engine *)handle, category);
  if (idx < 0 || idx >= (int)ids.size()) { if (buf_size > 0) buffer[0] = '\0'; return 0; }
  snprintf(buffer, buf_size, "%s", ids[idx].c_str());
  return 1;
}

// the packages of the reference build this engine stands for (SURVEY: MOLECULE, MC, MISC, USER-LE)
int lammps_config_package_name(int idx, char *buffer, int buf_size) {
  static const char *pkgs[] = {"MC", "MISC", "MOLECULE", "USER-LE"};
  if (idx < 0 || idx >= 4) { if (buf_size > 0) buffer[0] = '\0'; return 0; }
  snprintf(buffer, buf_size, "%s", pkgs[idx]);
  return 1;
}
// src/library.cpp:4063-4072 (Info::get_os_info + get_compiler_info): operating system, then the compiler
void lammps_get_os_info(char *buffer, int buf_size) {
  if (buf_size <= 0) return;
  struct utsname u;
  std::string txt = "unknown";
  if (uname(&u) == 0) txt = std::string(u.sysname) + " \"" + u.release + "\" " + u.version + " " + u.machine;
  txt += "\n";
#if defined(__clang_version__)
  txt += std::string("Clang C++ ") + __clang_version__;
#else
  txt += "C++";
#endif
  txt += " with OpenMP not enabled\n";
  snprintf(buffer, buf_size, "%s", txt.c_str());
}
int lammps_get_mpi_comm(void *) { return -1; }   // no MPI on this path (src/library.cpp:780-790 without MPI)

// src/library.cpp:691-720: a new orthogonal box; the device copies are re-uploaded at the next run
void lammps_reset_box(void *handle, double *boxlo, double *boxhi, double /*xy*/, double /*yz*/, double /*xz*/) {
  BEGIN_CAPTURE
    if (!e->box_exist) { e->warning("Calling lammps_reset_box without a box"); return; }
    e->download();
    for (int k = 0; k < 3; k++) {
      e->box.lo[k] = boxlo[k]; e->box.hi[k] = boxhi[k];
      e->box.prd[k] = e->box.hi[k] - e->box.lo[k];
      e->box.half[k] = 0.5 * e->box.prd[k];
      e->box.iprd[k] = 1.0 / e->box.prd[k];
    }
    e->dev_current = false;
  END_CAPTURE
}

// Timer::force_timeout (src/timer.h): the current run ends at the next step boundary, later runs do nothing.  A caller of
// this single-threaded engine is never inside a run when it calls this, so it is the next run that ends (at once)
void lammps_force_timeout(void *handle) { ((Engine *)handle)->timeout_forced = true; }

// ---- out of scope, exported with an explicit error (no fake data) ----
// neighbor lists (src/library.cpp:3869-4060): one GPU has no ghost atoms and the lists are stored by cell slot, so the
// reference's list indices have no meaning here
static void no_neighlist(Engine *e) {
  e->last_error = "neighbor list access is not supported";
  e->has_error = true;
}
int lammps_find_pair_neighlist(void *handle, char *, int, int, int) { no_neighlist((Engine *)handle); return -1; }
int lammps_find_fix_neighlist(void *handle, char *, int) { no_neighlist((Engine *)handle); return -1; }
int lammps_find_compute_neighlist(void *handle, char *, int) { no_neighlist((Engine *)handle); return -1; }
int lammps_neighlist_num_elements(void *handle, int) { no_neighlist((Engine *)handle); return 0; }
void lammps_neighlist_element_neighbors(void *handle, int, int, int *iatom, int *numneigh, int **neighbors) {
  no_neighlist((Engine *)handle);
  if (iatom) *iatom = -1;
  if (numneigh) *numneigh = 0;
  if (neighbors) *neighbors = nullptr;
}
// fix external (src/library.cpp:4578-4650): there is no such fix style here, so no fix ID is ever one of it
static void no_fix_external(Engine *e, const char *id) {
  const std::string msg = e->find_fix(id ? id : "") ? std::string("Fix '") + id + "' is not of style external!"
                                                    : std::string("Can not find fix with ID '") + (id ? id : "") + "'!";
  e->last_error = msg;
  e->has_error = true;
}
void lammps_set_fix_external_callback(void *handle, char *id, void *, void *) { no_fix_external((Engine *)handle, id); }
void lammps_fix_external_set_energy_global(void *handle, char *id, double) { no_fix_external((Engine *)handle, id); }
void lammps_fix_external_set_virial_global(void *handle, char *id, double *) { no_fix_external((Engine *)handle, id); }

// src/library.cpp:163-200: the MPI_Comm argument of an MPI-less (STUBS) build is an int and means nothing here
void *lammps_open(int argc, char **argv, int /*comm*/, void **ptr) { return lammps_open_no_mpi(argc, argv, ptr); }

int lammps_version(void *) { return 20201029; }
/* src/library.cpp lammps_encode_image_flags: 10 bits per dimension, offset 512 (LAMMPS_SMALLBIG) */
int lammps_encode_image_flags(int ix, int iy, int iz) {
  return ((ix + 512) & 1023) | (((iy + 512) & 1023) << 10) | (((iz + 512) & 1023) << 20);
}
void lammps_decode_image_flags(int image, int *flags) {
  flags[0] = (image & 1023) - 512;
  flags[1] = ((image >> 10) & 1023) - 512;
  flags[2] = (image >> 20) - 512;
}
void lammps_free(void *ptr) { free(ptr); }
int lammps_is_running(void *) { return 0; }
int lammps_has_error(void *handle) { return ((Engine *)handle)->has_error ? 1 : 0; }
int lammps_get_last_error_message(void *handle, char *buffer, int buf_size) {
  Engine *e = (Engine *)handle;
  if (!e->has_error) { if (buf_size > 0) buffer[0] = '\0'; return 0; }
  snprintf(buffer, buf_size, "%s", e->last_error.c_str());
  e->has_error = false;
  e->last_error.clear();
  return 1;   // 1 = normal (recoverable) error, as ERROR_NORMAL in src/library.cpp
}
int lammps_config_has_exceptions(void) { return 1; }
int lammps_has_style(void *, const char *category, const char *name) {
  const std::vector<std::string> *s = styles_of(category);
  if (s) for (auto &x : *s) if (x == name) return 1;
  return 0;
}

// every thermo line the engine has printed since it was opened, as numbers: rows of 7 doubles (step, temp, epair, emol,
// etotal, press, bonds).  Returns the number of rows there are; writes at most max_rows of them.
int lammps_le_thermo_log(void *handle, double *out, int max_rows) {
  Engine *e = (Engine *)handle;
  const int n = (int)e->thermo_log.size();
  for (int k = 0; k < n && k < max_rows; k++) {
    const ThermoRow &r = e->thermo_log[(size_t)k];
    double *o = out + 7 * (size_t)k;
    o[0] = (double)r.step; o[1] = r.temp; o[2] = r.epair; o[3] = r.emol; o[4] = r.etotal; o[5] = r.press; o[6] = (double)r.nbonds;
  }
  return n;
}
double lammps_le_stat(void *handle, const char *name) {
  Engine *e = (Engine *)handle;
  std::string k = name;
  if (k == "loop_time") return e->loop_time;
  if (k == "neigh_builds") return (double)e->neigh_builds;
  // the plan the last rebuild executed (RebuildBit, rebuild_plan.h): "rebuild_plan" the bits that follow from the 22 facts of
  // lammps_le_test_rebuild_plan, i.e. what that hook answers for the same facts; "rebuild_plan_full" with RB_LAZY_V as well
  if (k == "rebuild_plan") return (double)(e->rebuild_plan_bits & ~(unsigned)RB_LAZY_V);
  if (k == "rebuild_plan_full") return (double)e->rebuild_plan_bits;
  if (k == "lazy_rebuilds") return (double)e->lazy_rebuilds;         // rebuilds of the last run under RB_LAZY_V
  if (k == "velocities_settled") return e->dev ? (double)e->dev->v_settled : 0.0;   // settle_velocities launches since the arrays were allocated
  // time steps of the last run by the path they took: the step kernel (steps_fused_group of them its group variant), its
  // energy variant on a thermo step, the unfused kernels; the three add up to the steps of the run
  if (k == "steps_fused") return (double)e->steps.fused;
  if (k == "steps_fused_group") return (double)e->steps.fused_group;
  if (k == "steps_fused_thermo") return (double)e->steps.fused_thermo;
  if (k == "steps_unfused") return (double)e->steps.unfused;
  if (k == "steps_fused_ext") return (double)e->steps.fused_ext;        // of steps_fused: spring/self, addforce, setforce inside the step kernel
  if (k == "steps_fused_wall") return (double)e->steps.fused_wall;      // of steps_fused: fix wall/region inside the step kernel
  if (k == "steps_fused_indent") return (double)e->steps.fused_indent;  // of steps_fused: the launch carried an indenter of fix indent
  if (k == "steps_fused_soft") return (double)e->steps.fused_soft;      // of steps_fused: pair_style soft inside the step kernel
  if (k == "pair_table_copies") return (double)e->pair_table_copies;    // fix adapt: copies of the pair table in the middle of runs
  // the last `minimize`: iterations, force evaluations, index into Min::stopstrings, the last line search's alpha, times the host
  // waited for the device, list builds; and the numbers of its stats block
  if (k == "min_iterations") return (double)e->min_niter;
  if (k == "min_evals") return (double)e->min_neval;
  if (k == "min_stop") return (double)e->min_stop;
  if (k == "min_alpha") return e->min_alpha;
  if (k == "min_host_waits") return (double)e->min_host_waits;
  if (k == "min_rebuilds") return (double)e->min_rebuilds;
  if (k == "min_e_initial") return e->min_einitial;
  if (k == "min_e_previous") return e->min_eprevious;
  if (k == "min_e_final") return e->min_efinal;
  if (k == "min_fnorm_initial") return e->min_fnorm2_init;
  if (k == "min_fnorm_final") return e->min_fnorm2_final;
  if (k == "min_fmax_initial") return e->min_fnorminf_init;
  if (k == "min_fmax_final") return e->min_fnorminf_final;
  if (k == "host_waits") return e->dev ? (double)e->dev->host_waits : 0.0;
  if (k == "neigh_time" || k == "time_neigh") return e->timers[Engine::T_NEIGH];
  if (k == "time_pair") return e->timers[Engine::T_PAIR];
  if (k == "time_bond") return e->timers[Engine::T_BOND];
  if (k == "time_comm") return e->timers[Engine::T_COMM];
  if (k == "time_output") return e->timers[Engine::T_OUTPUT];
  if (k == "time_modify") return e->timers[Engine::T_MODIFY];
  if (k == "time_other") {
    double all = 0.0;
    for (int s = 0; s < Engine::T_NSECT; s++) all += e->timers[s];
    return e->loop_time - all;
  }
  if (k == "comm_nranks") return e->comm ? (double)e->comm->nranks() : 1.0;
  if (k == "rng_late_generations") return (double)e->rng_late_count;
  if (k == "rng_segments_held") return e->dev ? (double)rng_segments_held(*e->dev) : 0.0;
  if (k == "rng_segments") return e->dev ? (double)e->dev->rng_nseg : 0.0;
  if (k == "comm_bytes_allgather") return e->comm ? e->comm->bytes_allgather : 0.0;
  if (k == "comm_bytes_allreduce") return e->comm ? e->comm->bytes_allreduce : 0.0;
  if (k == "halo_window_mismatches") return e->dev ? (double)dd_halo_mismatches(*e->dev) : 0.0;   // LAMMPS_LE_FAST_HALO_VERIFY
  if (k == "angle_records" || k == "angle_records_max") {     // listed-angle records of the owned beads (sum / longest), as of the last reneighbor
    if (!e->dev || !e->dev->eff_n || e->dev->n <= 0) return 0.0;
    std::vector<int> c((size_t)e->dev->n);
    HIP_CHECK(hipMemcpy(c.data(), e->dev->eff_n, c.size() * sizeof(int), hipMemcpyDeviceToHost));
    double sum = 0.0, mx = 0.0;
    for (int v : c) { sum += v; mx = std::max(mx, (double)v); }
    return k == "angle_records" ? sum : mx;
  }
  if (k == "special_asym") return e->dev ? (double)e->dev->flags_h[FLAG_SPECIAL_ASYM] : 0.0;   // some 1-2 list lost an entry its partner still has (sticky)
  if (k == "halo_fused") return e->dev && e->dev->fast_halo && e->dev->halo_fused ? 1.0 : 0.0;   // counters + window copy in one launch
  if (k == "halo_sent_both") return e->dev ? (double)e->dev->nsend_both : 0.0;   // beads of this rank in both send lists at the last rebuild
  if (k == "halo_pack_launches") return e->dev ? (double)e->dev->halo_pack_launches : 0.0;   // k_dd_pack launches of dd_halo so far
  if (k == "halo_window_exchanges") return e->dev ? (double)e->dev->halo_seq : 0.0;   // per-step halos that went through the peer windows
  if (k == "pair_kernel_ms") return e->kstat_ms;
  if (k == "pair_kernel_launches") return (double)e->kstat_n;
  if (k == "neigh_pairs") return e->stat_neigh_pairs();
  if (k == "maxneigh") return e->dev ? (double)e->dev->maxneigh : 0.0;
  if (k == "nlocal") return e->dev ? (double)e->dev->n : 0.0;
  if (k == "nghost") return e->dev ? (double)e->dev->nghost : 0.0;
  if (k == "fene_warnings") return e->dev && e->dev->flags_h ? (double)e->dev->flags_h[FLAG_FENE_WARN] : 0.0;
  if (k == "bond_minimg") return e->dev ? (double)e->dev->bond_minimg : 0.0;   // bonds take the per-step minimum image (1) or the frozen image words (0), as of the last run
  if (k == "pair_row_passes") return (double)e->pair_row_passes;        // device passes of the local computes' pair rows so far
  if (k == "pair_rows") return (double)e->pair_rows_last;              // ... the rows of the last one (whole system)
  if (k == "pair_rows_count_ms") return e->pair_rows_ms[0];            // ... its count pass + scan, its fill pass + copy (host wall clock)
  if (k == "pair_rows_fill_ms") return e->pair_rows_ms[1];
  if (k == "host_downloads") return (double)e->host_downloads;          // whole-system downloads (Engine::download)
  if (k == "device_current") return (e->dev && e->dev_current) ? 1.0 : 0.0;   // 0: the host copies are the state, the next run uploads
  if (k == "device_bytes") return e->dev ? (double)e->dev->mem.device_bytes() : 0.0;   // device blocks this handle holds
  if (k == "subset_comm_bytes") return e->subset_comm_bytes;           // this rank's share of the subset calls' collectives
  return -1.0;
}

}  // extern "C"

// test hook (not part of the reference surface): RanMarsInt stream after a jump, for the CPU unit tests
extern "C" void lammps_le_test_ranmars(int seed, long long skip, int n, double *out) {
  lmp_le::RanMarsInt r;
  r.seed(seed);
  r.jump((uint64_t)skip);
  for (int i = 0; i < n; i++) out[i] = r.uniform();
}

// test hook (not part of the reference surface, not declared in include/lammps_le.h): the width rule of the z-slab
// decomposition (device.h slab_rule) without a device.  Returns 0 = accepted, 1 = thinner than one ghost cutoff, 2 = thinner
// than two pair shells, 3 = ghost shells overlap; the error text Engine::upload would throw goes to msg (cap bytes).
extern "C" int lammps_le_test_slab_rule(double prd_z, int world, double cutneighmax, double comm_cutoff, char *msg, int cap) {
  std::string why;
  const int code = (int)lmp_le::slab_rule(prd_z, world, cutneighmax, comm_cutoff, why);
  if (msg && cap > 0) { strncpy(msg, why.c_str(), (size_t)cap - 1); msg[cap - 1] = 0; }
  return code;
}

// test hooks (not part of the reference surface, not declared in include/lammps_le.h): the arithmetic of pair_style soft
// (soft_inl.h) compiled for the host - the same functions, the same fma's the kernels run.  The sine and cosine on [0, pi] for n
// arguments; the pair term for n squared distances with A and rc: fpair and energy without the special weight.  The host's
// estimate of the reciprocal square root stands in for v_rsq_f64 (cut to 24 bits: the Newton steps must do the rest here too)
extern "C" void lammps_le_test_soft_sincos(int n, const double *x, double *s, double *c) {
  for (int i = 0; i < n; i++) { s[i] = lmp_le::soft_sin_0pi(x[i]); c[i] = lmp_le::soft_cos_0pi(x[i]); }
}
extern "C" void lammps_le_test_soft_pair(int n, const double *rsq, double a, double rc, double *fpair, double *evdwl) {
  const double pi = 3.14159265358979323846;
  const double a_pi_rc = a * pi / rc, pi_rc = pi / rc;          // the table columns as Engine::init_pair_coeffs derives them
  for (int i = 0; i < n; i++) {
    double seed = 1.0 / std::sqrt(rsq[i]);
    if (seed < 3.0e38 && seed > 1.2e-38) seed = (double)(float)seed;      // (outside float's range: the estimate as it is)
    double e = 0.0;
    fpair[i] = lmp_le::soft_pair<true>(rsq[i], seed, a_pi_rc, pi_rc, a, e);
    evdwl[i] = e;
  }
}

// test hook (not part of the reference surface, not declared in include/lammps_le.h):
// indent_force (indent_inl.h) compiled for the host: n beads (x[3n]) against one indenter on the orthogonal box lo / hi.
// geo = kind, axis, side | planeside, K, ctr x y z (as written: remapped here by indent_remap, as FixIndent::entry does), R | pos;
// f[3n] the force on every bead, sums[4] the columns in bead order
extern "C" void lammps_le_test_indent_force(int n, const double *x, const double *lo, const double *hi, const double *geo, double *f,
                                            double *sums) {
  Box box{};
  for (int c = 0; c < 3; c++) { box.lo[c] = lo[c]; box.hi[c] = hi[c]; box.prd[c] = hi[c] - lo[c]; box.half[c] = 0.5 * box.prd[c]; box.iprd[c] = 1.0 / box.prd[c]; }
  IndentEntry o{};
  o.kind = (int)geo[0]; o.axis = (int)geo[1]; o.side = (int)geo[2]; o.groupbit = 1;
  o.k = geo[3]; o.k3 = o.k / 3.0; o.r = geo[7];
  for (int c = 0; c < 3; c++)
    o.ctr[c] = indent_remap((o.kind == INDENT_CYLINDER && c == o.axis) ? box.lo[c] : geo[4 + c], box.lo[c], box.hi[c], box.prd[c]);
  for (int c = 0; c < 4; c++) sums[c] = 0.0;
  for (int i = 0; i < n; i++) {
    double f0 = 0.0, f1 = 0.0, f2 = 0.0;
    indent_force<true>(x[3 * i], x[3 * i + 1], x[3 * i + 2], o, box, f0, f1, f2, sums);
    f[3 * i] = f0; f[3 * i + 1] = f1; f[3 * i + 2] = f2;
  }
}

// test hook (not part of the reference surface, not declared in include/lammps_le.h): the table of fix indent that the force
// evaluation of step `now` of a run over steps [begin, end] would carry, without a device - the init() of a run command, the
// fixes in order, the formulas evaluated, the centres remapped.  out: per indenter ten numbers - kind, axis, side | planeside,
// group bit, phase, K, centre x y z, radius | position.  Returns the number of indenters, or -1 with the error recorded
extern "C" int lammps_le_test_indent_table(void *handle, long begin, long end, long now, double *out) {
  BEGIN_CAPTURE
  struct InRun { Engine *e; bool was; long b0, e0, n0; InRun(Engine *en) : e(en), was(en->in_run), b0(en->beginstep), e0(en->endstep), n0(en->ntimestep) {}
                 ~InRun() { e->in_run = was; e->beginstep = b0; e->endstep = e0; e->ntimestep = n0; } } keep(e);
  e->init();
  e->postforce.build(e->fixes, e->natoms);
  e->in_run = true; e->beginstep = begin; e->endstep = end; e->ntimestep = now;
  const IndentTable t = e->postforce.indent_table();
  for (int k = 0; k < t.n; k++) {
    const IndentEntry &o = t.e[k];
    const double row[10] = {(double)o.kind, (double)o.axis, (double)o.side, (double)o.groupbit, (double)o.phase, o.k, o.ctr[0], o.ctr[1], o.ctr[2], o.r};
    for (int c = 0; c < 10; c++) out[10 * k + c] = row[c];
  }
  return t.n;
  END_CAPTURE
  return -1;
}

// test hook (not part of the reference surface, not declared in include/lammps_le.h): what the one walk over the fixes makes of
// the script, without a device - the init() of a run command, then PostForce::build.  out: per post-force fix, in fix order, four
// numbers - family (0 wall/region, 1 indent, 2 spring/self | addforce | setforce), index within its table, phase, group bit.
// Returns the number of rows, or -1 with the error recorded on the handle
extern "C" int lammps_le_test_post_force_rows(void *handle, int *out) {
  BEGIN_CAPTURE
  e->init();
  PostForce &pf = e->postforce;
  pf.build(e->fixes, e->natoms);
  int n = 0;
  auto put = [&](int family, size_t k, int phase, int bit) { int *r = out + 4 * n++; r[0] = family; r[1] = (int)k; r[2] = phase; r[3] = bit; };
  for (auto &f : e->fixes) {
    for (size_t k = 0; k < pf.wall_fixes.size(); k++) if (pf.wall_fixes[k] == f.get()) put(0, k, pf.walltab.w[k].after_langevin, pf.walltab.w[k].groupbit);
    for (size_t k = 0; k < pf.indent_fixes.size(); k++) if (pf.indent_fixes[k] == f.get()) put(1, k, pf.indent_phase[k], f->groupbit);
    for (size_t k = 0; k < pf.forceop_fixes.size(); k++) if (pf.forceop_fixes[k] == f.get()) put(2, k, pf.forceoptab.e[k].phase, pf.forceoptab.e[k].groupbit);
  }
  return n;
  END_CAPTURE
  return -1;
}

// test hook (not part of the reference surface, not declared in include/lammps_le.h): the derived pair coefficients as the
// script layer holds them, without a device - what Engine::push_pair_table would send.  phase 0: after the init() of a run
// command; 1: at the setup of a run over steps [begin, end] (fix adapt's setup_pre_force); 2: before the forces of step `now`
// of that run (pre_force); 3: after the run (post_run).  out: 6 columns of (ntypes+1)^2 - cutsq lj1 lj2 lj3 lj4 offset, under
// pair_style soft cutsq, A pi/rc, pi/rc, A, 0, 0.  Returns ntypes + 1, or -1 with the error recorded on the handle.
extern "C" int lammps_le_test_pair_coeffs(void *handle, int phase, long begin, long end, long now, double *out) {
  BEGIN_CAPTURE
  struct InRun { Engine *e; bool was; long b0, e0, n0; InRun(Engine *en) : e(en), was(en->in_run), b0(en->beginstep), e0(en->endstep), n0(en->ntimestep) {}
                 ~InRun() { e->in_run = was; e->beginstep = b0; e->endstep = e0; e->ntimestep = n0; } } keep(e);
  if (phase == 0) e->init();
  else {
    e->in_run = true; e->beginstep = begin; e->endstep = end; e->ntimestep = phase == 1 ? begin : now;
    if (phase == 1) e->adapt_set_values(true);
    else if (phase == 2) e->adapt_set_values(false);
    else e->adapt_restore_values();
  }
  const int nt = e->ntypes + 1;
  const std::vector<double> *col[6] = {&e->cutsq, &e->lj1, &e->lj2, &e->lj3, &e->lj4, &e->offset};
  for (int q = 0; q < 6; q++)
    for (int k = 0; k < nt * nt; k++) out[(size_t)q * nt * nt + k] = (*col[q])[k];
  return nt;
  END_CAPTURE
  return -1;
}

// test hook (not part of the reference surface, not declared in include/lammps_le.h): what all instances of this process
// hold at this moment - out[0] device + pinned blocks, out[1] their bytes, out[2] streams + events (DevMem, device.h)
extern "C" void lammps_le_test_live_resources(long long *out) { lmp_le::DevMem::live(out); }

// test hook (not part of the reference surface, not declared in include/lammps_le.h): the neighbor list of the last build,
// decoded on the host and named by TAGS.  Pair entries (i, j, special level bits of the word) go to itag / jtag / code,
// at most `cap` of them; the bond entries that open every list go to btag / bjtag / btype, at most `bcap` of them (their
// number to *nbond); owned_tag[nlocal] and xbuild[3 * nlocal] receive the owned beads in list order and the positions the
// list was built from (xhold).  Rank-local: a decomposed run hands out the lists of the beads this rank owns, ghost
// neighbors by their tag.  Returns the number of pair entries there are (a first call with cap = 0 sizes the buffers),
// -1 with the error string set when no list has been built yet.  Output pointers may be null.
extern "C" long long lammps_le_test_neighbor_list(void *handle, long long cap, int *itag, int *jtag, int *code,
                                                  int *btag, int *bjtag, int *btype, long long bcap, long long *nbond,
                                                  int *owned_tag, double *xbuild) {
  long long npair = -1;
  BEGIN_CAPTURE
  if (!e->dev || !e->dev->neigh || !e->dev->numneigh || e->reneigh_pending)
    throw LammpsError("lammps_le_test_neighbor_list: no neighbor list has been built yet");
  DeviceState &d = *e->dev;
  stream_sync(d);
  const size_t n = (size_t)d.n, nslots = n + (size_t)(d.dd ? d.nghost : 0), np = (size_t)d.npad;
  std::vector<int> nn(n), tg(nslots), row(n);
  std::vector<double4> xh(n);
  HIP_CHECK(hipMemcpy(nn.data(), d.numneigh, n * sizeof(int), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(tg.data(), d.tag, nslots * sizeof(int), hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(xh.data(), d.xhold, n * sizeof(double4), hipMemcpyDeviceToHost));
  int longest = 0;
  for (size_t s = 0; s < n; s++) longest = std::max(longest, nn[s] & NN_COUNT_MASK);
  if (longest > d.maxneigh) throw LammpsError("lammps_le_test_neighbor_list: a count word exceeds the table");
  std::vector<int> tab((size_t)longest * np);      // the table is column-major: row k of every bead is contiguous
  if (longest) HIP_CHECK(hipMemcpy(tab.data(), d.neigh, tab.size() * sizeof(int), hipMemcpyDeviceToHost));
  auto tag_of = [&](int q) -> int {
    if (q < 0 || (size_t)q >= nslots) throw LammpsError("lammps_le_test_neighbor_list: entry points outside the bead slots");
    return tg[(size_t)q];
  };
  long long np_out = 0, nb_out = 0;
  for (size_t s = 0; s < n; s++) {
    if (owned_tag) owned_tag[s] = tg[s];
    if (xbuild) { xbuild[3 * s] = xh[s].x; xbuild[3 * s + 1] = xh[s].y; xbuild[3 * s + 2] = xh[s].z; }
    const int cnt = nn[s] & NN_COUNT_MASK, nb = (nn[s] >> NN_BOND_SHIFT) & NN_NBOND_MASK;
    if (nb > cnt) throw LammpsError("lammps_le_test_neighbor_list: more bond entries than entries");
    for (int k = 0; k < cnt; k++) {
      const int w = tab[(size_t)k * np + s];
      if (k < nb) {
        if (nb_out < bcap && btag && bjtag && btype) {
          btag[nb_out] = tg[s]; bjtag[nb_out] = tag_of(w & BOND_IDX_MASK); btype[nb_out] = (w >> BOND_TYPE_SHIFT) & 0x1F;
        }
        nb_out++;
      } else {
        if (np_out < cap && itag && jtag && code) {
          itag[np_out] = tg[s]; jtag[np_out] = tag_of(w & NEIGH_MASK); code[np_out] = (w >> NEIGH_SB_SHIFT) & 3;
        }
        np_out++;
      }
    }
  }
  if (nbond) *nbond = nb_out;
  npair = np_out;
  END_CAPTURE
  return npair;
}

// ---- ranks: one process per GPU (bench.py passes the ncclUniqueId it broadcast with torch.distributed) ----
extern "C" int lammps_le_comm_unique_id(char *out128) {
  try { lmp_le::comm_unique_id(out128); return 0; } catch (const std::exception &ex) { fprintf(stderr, "%s\n", ex.what()); return 1; }
}
extern "C" void lammps_le_comm_init(void *handle, const char *backend, int rank, int world, const char *unique_id,
                                    const char *session) {
  BEGIN_CAPTURE e->comm_init(backend, rank, world, unique_id, session ? session : "default"); END_CAPTURE
}
// RCCL binding self-test on one GPU (size-1 communicator): 0 = pass
extern "C" int lammps_le_rccl_selftest() {
  try { return lmp_le::comm_rccl_selftest(); } catch (const std::exception &ex) { fprintf(stderr, "%s\n", ex.what()); return 1; }
}
// transport self-test without a GPU ("shm" backend): ring exchange + all-gather + max-reduce; returns 0 on success
extern "C" int lammps_le_comm_selftest(const char *session, int rank, int world) {
  using namespace lmp_le;
  try {
    Comm c;
    c.init("shm", rank, world, nullptr, session);
    int up = (rank + 1) % world, dn = (rank + world - 1) % world;
    double sendv[4] = {rank + 0.25, rank + 0.5, 0, 0}, recvv[4] = {0, 0, 0, 0};
    c.exchange_host({{&sendv[0], sizeof(double), dn}, {&sendv[1], sizeof(double), up}},
                    {{&recvv[1], sizeof(double), up}, {&recvv[0], sizeof(double), dn}});
    if (recvv[1] != up + 0.25 || recvv[0] != dn + 0.5) return 2;
    std::vector<int> all(world);
    int mine = 100 + rank;
    c.allgather_host(&mine, all.data(), sizeof(int));
    for (int r = 0; r < world; r++) if (all[r] != 100 + r) return 3;
    if (c.allreduce_host_max(rank * 7) != (world - 1) * 7) return 4;
    double s = c.allreduce_host_sum((double)rank);
    if (s != world * (world - 1) / 2.0) return 5;
    c.barrier();
    return 0;
  } catch (const std::exception &ex) { fprintf(stderr, "%s\n", ex.what()); return 1; }
}

// debug hook (tests only): copy one of the tag-indexed LE scratch arrays (int) or the pair-distance array (double)
extern "C" void lammps_le_debug_le_array(void *handle, int slot, int n, int *out_i, double *out_d) {
  lmp_le::Engine *e = (lmp_le::Engine *)handle;
  if (!e->dev) return;
  if (out_i) (void)hipMemcpy(out_i, e->dev->le_i[slot], (size_t)n * sizeof(int), hipMemcpyDeviceToHost);
  if (out_d) (void)hipMemcpy(out_d, e->dev->le_d[0], (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
}

// test hooks of the launch census (not part of the reference surface, not declared in include/lammps_le.h).  kernel: 0 = k_step
// (keys: StepKeyBit, the template argument of k_step), 1 = k_force (force_variant_key), step_plan.h.
// The launches of a handle so far as (key, count) pairs with count > 0, ascending by key; returns how many there are (at most
// `cap` are stored)
extern "C" int lammps_le_test_step_census(void *handle, int kernel, int cap, int *keys, long long *counts) {
  lmp_le::Engine *e = (lmp_le::Engine *)handle;
  if (!e || !e->dev) return 0;
  const unsigned *c = kernel ? e->dev->force_census : e->dev->step_census;
  const int space = kernel ? lmp_le::FORCE_KEY_SPACE : lmp_le::STEP_KEY_SPACE;
  int n = 0;
  for (int k = 0; k < space; k++)
    if (c[k]) { if (n < cap) { keys[n] = k; counts[n] = c[k]; } n++; }
  return n;
}
extern "C" void lammps_le_test_step_census_reset(void *handle) {
  lmp_le::Engine *e = (lmp_le::Engine *)handle;
  if (!e || !e->dev) return;
  std::fill(e->dev->step_census, e->dev->step_census + lmp_le::STEP_KEY_SPACE, 0u);
  std::fill(e->dev->force_census, e->dev->force_census + lmp_le::FORCE_KEY_SPACE, 0u);
}
// the keys of the instantiations that exist (step_variant_exists; the condition of launch_force), ascending, without a device;
// returns how many there are
extern "C" int lammps_le_test_step_keys(int kernel, int cap, int *keys) {
  const int space = kernel ? lmp_le::FORCE_KEY_SPACE : lmp_le::STEP_KEY_SPACE;
  int n = 0;
  for (int k = 0; k < space; k++)
    if (kernel ? lmp_le::force_key_exists(k) : lmp_le::step_variant_exists(k)) { if (n < cap) keys[n] = k; n++; }
  return n;
}
// key -> one number per bit, lowest first (k_step: fifteen, the lanes per bead of SK_LPB4 as 1 | 4; k_force: four) and back
extern "C" void lammps_le_test_step_key_decode(int kernel, int key, int *flags) {
  for (int b = 0; b < (kernel ? lmp_le::FORCE_KEY_BITS : lmp_le::STEP_KEY_BITS); b++) flags[b] = (key >> b) & 1;
  if (!kernel) flags[4] = (key & lmp_le::SK_LPB4) ? 4 : 1;
}
extern "C" int lammps_le_test_step_key(int kernel, const int *f) {
  int key = 0;
  for (int b = 0; b < (kernel ? lmp_le::FORCE_KEY_BITS : lmp_le::STEP_KEY_BITS); b++) key |= (f[b] != 0) << b;
  if (!kernel && f[4] != 4) key &= ~lmp_le::SK_LPB4;
  return key;
}
