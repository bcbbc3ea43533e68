// indent_inl.h — the force of one fix indent on one bead (FixIndent::post_force for one atom, src/fix_indent.cpp:184-355),
// written once for the device (k_indent and the wall variant of k_step, kernels_md.hip) and for the host (the test hook in
// capi.cpp, lammps_le_test_indent_force).
//
//   sphere | cylinder:  del = x - ctr (the axis component 0 for a cylinder), Domain::minimum_image, r = |del|,
//                       dr = r - R (side out) | R - r (side in); nothing if dr >= 0;  f += del * (+-K dr^2) / r
//   plane:              dr = planeside * (pos - x[dim]); nothing if dr >= 0;  f[dim] -= planeside * K dr^2
//
// Plain IEEE arithmetic in the reference's operation order: both translation units that include this header are compiled
// without contraction, and `/` is a divide.  The centre arrives remapped into the box (FixIndent::entry, as Domain::remap).
// A bead exactly at the centre of a `side out` indenter divides by zero here as it does in the reference.
#pragma once
#include <cmath>

#include "engine.h"

#if defined(__HIPCC__)
#define INDENT_HD __host__ __device__ __forceinline__
#else
#define INDENT_HD inline
#endif

namespace lmp_le {

// Domain::minimum_image on the orthogonal periodic box, one component (src/domain.cpp:983-988).  The reference's `while` ends
// only once |d| <= half: on a coordinate that has blown up (inf, or so large that the period no longer changes it) it never
// would, and a kernel has to end.  INDENT_MINIMG_TRIPS periods is far beyond what a bead can be away from a centre inside the
// box between two list builds (positions are wrapped at every build); up to there the result is the reference's
constexpr int INDENT_MINIMG_TRIPS = 64;
INDENT_HD double indent_minimg(double d, double prd, double half) {
  for (int trip = 0; trip < INDENT_MINIMG_TRIPS && fabs(d) > half; trip++) {
    if (d < 0.0) d += prd;
    else d -= prd;
  }
  return d;
}

// Domain::remap on one coordinate of the periodic orthogonal box (src/domain.cpp:1460-1464): while below lo add a period, while
// at or above hi take one off, then max(coord, lo).  Host only (FixIndent::entry and the test hook): a value that is not finite
// is left alone - the reference's loops would not end on it, and the force is nan either way
inline double indent_remap(double x, double lo, double hi, double prd) {
  if (!std::isfinite(x)) return x;
  while (x < lo) x += prd;
  while (x >= hi) x -= prd;
  return x > lo ? x : lo;
}

// `acc` (EFLAG), four columns: -K/3 dr^3, -fx, -fy, -fz - the energy and the force on the indenter.  Every branch on the entry
// is wave-uniform
template <bool EFLAG>
INDENT_HD void indent_force(double x0, double x1, double x2, const IndentEntry &o, const Box &box, double &f0, double &f1,
                            double &f2, double *acc) {
  const int kind = o.kind, dim = o.axis;
  const double k = o.k;
  if (kind == INDENT_PLANE) {
    const double planeside = (double)o.side;
    const double xd = dim == 0 ? x0 : dim == 1 ? x1 : x2;
    const double dr = planeside * (o.r - xd);
    if (dr >= 0.0) return;
    const double fatom = -planeside * k * dr * dr;
    // (three selects, not `if (dim == 0) f0 += ..`: the compiler turns that chain into f[dim] += .. on an array in scratch)
    f0 = dim == 0 ? f0 + fatom : f0;
    f1 = dim == 1 ? f1 + fatom : f1;
    f2 = dim == 2 ? f2 + fatom : f2;
    if (EFLAG) {
      acc[0] -= o.k3 * dr * dr * dr;
      acc[1] = dim == 0 ? acc[1] - fatom : acc[1];
      acc[2] = dim == 1 ? acc[2] - fatom : acc[2];
      acc[3] = dim == 2 ? acc[3] - fatom : acc[3];
    }
    return;
  }
  double delx = x0 - o.ctr[0], dely = x1 - o.ctr[1], delz = x2 - o.ctr[2];
  const bool cyl = kind == INDENT_CYLINDER;
  delx = (cyl && dim == 0) ? 0.0 : delx;
  dely = (cyl && dim == 1) ? 0.0 : dely;
  delz = (cyl && dim == 2) ? 0.0 : delz;
  delx = indent_minimg(delx, box.prd[0], box.half[0]);
  dely = indent_minimg(dely, box.prd[1], box.half[1]);
  delz = indent_minimg(delz, box.prd[2], box.half[2]);
  const double r = sqrt(delx * delx + dely * dely + delz * delz);
  double dr, fmag;
  if (!o.side) {
    dr = r - o.r;
    fmag = k * dr * dr;
  } else {
    dr = o.r - r;
    fmag = -k * dr * dr;
  }
  if (dr >= 0.0) return;
  const double fx = delx * fmag / r, fy = dely * fmag / r, fz = delz * fmag / r;
  f0 += fx; f1 += fy; f2 += fz;
  if (EFLAG) {
    acc[0] -= o.k3 * dr * dr * dr;
    acc[1] -= fx; acc[2] -= fy; acc[3] -= fz;
  }
}

}  // namespace lmp_le
