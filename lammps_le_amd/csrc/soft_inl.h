// soft_inl.h — the arithmetic of pair_style soft (src/pair_soft.cpp:96-117), written once for the device (pair_term<SOFT>,
// kernels_md.hip) and for the host (the test hooks in capi.cpp, lammps_le_test_soft_*).
//
//   E = A (1 + cos(pi r / rc)),  fpair = A sin(pi r / rc) (pi / rc) / r      for r < rc
//
// The cutoff test keeps arg = pi r / rc inside [0, pi), so neither function needs the library's range reduction (a call, a
// table of 2/pi and a slow path the step kernel would carry in every instantiation): one fold at pi/2, then the odd Taylor
// polynomial of the sine up to x^21 on [-pi/2, pi/2], whose first dropped term is (pi/2)^23 / 23! = 1.3e-18.  Every product-sum
// is an explicit fma, so host and device round alike whatever -ffp-contract says.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SOFT_HD __host__ __device__ __forceinline__
#else
#define SOFT_HD inline
#endif

namespace lmp_le {

// pi and pi/2 as double + remainder (fdlibm's pio2_hi / pio2_lo and their doubles): pi - x is then right to the last bit of
// the SMALL result, which is what the sine near the cutoff is made of
constexpr double SOFT_PI_HI = 3.14159265358979311600e+00, SOFT_PI_LO = 1.22464679914735317723e-16;
constexpr double SOFT_PIO2_HI = 1.57079632679489655800e+00, SOFT_PIO2_LO = 6.12323399573676603587e-17;

// sin(y) for |y| <= pi/2: y + y^3 P(y^2), P = -1/3! + y^2/5! - ... - y^18/21! by Horner
SOFT_HD double soft_sin_core(double y) {
  const double z = y * y;
  double p = -1.9572941063391261231e-20;      // -1/21!
  p = fma(p, z, 8.2206352466243297170e-18);   //  1/19!
  p = fma(p, z, -2.8114572543455207632e-15);  // -1/17!
  p = fma(p, z, 7.6471637318198164759e-13);   //  1/15!
  p = fma(p, z, -1.6059043836821614599e-10);  // -1/13!
  p = fma(p, z, 2.5052108385441718775e-08);   //  1/11!
  p = fma(p, z, -2.7557319223985890653e-06);  // -1/9!
  p = fma(p, z, 1.9841269841269841270e-04);   //  1/7!
  p = fma(p, z, -8.3333333333333333333e-03);  // -1/5!
  p = fma(p, z, 1.6666666666666666667e-01);   //  1/3!
  return fma(-(y * z), p, y);
}
// sin(x), 0 <= x <= pi
SOFT_HD double soft_sin_0pi(double x) {
  const double y = (x > SOFT_PIO2_HI) ? (SOFT_PI_HI - x) + SOFT_PI_LO : x;
  return soft_sin_core(y);
}
// cos(x), 0 <= x <= pi: sin(pi/2 - x)
SOFT_HD double soft_cos_0pi(double x) { return soft_sin_core((SOFT_PIO2_HI - x) + SOFT_PIO2_LO); }

// r = sqrt(rsq) and rinv = 1 / r from ONE reciprocal square root (`seed`: v_rsq_f64 on the device, any estimate good to 2^-20
// on the host) and two Newton steps, in the manner of rcp_nr; rsq == 0: r = rinv = 0, so that coincident beads get zero force
// instead of 0 * inf
SOFT_HD void soft_r_rinv(double rsq, double seed, double &r, double &rinv) {
  double y = (rsq > 0.0) ? seed : 0.0;
  double e = fma(-(rsq * y), y, 1.0);
  y = fma(0.5 * y, e, y);
  e = fma(-(rsq * y), y, 1.0);
  y = fma(0.5 * y, e, y);
  double s = rsq * y;
  s = fma(fma(-s, s, rsq), 0.5 * y, s);       // (one correction of the root itself: <= 1 ulp from sqrt)
  r = s; rinv = y;
}

// one pair: the columns of the pair table under pair_style soft are cutsq, A pi/rc, pi/rc, A (Engine::init_pair_coeffs).
// Returns fpair without the special weight; `e` (EFLAG) the energy likewise
template <bool EFLAG>
SOFT_HD double soft_pair(double rsq, double seed, double a_pi_rc, double pi_rc, double a, double &e) {
  double r, rinv;
  soft_r_rinv(rsq, seed, r, rinv);
  const double arg = r * pi_rc;
  if (EFLAG) e = fma(a, soft_cos_0pi(arg), a);
  return a_pi_rc * soft_sin_0pi(arg) * rinv;
}

}  // namespace lmp_le
