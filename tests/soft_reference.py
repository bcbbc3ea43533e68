"""pair_style soft for the long-double brute-force reference (force_reference.py): the same candidate pairs, weights, images
and sums, with the soft term in place of lj/cut.

The statements of the reference program the formula was read from (paths below its src/):
  pair soft        pair_soft.cpp:96-117: strict rsq < cutsq; arg = pi r / rc; fpair = factor_lj A sin(arg) pi / rc / r for
                   r > 0 and 0 at r = 0; evdwl = factor_lj A (1 + cos(arg))
                   :200-213 init_one: A of a pair not given = sqrt(A_ii A_jj) whatever pair_modify mix says, rc by mix_distance
                   no offset (pair_modify shift does nothing), no tail correction

SoftSystem takes a force_reference.Model whose `pair` is dict(cut, mix, rows=[(i, j, A, rc)], shift=False); bonds, angles,
thermo and the integration are force_reference.System's own.
"""
import numpy as np

import force_reference as fr
from neigh_reference import LD

PI = fr.PI


def soft_model_pair(cut, rows, mix="geometric"):
    """Model.pair for SoftSystem: rows (i, j, A) or (i, j, A, rc)"""
    return dict(style="soft", cut=float(cut), shift=False, mix=mix,
                rows=[(int(r[0]), int(r[1]), float(r[2]), 1.0, float(r[3]) if len(r) > 3 else float(cut)) for r in rows])


def soft_terms(rsq, a, rc):
    """-> (fpair, evdwl) in long double; fpair = 0 where rsq = 0"""
    r = np.sqrt(rsq)
    arg = PI * r / rc
    safe = np.where(r > 0, r, LD(1))
    f = np.where(r > 0, a * np.sin(arg) * PI / rc / safe, LD(0))
    return f, a * (1 + np.cos(arg))


class SoftSystem(fr.System):
    """force_reference.System with the soft pair term.  The pair rows travel through pair_matrix as (A, sigma = 1, rc): its
    energy mixing is the geometric mean under both `mix` settings, which is PairSoft::init_one's rule."""

    def evaluate(self, x, only=None):
        assert self.model.pair is not None and self.model.pair.get("style") == "soft"
        pair, self.model.pair = self.model.pair, None
        try:
            rest = super().evaluate(x, only)          # bonds and angles
        finally:
            self.model.pair = pair
        x = fr.ld(x)
        n, prd = self.n, self.prd
        f_pair = np.zeros((n, 3), dtype=LD)
        evdwl, vpair = LD(0), np.zeros(6, dtype=LD)
        gap, gap_pair, terms = LD(np.inf), None, dict(rest.terms)
        sel = slice(None) if only is None else np.nonzero((self.iu == only) | (self.ju == only))[0]
        iu, ju = self.iu[sel], self.ju[sel]
        d0 = fr.min_image(x[iu] - x[ju], prd)
        shifts = [np.zeros(3, dtype=LD)]
        if self.multi_image:
            shifts += [fr.ld(s) * prd for s in (np.array(t) - 1 for t in np.ndindex(3, 3, 3)) if s.any()]
        for k, sh in enumerate(shifts):
            d = d0 + sh
            rsq = (d * d).sum(axis=1)
            g = np.abs(rsq - self.p_cutsq[sel])
            if k == 0:
                g = np.where(self.w[sel] != 0, g, LD(np.inf))
            if len(g) and g.min() < gap:
                q = int(np.argmin(g))
                gap, gap_pair = g[q], (int(iu[q]), int(ju[q]), float(self.p_cut[sel][q]))
            hit = np.nonzero((rsq < self.p_cutsq[sel]) & ((self.w[sel] != 0) if k == 0 else True))[0]
            fp, e = soft_terms(rsq[hit], self.p_eps[sel][hit], self.p_cut[sel][hit])
            wt = self.w[sel][hit] if k == 0 else LD(1)
            fp, e = fp * wt, e * wt
            fv = d[hit] * fp[:, None]
            np.add.at(f_pair, iu[hit], fv)
            np.add.at(f_pair, ju[hit], -fv)
            evdwl += e.sum()
            vpair += fr.virial6(d[hit], fv)
            if k == 0:
                terms["pair"] = (iu[hit], ju[hit], d[hit], fv)
        return fr.Eval(f_pair + rest.f_bond + rest.f_angle, f_pair, rest.f_bond, rest.f_angle, evdwl, rest.ebond, rest.eangle,
                       vpair, rest.vbond, rest.vangle, gap, gap_pair, rest.fene_clamped, rest.angle_clamped, rest.max_bond_frac,
                       terms)
