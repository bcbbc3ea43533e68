"""Brute-force reference of forces, energies, virial, pressure and the integration (plain numpy, no GPU, no oracle).

What the force kernels (kernels_md.hip pair_term, bond_term, bead_force, k_force, the k_step variants, k_angle, k_ke_tensor,
k_colsum) have to produce, derived without any of their machinery: no cells, no neighbor list, no frozen image words, no
coefficient tables - every pair of beads is measured in numpy.longdouble (64-bit mantissa) with the minimum image, every
formula is written in its textbook form (sigma / r, not lj1 .. lj4), and the sums run over pairs, bonds and angles once
each, not from both ends.  Only `neigh_reference.reference_specials` (the breadth-first search over the bond graph) and
`LD` are reused.

The statements of the reference program each formula was read from (paths below its src/):
  pair lj/cut      pair_lj_cut.cpp:112-134 (strict rsq < cutsq, force, energy minus offset, factor_lj on both),
                   :459-494 init_one (mixing of the pairs not given, offset = 4 eps ((sigma/rc)^12 - (sigma/rc)^6) under
                   `shift yes`), pair.cpp:675-700 mix_energy / mix_distance (geometric | arithmetic; the energy is sqrt(eps_i eps_j) under both)
  special weight   npair_half_bin_newtoff.cpp:103-112: by the level find_special gives, and only for the closest image of
                   the partner (minimum_image_check) - a farther image is an ordinary neighbor
  bond fene        MOLECULE/bond_fene.cpp:81-110: rlogarg = 1 - r^2 / R0^2, clamped to 0.1 below 0.1 (with a warning; an
                   error at <= -3), the WCA part below 2^(1/3) sigma^2
  bond harmonic    MOLECULE/bond_harmonic.cpp:74-83; bond morse: MOLECULE/bond_morse.cpp:76-85
  bond / angle image   ntopo_bond_all.cpp:65, ntopo_angle_all.cpp:69-71 (Domain::closest_image): with every bond shorter
                   than half the shortest box edge (asserted at every evaluation) that is the minimum image
  angle harmonic   MOLECULE/angle_harmonic.cpp:95-140 (sin theta clamped to SMALL = 0.001 from below, :30, :104)
  angle cosine     MOLECULE/angle_cosine.cpp:90-125
  virial           pair.cpp ev_tally / bond.cpp ev_tally / angle.cpp ev_tally: del (x) force per term, order xx yy zz xy xz yz
  temperature      compute_temp.cpp:60-68, 90-101 (dof = 3N - 3); ke: thermo.cpp:1724-1725
  pressure         compute_pressure.cpp:244-256 (scalar), :282-300 (tensor, with the kinetic tensor of compute_temp.cpp)
  fix nve          fix_nve.cpp:64-141 (initial_integrate / final_integrate, on the members of its group)
  fix langevin     fix_langevin.cpp:298-305 (gfactor1, gfactor2), :662-671, 714-716 (f += gamma1 v + gamma2 (u - 0.5), three
                   uniform draws per member in local order), setup() -> post_force (:280-290 of the same file, verlet.cpp:153)
  wrap             domain.cpp Domain::remap / pbc: x -+ prd with the image flag counting the other way
"""
import collections
import contextlib
import sys

import numpy as np

from neigh_reference import LD, reference_specials

UNITS = {  # update.cpp Update::set_units
    "lj": dict(boltz=1.0, mvv2e=1.0, ftm2v=1.0, nktv2p=1.0),
    "real": dict(boltz=0.0019872067, mvv2e=48.88821291 * 48.88821291, ftm2v=1.0 / 48.88821291 / 48.88821291, nktv2p=68568.415),
}
SMALL = LD("0.001")
PI = LD("3.14159265358979323846264338327950288")
TWO_1_3 = LD(2) ** (LD(1) / LD(3))


def ld(a):
    return np.asarray(a, dtype=LD)


def _constants():
    global SMALL, PI, TWO_1_3
    SMALL, PI, TWO_1_3 = LD("0.001"), LD("3.14159265358979323846264338327950288"), LD(2) ** (LD(1) / LD(3))


@contextlib.contextmanager
def precision(dtype):
    """The dtype switch of the restatement: inside the block this module and the modules that add terms to it (soft_reference,
    wall_reference, extforce_reference, indent_reference, as far as they are loaded) compute in `dtype` instead of long double -
    the same statements in the same order.  A System has to be built AND used inside the block.  What a run in np.float64 is off
    by from the long-double run is the rounding of this restatement in the engine's own number format: the figure that stands
    in for the oracle's deviation (force_compare.bound) where the oracle has no such term."""
    global LD
    mods = [sys.modules[m] for m in ("soft_reference", "wall_reference", "extforce_reference", "indent_reference") if m in sys.modules]
    keep = LD
    try:
        LD = dtype
        _constants()
        for m in mods:
            m.LD = dtype
            if hasattr(m, "PI"):
                m.PI = PI
        yield
    finally:
        LD = keep
        _constants()
        for m in mods:
            m.LD = keep
            if hasattr(m, "PI"):
                m.PI = PI


# ------------------------------------------------------------------------------------------------
# the model: everything a script says about forces and integration
# ------------------------------------------------------------------------------------------------
class Model:
    def __init__(self):
        self.units = "lj"
        self.special_lj = (0.0, 0.0, 0.0)
        self.pair = None            # dict(cut, shift, mix, rows=[(i, j, eps, sigma, cut)]) in the order given
        self.bond = {}              # type -> (style, coefficients ...)
        self.angle = {}             # type -> (style, coefficients ...)
        self.dt = 0.005
        self.norm = None            # thermo_modify norm (None: the units' default - lj yes, real no)
        self.nve_types = None       # fix nve on `group ID type ...`: the atom types that move (None: all)
        self.langevin = None        # (t_start, t_stop, damp, seed)
        self.nve = False


def model_from_script(script, ntypes):
    """Reads the force-field and integration commands of a script (the subset the force tests use); every other command
    of the scripts the tests run (neighbor, neigh_modify, newton, atom_modify, read_data, thermo, run ...) says nothing
    about what the forces are."""
    m = Model()
    groups = {"all": None}
    bstyle = astyle = None
    for line in script.split("\n"):
        w = line.split("#")[0].split()
        if not w:
            continue
        c, a = w[0], w[1:]
        if c == "units":
            m.units = a[0]
        elif c == "special_bonds":
            if a[0] == "fene":
                m.special_lj = (0.0, 1.0, 1.0)
            else:
                assert a[0] == "lj" and len(a) == 4, line
                m.special_lj = tuple(float(v) for v in a[1:4])
        elif c == "pair_style":
            assert a[0] in ("lj/cut", "zero"), line
            m.pair = dict(cut=float(a[1]), shift=False, mix="geometric", rows=[]) if a[0] == "lj/cut" else None
        elif c == "pair_modify":
            kw = dict(zip(a[::2], a[1::2]))
            if "shift" in kw:
                m.pair["shift"] = kw["shift"] == "yes"
            if "mix" in kw:
                m.pair["mix"] = kw["mix"]
        elif c == "pair_coeff" and m.pair is not None:
            def span(tok):
                if "*" not in tok:
                    return [int(tok)]
                lo, hi = tok.split("*")
                return range(int(lo) if lo else 1, (int(hi) if hi else ntypes) + 1)
            for i in span(a[0]):
                for j in span(a[1]):
                    if j >= i:
                        m.pair["rows"].append((i, j, float(a[2]), float(a[3]), float(a[4]) if len(a) > 4 else m.pair["cut"]))
        elif c == "bond_style":
            bstyle = a[0]
        elif c == "bond_coeff":
            st, vals = (a[1], a[2:]) if bstyle == "hybrid" else (bstyle, a[1:])
            if st != "zero":
                m.bond[int(a[0])] = (st,) + tuple(float(v) for v in vals)
        elif c == "angle_style":
            astyle = a[0]
        elif c == "angle_coeff":
            m.angle[int(a[0])] = (astyle,) + tuple(float(v) for v in a[1:])
        elif c == "timestep":
            m.dt = float(a[0])
        elif c == "thermo_modify":
            kw = dict(zip(a[::2], a[1::2]))
            if "norm" in kw:
                m.norm = kw["norm"] == "yes"
        elif c == "group":
            assert a[1] == "type", line
            groups[a[0]] = tuple(int(v) for v in a[2:])
        elif c == "fix" and a[2] == "nve":
            m.nve, m.nve_types = True, groups[a[1]]
        elif c == "fix" and a[2] == "langevin":
            assert a[1] == "all" and len(a) == 7, line
            m.langevin = (float(a[3]), float(a[4]), float(a[5]), int(a[6]))
            assert m.langevin[0] == m.langevin[1]
    return m


def pair_matrix(model, ntypes):
    """(eps, sigma, cut, offset) as [ntypes + 1, ntypes + 1] long-double arrays: the rows given, then mixing for the rest."""
    p = model.pair
    eps, sig, cut = (np.zeros((ntypes + 1, ntypes + 1), dtype=LD) for _ in range(3))
    given = np.zeros((ntypes + 1, ntypes + 1), dtype=bool)
    for i, j, e, s, c in p["rows"]:
        eps[i, j], sig[i, j], cut[i, j], given[i, j] = LD(e), LD(s), LD(c), True
    for i in range(1, ntypes + 1):
        assert given[i, i], "pair_coeff %d %d is not set" % (i, i)
        for j in range(i + 1, ntypes + 1):
            if given[i, j]:
                continue
            e1, e2, s1, s2 = eps[i, i], eps[j, j], sig[i, i], sig[j, j]
            if p["mix"] == "geometric":
                eps[i, j], sig[i, j], cut[i, j] = np.sqrt(e1 * e2), np.sqrt(s1 * s2), np.sqrt(cut[i, i] * cut[j, j])
            else:
                assert p["mix"] == "arithmetic"
                eps[i, j], sig[i, j], cut[i, j] = np.sqrt(e1 * e2), (s1 + s2) / 2, (cut[i, i] + cut[j, j]) / 2
    off = np.zeros_like(eps)
    for i in range(1, ntypes + 1):
        for j in range(i, ntypes + 1):
            if p["shift"] and cut[i, j] > 0:
                ratio = sig[i, j] / cut[i, j]
                off[i, j] = 4 * eps[i, j] * (ratio ** 12 - ratio ** 6)
            for arr in (eps, sig, cut, off):
                arr[j, i] = arr[i, j]
    return eps, sig, cut, off


# ------------------------------------------------------------------------------------------------
# the terms: separation vectors in, (force factor, energy) out.  force on the first bead of a term = del * factor
# ------------------------------------------------------------------------------------------------
def min_image(d, prd):
    """Closest periodic image of the separation vectors d [..., 3] (long double)."""
    half = prd / 2
    return np.where(d > half, d - prd, np.where(d < -half, d + prd, d))


def lj_terms(rsq, eps, sig, off):
    s6 = (sig * sig / rsq) ** 3
    return 24 * eps * (2 * s6 * s6 - s6) / rsq, 4 * eps * (s6 * s6 - s6) - off


def bond_terms(rsq, coeff):
    """-> (fbond, ebond, clamped)"""
    st = coeff[0]
    c = [LD(v) for v in coeff[1:]]
    clamped = np.zeros(rsq.shape, dtype=bool)
    if st == "fene":
        K, R0, eps, sig = c
        rlogarg = 1 - rsq / (R0 * R0)
        assert (rlogarg > -3).all(), "Bad FENE bond"
        clamped = rlogarg < LD("0.1")
        rlogarg = np.where(clamped, LD("0.1"), rlogarg)
        f = -K / rlogarg
        e = -K * R0 * R0 * np.log(rlogarg) / 2
        wca = rsq < TWO_1_3 * sig * sig
        s6 = (sig * sig / rsq) ** 3
        f = f + np.where(wca, 48 * eps * s6 * (s6 - LD("0.5")) / rsq, 0)
        e = e + np.where(wca, 4 * eps * s6 * (s6 - 1) + eps, 0)
    elif st == "harmonic":
        K, r0 = c
        r = np.sqrt(rsq)
        f, e = -2 * K * (r - r0) / r, K * (r - r0) ** 2
    else:
        assert st == "morse", st
        D, alpha, r0 = c
        r = np.sqrt(rsq)
        ra = np.exp(-alpha * (r - r0))
        f, e = -2 * D * alpha * (1 - ra) * ra / r, D * (1 - ra) ** 2
    return f, e, clamped


def angle_terms(d1, d2, coeff):
    """d1 = x1 - x2, d2 = x3 - x2 (x2 the vertex) -> (f1, f3, eangle, clamped); the vertex takes -(f1 + f3)."""
    rsq1, rsq2 = (d1 * d1).sum(axis=-1), (d2 * d2).sum(axis=-1)
    r1r2 = np.sqrt(rsq1) * np.sqrt(rsq2)
    c = np.clip((d1 * d2).sum(axis=-1) / r1r2, -1, 1)
    clamped = np.zeros(c.shape, dtype=bool)
    if coeff[0] == "harmonic":
        K, theta0 = LD(coeff[1]), LD(coeff[2]) / 180 * PI
        s = np.sqrt(1 - c * c)
        clamped = s < SMALL
        s = np.where(clamped, SMALL, s)
        dtheta = np.arccos(c) - theta0
        e, a = K * dtheta * dtheta, -2 * K * dtheta / s
    else:
        assert coeff[0] == "cosine", coeff[0]
        K = LD(coeff[1])
        e, a = K * (1 + c), K + 0 * c
    a11, a12, a22 = (a * c / rsq1)[..., None], (-a / r1r2)[..., None], (a * c / rsq2)[..., None]
    return a11 * d1 + a12 * d2, a22 * d2 + a12 * d1, e, clamped


def virial6(d, f):
    """sum over terms of d (x) f in the reference program's order xx yy zz xy xz yz"""
    return np.array([(d[:, a] * f[:, b]).sum() for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))], dtype=LD)


# ------------------------------------------------------------------------------------------------
# one system + one model, prepared once: the N (N - 1) / 2 candidate pairs with their coefficients
# ------------------------------------------------------------------------------------------------
Eval = collections.namedtuple("Eval", "f f_pair f_bond f_angle evdwl ebond eangle vpair vbond vangle gap gap_pair "
                                      "fene_clamped angle_clamped max_bond_frac terms")


class System:
    """types, masses, box, bonds (type, tag, tag), angles (type, tag, tag, tag) with tags = row + 1."""

    def __init__(self, model, box, types, mass, bonds, angles=None, special_from=None):
        """angles: rows, or a multiset {(type, tag, tag, tag): copies} - a duplicate counts twice, as the engines evaluate every
        stored copy.  special_from: the bonds the special levels are searched over, if not `bonds` (a deliberately stale
        table, for the tests that show a wrong level moves a force)."""
        self.model = model
        self.units = UNITS[model.units]
        self.box = np.asarray(box, dtype=np.float64)
        self.lo, self.prd = ld(self.box[:, 0]), ld(self.box[:, 1]) - ld(self.box[:, 0])
        self.types = np.asarray(types, dtype=np.int64)
        self.n = n = len(self.types)
        self.ntypes = len(mass)
        self.m = ld([mass[t - 1] for t in self.types])
        self.norm = (model.units == "lj") if model.norm is None else model.norm
        self.mobile = np.ones(n, dtype=bool) if model.nve_types is None else np.isin(self.types, model.nve_types)
        if model.pair is not None:
            self.pair_coeffs = pair_matrix(model, self.ntypes)
            self.cutmax = float(self.pair_coeffs[2].max())
        self.set_topology(bonds, angles, special_from)

    def set_topology(self, bonds, angles=None, special_from=None):
        """The bonds, the angles and the pair weights that follow from the bond graph (the candidate pairs with them)."""
        model, n = self.model, self.n
        graph = np.asarray(bonds if special_from is None else special_from).reshape(-1, 3)
        self.bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 3)
        self.bonds = self.bonds[[model.bond.get(int(t), ("zero",))[0] != "zero" for t in self.bonds[:, 0]]] if len(self.bonds) else self.bonds
        if isinstance(angles, dict):
            angles = [row for row, copies in sorted(angles.items()) for _ in range(copies)]
        self.angles = np.zeros((0, 4), dtype=np.int64) if angles is None or not model.angle else np.asarray(angles, dtype=np.int64).reshape(-1, 4)
        if model.pair is not None:
            eps, sig, cut, off = self.pair_coeffs
            iu, ju = np.triu_indices(n, 1)
            w = np.ones(len(iu), dtype=LD)
            sp = reference_specials(n, graph)          # (all bonds of the table: the graph, not the styles)
            pos = {}
            for a, lv in sp.items():
                for b, level in lv.items():
                    if a < b:
                        pos[(a - 1, b - 1)] = level
            if pos:
                keys = np.array(list(pos.keys()))
                flat = keys[:, 0] * n - keys[:, 0] * (keys[:, 0] + 1) // 2 + keys[:, 1] - keys[:, 0] - 1     # row of (i, j) in triu order
                w[flat] = ld([model.special_lj[v - 1] for v in pos.values()])
            self.multi_image = float(self.prd.min()) < 2 * self.cutmax          # more than one image of a partner within the cutoff
            # a pair whose closest image has weight 0 is in no list and exerts no force: it is no candidate - unless farther
            # images of the partner can lie within the cutoff, which are ordinary neighbors (evaluate gives it weight 0 at
            # the closest image alone)
            keep = (w != 0) | self.multi_image
            self.iu, self.ju, self.w = iu[keep], ju[keep], w[keep]
            ti, tj = self.types[self.iu], self.types[self.ju]
            self.p_eps, self.p_sig, self.p_off = eps[ti, tj], sig[ti, tj], off[ti, tj]
            self.p_cut = cut[ti, tj]
            self.p_cutsq = self.p_cut * self.p_cut

    # -- forces --
    def evaluate(self, x, only=None):
        """Forces, energies, virials at the positions x (inside the box).  only = a row: just the terms that bead takes part
        in (their energy is all the finite-difference test needs)."""
        x = ld(x)
        n, prd = self.n, self.prd
        f_pair, f_bond, f_angle = (np.zeros((n, 3), dtype=LD) for _ in range(3))
        evdwl = ebond = eangle = LD(0)
        vpair, vbond, vangle = (np.zeros(6, dtype=LD) for _ in range(3))
        gap, gap_pair, terms = LD(np.inf), None, {}
        if self.model.pair is not None:
            sel = slice(None) if only is None else np.nonzero((self.iu == only) | (self.ju == only))[0]
            iu, ju = self.iu[sel], self.ju[sel]
            d0 = min_image(x[iu] - x[ju], prd)
            shifts = [np.zeros(3, dtype=LD)]
            if self.multi_image:
                shifts += [ld(s) * prd for s in (np.array(t) - 1 for t in np.ndindex(3, 3, 3)) if s.any()]
            for k, sh in enumerate(shifts):
                d = d0 + sh
                rsq = (d * d).sum(axis=1)
                g = np.abs(rsq - self.p_cutsq[sel])
                if k == 0:
                    g = np.where(self.w[sel] != 0, g, LD(np.inf))          # (closest images of weight 0 are no candidates)
                if len(g) and g.min() < gap:
                    q = int(np.argmin(g))
                    gap, gap_pair = g[q], (int(iu[q]), int(ju[q]), float(self.p_cut[sel][q]))
                hit = np.nonzero((rsq < self.p_cutsq[sel]) & ((self.w[sel] != 0) if k == 0 else True))[0]
                fp, e = lj_terms(rsq[hit], self.p_eps[sel][hit], self.p_sig[sel][hit], self.p_off[sel][hit])
                wt = self.w[sel][hit] if k == 0 else LD(1)          # the special weight belongs to the closest image alone
                fp, e = fp * wt, e * wt
                fv = d[hit] * fp[:, None]
                np.add.at(f_pair, iu[hit], fv)
                np.add.at(f_pair, ju[hit], -fv)
                evdwl += e.sum()
                vpair += virial6(d[hit], fv)
                if k == 0:
                    terms["pair"] = (iu[hit], ju[hit], d[hit], fv)
        fene_clamped, max_frac = [], 0.0
        half_min = self.prd.min() / 2
        if len(self.bonds):
            b = self.bonds if only is None else self.bonds[(self.bonds[:, 1] == only + 1) | (self.bonds[:, 2] == only + 1)]
            i1, i2 = b[:, 1] - 1, b[:, 2] - 1
            d = min_image(x[i1] - x[i2], prd)
            rsq = (d * d).sum(axis=1)
            if len(b):
                max_frac = float(np.sqrt(rsq.max()) / half_min)
            fv = np.zeros((len(b), 3), dtype=LD)
            for bt in np.unique(b[:, 0]):
                k = np.nonzero(b[:, 0] == bt)[0]
                fb, e, cl = bond_terms(rsq[k], self.model.bond[int(bt)])
                fv[k] = d[k] * fb[:, None]
                ebond += e.sum()
                fene_clamped += [(int(i1[q]) + 1, int(i2[q]) + 1) for q in k[cl]]
            np.add.at(f_bond, i1, fv)
            np.add.at(f_bond, i2, -fv)
            vbond += virial6(d, fv)
            terms["bond"] = (i1, i2, d, fv)
        angle_clamped = []
        if len(self.angles):
            a = self.angles if only is None else self.angles[((self.angles[:, 1:] - 1) == only).any(axis=1)]
            i1, i2, i3 = a[:, 1] - 1, a[:, 2] - 1, a[:, 3] - 1
            d1, d2 = min_image(x[i1] - x[i2], prd), min_image(x[i3] - x[i2], prd)
            if len(a):
                max_frac = max(max_frac, float(np.sqrt(max((d1 * d1).sum(axis=1).max(), (d2 * d2).sum(axis=1).max())) / half_min))
            f1, f3 = np.zeros((len(a), 3), dtype=LD), np.zeros((len(a), 3), dtype=LD)
            for at in np.unique(a[:, 0]):
                k = np.nonzero(a[:, 0] == at)[0]
                f1[k], f3[k], e, cl = angle_terms(d1[k], d2[k], self.model.angle[int(at)])
                eangle += e.sum()
                angle_clamped += [tuple(int(v) for v in a[q, 1:]) for q in k[cl]]
            np.add.at(f_angle, i1, f1)
            np.add.at(f_angle, i3, f3)
            np.add.at(f_angle, i2, -(f1 + f3))
            vangle += virial6(d1, f1) + virial6(d2, f3)
            terms["angle"] = (i1, i2, i3, d1, d2, f1, f3)
        # every bond (and angle leg) below half the shortest box edge: the closest image is the image the reference
        # program froze at its last reneighbor, whenever that was
        assert max_frac < 1.0, "a bond or angle leg reaches half the shortest box edge (%.3f of it)" % max_frac
        return Eval(f_pair + f_bond + f_angle, f_pair, f_bond, f_angle, evdwl, ebond, eangle, vpair, vbond, vangle, gap,
                    gap_pair, fene_clamped, angle_clamped, max_frac, terms)

    # -- thermo --
    def thermo(self, ev, v, norm=None):
        """The thermo keywords of one step from an evaluation and the velocities of that step (norm: thermo_modify norm, if
        not the script's)."""
        u, n = self.units, self.n
        v = ld(v)
        mv = self.m[:, None] * v
        k6 = np.array([(mv[:, a] * v[:, b]).sum() for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))], dtype=LD) * LD(u["mvv2e"])
        dof = LD(3 * n - 3)
        temp = (k6[0] + k6[1] + k6[2]) / (dof * LD(u["boltz"]))
        ke = temp * dof * LD(u["boltz"]) / 2
        vol = self.prd[0] * self.prd[1] * self.prd[2]
        vir = ev.vpair + ev.vbond + ev.vangle
        press = (dof * LD(u["boltz"]) * temp + vir[0] + vir[1] + vir[2]) / 3 / vol * LD(u["nktv2p"])
        pt = (k6 + vir) / vol * LD(u["nktv2p"])
        norm = LD(n) if (self.norm if norm is None else norm) else LD(1)
        emol = ev.ebond + ev.eangle
        out = dict(temp=temp, press=press, evdwl=ev.evdwl / norm, epair=ev.evdwl / norm, ebond=ev.ebond / norm, eangle=ev.eangle / norm,
                   emol=emol / norm, pe=(ev.evdwl + emol) / norm, ke=ke / norm, etotal=(ke + ev.evdwl + emol) / norm)
        out.update(zip(("pxx", "pyy", "pzz", "pxy", "pxz", "pyz"), pt))
        return out

    # -- integration --
    def langevin_force(self, v, u3):
        """gamma1 v + gamma2 (u - 0.5): u3 = this call's 3 N uniform draws, three per bead in tag order."""
        t0, _, damp, _ = self.model.langevin
        u = self.units
        g1 = -self.m / LD(damp) / LD(u["ftm2v"])
        g2 = np.sqrt(self.m) * np.sqrt(24 * LD(u["boltz"]) / LD(damp) / LD(self.model.dt) / LD(u["mvv2e"])) / LD(u["ftm2v"]) * np.sqrt(LD(t0))
        return g1[:, None] * v + g2[:, None] * (ld(u3).reshape(self.n, 3) - LD("0.5"))

    def wrap(self, x, img):
        for d in range(3):
            lo, hi, prd = self.lo[d], self.lo[d] + self.prd[d], self.prd[d]
            m = x[:, d] < lo
            x[m, d] += prd; img[m, d] -= 1
            m = x[:, d] >= hi
            x[m, d] -= prd; img[m, d] += 1

    def unwrapped(self, x, img):
        return ld(x) + ld(img) * self.prd

    def trajectory(self, x0, v0, img0, nsteps, uniforms=None, topology=None, extra=None, after=None):
        """Velocity Verlet from the state read_data leaves (x0 inside the box, image flags img0): setup, then nsteps steps.
        Returns per step (0 .. nsteps) the unwrapped positions, velocities, thermo rows and min |r^2 - cut^2|, and the
        force array of the last step (with the Langevin force, as the engine's f holds it).
        topology(step) -> (bonds, angles): the tables in force at the force evaluation of `step` (a fix that edits them does so
        between the position update and that evaluation); where the answer differs from the previous step's, the bonds, the
        angles and the pair weights are rebuilt before the evaluation.  Without it the topology is static.
        extra(step, x, img, f) -> f: the hook for force terms of other modules (a wall, an indenter, a tether, a pull) - it takes
        the positions inside the box, the image flags and the force of the model's own terms at the evaluation of `step` and
        returns the force with its terms added, before the thermostat's.  The thermo rows stay the model's own (a fix enters
        them only under fix_modify).
        after(step, x, img, f) -> f: the same for the terms of fixes defined behind the thermostat - it takes the force with the
        thermostat's in it (a fix setforce there overwrites that too)."""
        assert self.model.nve
        x, v, img = ld(x0).copy(), ld(v0).copy(), np.asarray(img0, dtype=np.int64).copy()
        dt = LD(self.model.dt)
        dtfm = (dt / 2 * LD(self.units["ftm2v"]) / self.m)[:, None]
        mob = self.mobile[:, None]
        n3 = 3 * self.n
        xs, vs, rows, gaps, fracs = [], [], [], [], []

        held = [None]

        def forces(step):
            if topology is not None:
                bonds, angles = topology(step)
                key = (sorted(map(tuple, np.asarray(bonds).reshape(-1, 3).tolist())),
                       sorted(angles.items()) if isinstance(angles, dict) else None if angles is None else sorted(map(tuple, np.asarray(angles).reshape(-1, 4).tolist())))
                if key != held[0]:
                    self.set_topology(bonds, angles)
                    held[0] = key
            ev = self.evaluate(x)
            f = ev.f if extra is None else extra(step, x, img, ev.f)
            if self.model.langevin:
                f = f + self.langevin_force(v, uniforms[step * n3:(step + 1) * n3])
            if after is not None:
                f = after(step, x, img, f)
            return ev, f

        ev, f = forces(0)
        for step in range(nsteps + 1):
            if step:
                v = np.where(mob, v + dtfm * f, v)
                x = np.where(mob, x + dt * v, x)
                self.wrap(x, img)
                ev, f = forces(step)
                v = np.where(mob, v + dtfm * f, v)
            xs.append(self.unwrapped(x, img)); vs.append(v.copy()); rows.append(self.thermo(ev, v)); gaps.append(ev.gap)
            fracs.append(ev.max_bond_frac)
        return dict(x=xs, v=vs, rows=rows, gaps=gaps, f=f, xw=x, img=img, fracs=fracs, last=ev)
