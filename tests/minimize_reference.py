"""`minimize` in long double over the brute-force energies and forces of force_reference.py (soft_reference.py for the soft pair
term, wall_reference.py and extforce_reference.py for the fixes with a minimisation hook): min_style cg | sd with the
backtracking and the quadratic line search, written from the description of the algorithm - steepest descent or Polak-Ribiere
directions with a restart when the direction is not downhill, a step limit of dmax / max|h|, a line search that halves alpha
until the energy drop is at least 0.4 alpha f.h and, in the quadratic form, first tries the secant step to f.h = 0 when the
energy change agrees with the trapezoid of the two slopes to 10 % - and sharing nothing with the engine.

The displacement test of the neighbour list (a bead farther than skin / 2 from where the last build found it) is kept, because
a build is when beads outside the box are wrapped and their image flags and stored start coordinates move with them: the walls
see stored coordinates.  `run(scn, system)` returns the thermo rows (pe, epair, emol, fmax, fnorm, the fixes' energies), the counts, the stop index,
the list builds, which exit every line search took, and the end state."""
import numpy as np

import force_reference as fr
import minimize_runs as mn

LD = np.longdouble
ALPHA_MAX, ALPHA_REDUCE, BACKTRACK_SLOPE, QUADRATIC_TOL, EMACH, EPS_QUAD, EPS_ENERGY = LD(1), LD("0.5"), LD("0.4"), LD("0.1"), LD("1e-8"), LD("1e-28"), LD("1e-8")
ROW = ("pe", "epair", "emol", "fmax", "fnorm")


class Model:
    """Energy and forces of a scenario at stored coordinates (x, image flags), the fixes included."""

    def __init__(self, scn, system):
        self.scn, self.s = scn, system
        text = scn["head"] + "run 0\n"          # (styles and coefficients; the lines of `before` are read here, not by the force model)
        s = system
        if "pair_style soft" in text:
            import soft_reference as sr
            model = fr.model_from_script(text.replace("pair_style soft 1.12246\npair_coeff * * 30.0\n", "pair_style zero 1.12246\n"), s["ntypes"])
            model.pair = sr.soft_model_pair(1.12246, [(1, 1, 30.0)])
            self.S = sr.SoftSystem(model, s["box"], s["type"], s["mass"], s["bonds"])
        else:
            self.S = fr.System(fr.model_from_script(text, s["ntypes"]), s["box"], s["type"], s["mass"], s["bonds"], s.get("angles"))
        S = self.S
        self.n = S.n
        self.lo, self.prd = S.lo, S.prd
        self.all_pairs = (S.iu, S.ju, S.w, S.p_eps, S.p_sig, S.p_off, S.p_cut, S.p_cutsq)
        self.key = S.iu.astype(np.int64) * S.n + S.ju
        lines = [ln.split() for ln in scn["before"].split("\n") if ln.split()]
        self.frozen = any(w[0] == "fix" and w[3] == "setforce" and w[2] == "all" for w in lines)
        self.confined = scn["name"] == "confined_tethered"
        self.norm = LD(1) if "norm no" in scn["modify"] else LD(S.n)
        self.last_add = LD(0)

    def wrapped(self, x):
        return self.lo + np.mod(x - self.lo, self.prd)

    def evaluate(self, x, image, step):
        """-> dict(f, pe, epair, emol) with the energies as thermo prints them"""
        from scipy.spatial import cKDTree
        S, xw = self.S, self.wrapped(x)
        # the candidate pairs of this evaluation: those within the cutoff and a margin, found in double; the terms in long double
        y = np.mod(np.asarray(xw, dtype=np.float64) - np.asarray(self.lo, dtype=np.float64), np.asarray(self.prd, dtype=np.float64))
        y = np.where(y >= np.asarray(self.prd, dtype=np.float64), 0.0, y)
        pairs = cKDTree(y, boxsize=np.asarray(self.prd, dtype=np.float64)).query_pairs(S.cutmax + 0.05, output_type="ndarray")
        lo_, hi_ = np.minimum(pairs[:, 0], pairs[:, 1]).astype(np.int64), np.maximum(pairs[:, 0], pairs[:, 1])
        k = np.nonzero(np.isin(self.key, lo_ * S.n + hi_))[0]
        S.iu, S.ju, S.w, S.p_eps, S.p_sig, S.p_off, S.p_cut, S.p_cutsq = (a[k] for a in self.all_pairs)
        try:
            ev = S.evaluate(xw)
        finally:
            S.iu, S.ju, S.w, S.p_eps, S.p_sig, S.p_off, S.p_cut, S.p_cutsq = self.all_pairs
        f, efix, out = ev.f, LD(0), {}
        if self.confined:
            f, e = confined_fixes(self.scn, self.s, x, image, f, step)
            # (an addforce that skips this step keeps the energy of the last step on which it acted, and reports it)
            self.last_add = e["f_a"] if e["f_a"] is not None else self.last_add
            e["f_a"] = self.last_add
            efix = e["f_w"] + e["f_s"] + e["f_a"]          # (fix_modify energy yes on w, s and a; w2 has none)
            out = {k: v / self.norm for k, v in e.items()}
        if self.frozen:
            f = np.zeros_like(f)
        emol = ev.ebond + ev.eangle
        out["eangle"] = ev.eangle / self.norm
        return dict(out, f=f, pe=(ev.evdwl + emol + efix) / self.norm, epair=ev.evdwl / self.norm, emol=emol / self.norm)


def confined_fixes(scn, s, x, image, f, step):
    """The two walls and the tether, pull and pinned group of confined_tethered on the forces f at the stored coordinates x, in
    fix order -> (forces, the energy every fix reports: f_w, f_w2, f_s, f_a - None on a step the addforce skips)."""
    import extforce_reference as er
    import wall_reference as wr
    lines = [ln.split() for ln in scn["before"].split("\n") if ln.split()]
    regions = {w[1]: wr.parse_region(w[2:]) for w in lines if w[0] == "region"}
    n, energy = len(x), {}
    f = np.asarray(f, dtype=LD).copy()
    for w in lines:
        if w[0] == "fix" and w[3] == "wall/region":
            t = wr.wall_terms(x, regions[w[4]], wr.parse_wall(w[5:]))
            assert not t["outside"].any()
            f += t["f"]
            energy["f_" + w[1]] = t["energy"]
    member = {nm: er.members(n, list(range(a, n + 1, b))) for nm, a, b in (("teth", 20, 20), ("pull", 10, 40), ("pin", 7, 50))}
    origin = er.unwrapped(s["x"], s["image"], s["box"])          # (the tethers' origins: where the fix command found the beads)
    fixes = [er.spring(10.0, member["teth"], origin), er.add((0.5, -0.25, 0.75), member["pull"], every=3), er.setforce((None, 0.0, 0.0), member["pin"])]
    f, out = er.apply(fixes, x, image, s["box"], f, step=step)
    energy["f_s"], energy["f_a"] = out[0]["energy"], (out[1]["energy"] if out[1] is not None else None)
    return f, energy


def columns(scn):
    """The thermo columns the rows of run() hold behind the step."""
    return ROW + (("f_w", "f_w2", "f_s", "f_a") if scn["name"] == "confined_tethered" else ()) + (("eangle",) if "eangle" in scn["extra_columns"] else ())


def start(scn, system):
    """Stored coordinates of the start: the data file's, with the script's `set atom` lines applied."""
    x = np.array(system["x"], dtype=LD)
    for w in (ln.split() for ln in scn["before"].split("\n")):
        if w[:2] == ["set", "atom"]:
            for name, val in zip(w[3::2], w[4::2]):
                x[int(w[2]) - 1, "xyz".index(name)] = LD(val)
    return x


def run(scn, system, skin=0.4):
    etol, ftol, maxiter, maxeval = (LD(v) if k < 2 else v for k, v in enumerate(mn.minimize_args(scn)))
    words = scn["before"].split()
    cg = "sd" not in [words[i + 1] for i, w in enumerate(words) if w == "min_style"]
    backtrack = "backtrack" in words
    norm = ([words[i + 1] for i, w in enumerate(words) if w == "norm"] or ["two"])[-1]
    dmax = LD(([words[i + 1] for i, w in enumerate(words) if w == "dmax"] or ["0.1"])[-1])
    M = Model(scn, system)
    natoms = LD(M.n) if M.norm != 1 else LD(1)
    st = dict(x=start(scn, system), image=np.array(system["image"], dtype=np.int64), step=0, neval=0, builds=0, exits=[])
    st["hold"] = st["x"].copy()
    trigger = LD(skin) * LD(skin) / 4
    every = scn["thermo"]

    def energy_force(x0=None):
        d = st["x"] - st["hold"]
        if ((d * d).sum(axis=1) > trigger).any():          # a list build: wrap, and the stored start coordinates follow
            shift = np.floor((st["x"] - M.lo) / M.prd)
            st["x"] = st["x"] - shift * M.prd
            st["image"] = st["image"] + shift.astype(np.int64)
            if x0 is not None:
                x0 -= shift * M.prd
            st["hold"] = st["x"].copy()
            st["builds"] += 1
        st["ev"] = M.evaluate(st["x"], st["image"], st["step"])
        return st["ev"]["pe"]

    names = columns(scn)

    def row():
        f = st["ev"]["f"]
        return [st["step"]] + [float(st["ev"][k]) for k in ROW[:3]] + [float(np.abs(f).max()), float(np.sqrt((f * f).sum()))] + \
               [float(st["ev"][k]) for k in names[len(ROW):]]

    ecurrent = energy_force()
    rows = [row()]
    f = st["ev"]["f"]
    g, h = f.copy(), f.copy()
    gg = (f * f).sum()
    niter, stop, alpha_final, eprevious = 0, mn.MAXITER, LD(0), ecurrent

    def linemin(eoriginal):
        """-> (stop or 0, alpha)"""
        nonlocal ecurrent
        fdoth = (st["ev"]["f"] * h).sum() / natoms
        if fdoth <= 0:
            return mn.DOWNHILL, LD(0)
        hmax = np.abs(h).max()
        alphamax = min(ALPHA_MAX, dmax / hmax) if hmax > 0 else ALPHA_MAX
        if hmax == 0:
            return mn.ZEROFORCE, alphamax
        x0 = st["x"].copy()

        def step_to(a):
            nonlocal ecurrent
            st["x"] = x0 + a * h if a > 0 else x0.copy()
            st["neval"] += 1
            ecurrent = energy_force(x0)

        alpha, fhprev, engprev, alphaprev = alphamax, fdoth, eoriginal, LD(0)
        while True:
            step_to(alpha)
            if not backtrack:
                fh = (st["ev"]["f"] * h).sum() / natoms
                delfh = fh - fhprev
                if abs(fh) < EPS_QUAD or abs(delfh) < EPS_QUAD:
                    step_to(LD(0))
                    return mn.ZEROQUAD, alpha
                relerr = abs(1 - (LD("0.5") * (alpha - alphaprev) * (fh + fhprev) + ecurrent) / engprev)
                alpha0 = alpha - (alpha - alphaprev) * fh / delfh
                if relerr <= QUADRATIC_TOL and 0 < alpha0 < alphamax:
                    step_to(alpha0)
                    if ecurrent - eoriginal < EMACH:
                        st["exits"].append("quadratic")
                        return 0, alpha
            de_ideal = -BACKTRACK_SLOPE * alpha * fdoth
            de = ecurrent - eoriginal
            if de <= de_ideal:
                st["exits"].append("backtrack" if alpha < alphamax else "alphamax")
                return 0, alpha
            if not backtrack:
                fhprev, engprev, alphaprev = fh, ecurrent, alpha
            alpha = alpha * ALPHA_REDUCE
            if alpha <= 0 or de_ideal >= -EMACH:
                step_to(LD(0))
                return (mn.ETOL if (backtrack and de < 0) else mn.ZEROALPHA), alpha

    for it in range(maxiter):
        st["step"] += 1
        niter += 1
        eprevious = ecurrent
        fail, alpha_final = linemin(ecurrent)
        if fail:
            stop = fail
            break
        if st["neval"] >= maxeval:
            stop = mn.MAXEVAL
            break
        if abs(ecurrent - eprevious) < etol * LD("0.5") * (abs(ecurrent) + abs(eprevious) + EPS_ENERGY):
            stop = mn.ETOL
            break
        f = st["ev"]["f"]
        ff, fg = (f * f).sum(), (f * g).sum()
        if ftol > 0:
            fdotf = (f * f).sum(axis=1).max() if norm == "max" else (np.abs(f).max() ** 2 if norm == "inf" else ff)
            if fdotf < ftol * ftol:
                stop = mn.FTOL
                break
        if cg:
            beta = max(LD(0), (ff - fg) / gg)
            if (niter + 1) % (3 * M.n) == 0:
                beta = LD(0)
            gg = ff
            g = f.copy()
            h = g + beta * h
            if (g * h).sum() <= 0:
                h = g.copy()
        else:
            h = f.copy()
        if st["step"] % every == 0 or st["step"] == maxiter:
            rows.append(row())
    if stop != mn.MAXITER:          # the row of the iteration reached, after one more evaluation
        energy_force()
        rows.append(row())
    return dict(rows=np.array(rows), iterations=niter, evals=st["neval"], stop=stop, builds=st["builds"], exits=st["exits"],
                x=np.asarray(st["x"], dtype=np.float64), image=st["image"], alpha=float(alpha_final))
