"""The runs of the launch-census matrix (test_gpu_step_census.py) that nothing else in the suite had: twelve steps of the input
`census` of force_inputs.py (2145 beads) with a wall, an indenter, a tether and a pull, pair_style soft, or no pair style, with
and without fix langevin - each against force_reference.System.trajectory with the term of wall_reference, indent_reference,
extforce_reference or soft_reference added through its `extra` hook.  No GPU here: test_step_census_cpu.py checks the inputs
from these references alone.

The oracle has none of these terms.  What enters force_compare.bound in its place is the deviation of the same restatement
run in float64 (force_reference.precision) from the long-double run.

Candidate pairs: the reference measures every pair of beads at every step - 2.3 million of them here, most of them a box
apart.  PrunedSystem keeps the pairs that start within cutoff + REACH of each other (measured once, in long double, over all
pairs) and the test asserts that no bead moves REACH / 2 in the twelve steps: a pair outside the set cannot reach the cutoff."""
import functools

import numpy as np

import extforce_reference as er
import force_compare as fc
import force_inputs as fi
import force_reference as fr
import indent_reference as ir
import soft_reference as sr
import wall_reference as wr
from neigh_reference import reference_specials
from systems import wrap_into_box

NAME = "census"
SKIN = 0.2
THERMO = 4
REACH = 2.0
SOFT_CUT, SOFT_A = 1.12246, 12.0
WALL = dict(style="lj126", epsilon=1e-5, sigma=2.0, cutoff=2.24)          # the wall of test_gpu_wall_steps.py: repulsive throughout
BALL_RADIUS = 0.05
INDENT_K, INDENT_DEPTH = 10.0, 0.6                                         # the indenter reaches INDENT_DEPTH past the nearest bead
TETHER_K, PULL = 10.0, (0.5, -0.25, 0.75)
FAMILIES = ("wall", "soft", "ext", "indent", "nopair")
LANGEVIN = "fix 2 all langevin 1.0 1.0 1.0 %d\n" % fc.LANGEVIN_SEED


def system():
    return fi.INPUTS[NAME]()["system"]


@functools.lru_cache(maxsize=None)
def hole():
    """(a point far from every bead of the start - by the minimum image, the indenter's own measure -, its distance to the
    nearest bead): the best point of a 0.4 grid, then of a 0.1 grid around it."""
    s = system()
    x, _ = wrap_into_box(s)
    box = np.asarray(s["box"], dtype=np.float64)
    prd = box[:, 1] - box[:, 0]
    keep = BALL_RADIUS + WALL["cutoff"] + 0.2          # (the wall's reach stays inside the box: it has no minimum image)

    def best_of(axes):
        g = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
        r = np.empty(len(g))
        for lo in range(0, len(g), 512):
            d = g[lo:lo + 512, None, :] - x[None, :, :]
            d -= prd * np.round(d / prd)
            r[lo:lo + 512] = np.sqrt((d ** 2).sum(axis=2)).min(axis=1)
        k = int(np.argmax(r))
        return g[k], float(r[k])
    coarse, _ = best_of([np.arange(box[d, 0] + keep, box[d, 1] - keep, 0.4) for d in range(3)])
    where, best = best_of([np.clip(coarse[d] + 0.1 * np.arange(-4, 5), box[d, 0] + keep, box[d, 1] - keep) for d in range(3)])
    return tuple(float(c) for c in where), best


def indenter():
    c, r = hole()
    return dict(kind="sphere", K=INDENT_K, side="out", ctr=list(c), R=r + INDENT_DEPTH)


def wall_region():
    c, _ = hole()
    return dict(style="sphere", side="out", args=(c[0], c[1], c[2], BALL_RADIUS))


def family_lines(family):
    """(force field, the fix lines between fix nve and fix langevin) of a family"""
    ff = fi.INPUTS[NAME]()["force_field"]
    c, _ = hole()
    if family == "wall":
        return ff, ("region hole sphere %.17g %.17g %.17g %.17g side out\n" % (c[0], c[1], c[2], BALL_RADIUS) +
                    "fix w all wall/region hole lj126 %.17g %.17g %.17g\n" % (WALL["epsilon"], WALL["sigma"], WALL["cutoff"]))
    if family == "indent":
        o = indenter()
        return ff, "fix c all indent %.17g sphere %.17g %.17g %.17g %.17g side out\n" % (o["K"], c[0], c[1], c[2], o["R"])
    if family == "ext":
        return ff, "fix s all spring/self %.17g\nfix a all addforce %.17g %.17g %.17g\n" % ((TETHER_K,) + PULL)
    if family == "soft":
        return fi.FENE + "pair_style soft %.17g\npair_coeff * * %.17g\n" % (SOFT_CUT, SOFT_A), ""
    assert family == "nopair"
    return fi.FENE + "pair_style zero %.17g\npair_coeff * *\n" % 1.12, ""


def script(family, langevin, thermo=THERMO, steps=fc.STEPS, head=""):
    ff, fixes = family_lines(family)
    case = dict(fi.INPUTS[NAME](), force_field=ff)
    return (fi.script(case, skin=repr(SKIN)) + head + "fix 1 all nve\n" + fixes + (LANGEVIN if langevin else "") +
            "thermo %d\nrun %d\n" % (thermo, steps))


# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def candidates():
    """(iu, ju) of the pairs of beads that start within the largest cutoff + REACH of each other, in the order of
    np.triu_indices; long double, every pair measured."""
    s = system()
    x, _ = wrap_into_box(s)
    box = np.asarray(s["box"], dtype=np.float64)
    prd = fr.ld(box[:, 1]) - fr.ld(box[:, 0])
    x = fr.ld(x)
    n = len(x)
    lim = fr.LD(max(SOFT_CUT, 1.12) + REACH) ** 2
    iu, ju = [], []
    for i in range(n - 1):
        d = fr.min_image(x[i + 1:] - x[i], prd)
        j = np.nonzero((d * d).sum(axis=1) < lim)[0] + i + 1
        iu.append(np.full(len(j), i, dtype=np.int64)); ju.append(j)
    return np.concatenate(iu), np.concatenate(ju)


class Pruned:
    """force_reference.System over candidates() instead of every pair."""

    def set_topology(self, bonds, angles=None, special_from=None):
        model, n = self.model, self.n
        pair, model.pair = model.pair, None
        try:
            super().set_topology(bonds, angles, special_from)          # bonds and angles
        finally:
            model.pair = pair
        if pair is None:
            return
        eps, sig, cut, off = self.pair_coeffs
        iu, ju = candidates()
        w = np.ones(len(iu), dtype=fr.LD)
        flat = iu * n + ju
        graph = np.asarray(bonds if special_from is None else special_from).reshape(-1, 3)
        for a, lv in reference_specials(n, graph).items():
            for b, level in lv.items():
                if a < b:
                    q = np.searchsorted(flat, (a - 1) * n + (b - 1))
                    if q < len(flat) and flat[q] == (a - 1) * n + (b - 1):
                        w[q] = model.special_lj[level - 1]
                    else:          # (three stretched bonds apart: out of reach, and its weight must not matter)
                        assert model.special_lj[level - 1] == 1.0, "a special pair with a weight of its own is no candidate"
        self.multi_image = float(self.prd.min()) < 2 * self.cutmax
        assert not self.multi_image
        keep = w != 0
        self.iu, self.ju, self.w = iu[keep], ju[keep], w[keep]
        ti, tj = self.types[self.iu], self.types[self.ju]
        self.p_eps, self.p_sig, self.p_off = eps[ti, tj], sig[ti, tj], off[ti, tj]
        self.p_cut = cut[ti, tj]
        self.p_cutsq = self.p_cut * self.p_cut


class PrunedSystem(Pruned, fr.System):
    pass


class PrunedSoft(Pruned, sr.SoftSystem):
    pass


def _trajectory(family, langevin):
    """One run of the restatement in the precision in force (force_reference.precision).  family "together": the families in
    one run, `langevin` = the run style ("verlet" | "respa")."""
    if family == "together":
        return _together(langevin)
    from oracle import ranmars_stream
    s = system()
    model = fr.model_from_script(script("nopair" if family == "soft" else family, langevin), s["ntypes"])
    if family == "soft":
        model.pair = sr.soft_model_pair(SOFT_CUT, [(1, 1, SOFT_A)])
    S = (PrunedSoft if family == "soft" else PrunedSystem)(model, s["box"], s["type"], s["mass"], s["bonds"])
    x0, img0 = wrap_into_box(s)
    acting = []
    ext = None
    if family == "ext":
        every = np.ones(S.n, dtype=bool)
        ext = [er.spring(TETHER_K, every, er.unwrapped(x0, img0, s["box"])), er.add(PULL, every)]

    def extra(step, x, img, f):
        if family == "wall":
            t = wr.wall_terms(x, wall_region(), WALL)
            assert not t["outside"].any(), "a bead inside the ball"
            acting.append((int((t["ncontact"] > 0).sum()), float(np.abs(t["f"]).max())))
            return f + t["f"]
        if family == "indent":
            t = ir.terms(x, indenter(), s["box"])
            acting.append((int(t["touched"].sum()), float(np.abs(t["f"]).max())))
            return f + t["f"]
        if family == "ext":
            out, _ = er.apply(ext, x, img, s["box"], f, step)
            acting.append((S.n, float(np.abs(fr.ld(out) - fr.ld(f)).max())))
            return out
        return f

    u = ranmars_stream(fc.LANGEVIN_SEED, 3 * S.n * (fc.STEPS + 1)) if langevin else None
    tr = S.trajectory(x0, s["v"], img0, fc.STEPS, u, extra=extra if family in ("wall", "indent", "ext") else None)
    tr["acting"] = acting
    return S, tr


# ------------------------------------------------------------------------------------------------------------------
# The post-force families together (test_gpu_postforce_together.py): the wall, a tether on a group and a pull with `every 3`
# ahead of fix langevin, the indenter and a pinned group behind it, through the three callers of the engine's post-force
# sequence.  Under run_style respa the engine refuses fix setforce (FixForceOp::init): that run goes without the pinned group.
# The minimiser ignores the thermostat; its line stays in the script, so the indenter and the pinned group keep their place.
MODES = ("verlet", "respa", "minimize")
TETHERED, PINNED = (200, 900), (40, 47)          # ranges of IDs, both ends included
PIN = (0.0, None, 0.25)
PULL_EVERY = 3
RESPA_INNER = 2
FIX_COLUMNS = {"w": 3, "s": 0, "a": 3, "c": 3, "z": -3}          # fix ID -> length of its vector (negative: it has no scalar)


def fix_columns(mode):
    """The f_ID / f_ID[k] thermo columns of the run's fixes, in fix order."""
    out = []
    for fid, nvec in FIX_COLUMNS.items():
        if fid == "z" and mode == "respa":
            continue
        out += ["f_" + fid] * (nvec >= 0) + ["f_%s[%d]" % (fid, k + 1) for k in range(abs(nvec))]
    return out


def together_script(mode, log=None):
    ff, wall = family_lines("wall")
    _, indent = family_lines("indent")
    text = fi.script(dict(fi.INPUTS[NAME](), force_field=ff), skin=repr(SKIN))
    text += "group teth id <> %d %d\ngroup pin id <> %d %d\n" % (TETHERED + PINNED)
    text += "fix 1 all nve\n" + wall + "fix s teth spring/self %.17g\n" % TETHER_K
    text += "fix a all addforce %.17g %.17g %.17g every %d\n" % (PULL + (PULL_EVERY,)) + LANGEVIN + indent
    if mode != "respa":
        text += "fix z pin setforce %s\n" % " ".join("NULL" if c is None else repr(c) for c in PIN)
    text += "fix_modify w energy yes\nfix_modify c energy yes\nfix_modify a energy yes\n"
    text += "thermo_style custom step temp epair emol etotal press pe %s\nthermo_modify format float %%.17g\n" % " ".join(fix_columns(mode))
    text += "thermo %d\n" % THERMO + ("log %s\n" % log if log else "")
    if mode == "respa":
        text += "run_style respa 2 %d\n" % RESPA_INNER
    return text + ("minimize 0.0 0.0 %d 1000\n" % fc.STEPS if mode == "minimize" else "run %d\n" % fc.STEPS)


class Together:
    """The five fixes on the forces of one evaluation, in fix order: ahead() of the thermostat, behind() it.  efix = what
    `fix_modify energy yes` adds to pe at the last evaluation (an addforce that skipped it keeps what it last reported)."""

    def __init__(self, s, x0, img0, pinned=True):
        n = len(x0)
        self.box, self.pinned = s["box"], pinned
        self.teth = er.members(n, range(TETHERED[0], TETHERED[1] + 1))
        self.pin = er.members(n, range(PINNED[0], PINNED[1] + 1))
        self.ahead_fixes = [er.spring(TETHER_K, self.teth, er.unwrapped(x0, img0, s["box"])), er.add(PULL, np.ones(n, dtype=bool), every=PULL_EVERY)]
        self.e = dict(w=0, a=0, c=0)
        self.acting = dict(w=0, c=0, z=0.0)

    def ahead(self, step, x, img, f):
        t = wr.wall_terms(x, wall_region(), WALL)
        assert not t["outside"].any(), "a bead inside the ball"
        self.acting["w"] = max(self.acting["w"], int((t["ncontact"] > 0).sum()))
        f, out = er.apply(self.ahead_fixes, x, img, self.box, f + t["f"], step)
        self.e["w"] = t["energy"]
        if out[1] is not None:
            self.e["a"] = out[1]["energy"]
        return f

    def behind(self, step, x, img, f):
        t = ir.terms(x, indenter(), self.box)
        self.acting["c"] = max(self.acting["c"], int(t["touched"].sum()))
        self.e["c"] = t["energy"]
        f = f + t["f"]
        if self.pinned:
            before = f
            f, _ = er.apply([er.setforce(PIN, self.pin)], x, img, self.box, f, step)
            self.acting["z"] = max(self.acting["z"], float(np.abs(fr.ld(f) - fr.ld(before)).max()))
        return f

    def efix(self):
        return self.e["w"] + self.e["a"] + self.e["c"]


def respa_trajectory(S, x0, v0, img0, nsteps, uniforms, ahead, behind, inner=RESPA_INNER):
    """force_reference.System.trajectory under `run_style respa 2 inner`: the bonds on the inner level with timestep dt / inner,
    the pair term, the post-force fixes and the thermostat on the outer one (Respa::recurse: the outer half-kick, `inner` inner
    velocity-Verlet steps, the outer forces at the positions those leave and with the velocities of that moment, the outer
    half-kick).  f = the sum of the levels, as the engine holds it after a step with a thermo row."""
    x, v, img = fr.ld(x0).copy(), fr.ld(v0).copy(), np.asarray(img0, dtype=np.int64).copy()
    dt = fr.LD(S.model.dt)
    dti = dt / inner
    half_o = (dt / 2 * fr.LD(S.units["ftm2v"]) / S.m)[:, None]
    half_i = (dti / 2 * fr.LD(S.units["ftm2v"]) / S.m)[:, None]
    n3 = 3 * S.n

    def outer(step, ev):
        f = ahead(step, x, img, ev.f_pair)
        return behind(step, x, img, f + S.langevin_force(v, uniforms[step * n3:(step + 1) * n3]))
    ev = S.evaluate(x)
    f0, f1 = ev.f_bond, outer(0, ev)
    xs, vs, rows, gaps, hooks = [], [], [], [], []
    for step in range(nsteps + 1):
        if step:
            v = v + half_o * f1
            for _ in range(inner):
                v = v + half_i * f0
                x = x + dti * v
                S.wrap(x, img)
                ev = S.evaluate(x)
                f0 = ev.f_bond
                v = v + half_i * f0
            f1 = outer(step, ev)
            v = v + half_o * f1
        xs.append(S.unwrapped(x, img)); vs.append(v.copy()); rows.append(S.thermo(ev, v)); gaps.append(ev.gap)
    return dict(x=xs, v=vs, rows=rows, gaps=gaps, f=f0 + f1, xw=x, img=img, last=ev)


def _together(mode):
    from oracle import ranmars_stream
    s = system()
    S = PrunedSystem(fr.model_from_script(script("wall", True), s["ntypes"]), s["box"], s["type"], s["mass"], s["bonds"])
    x0, img0 = wrap_into_box(s)
    T = Together(s, x0, img0, pinned=mode != "respa")
    efix = {}

    def behind(step, x, img, f):
        f = T.behind(step, x, img, f)
        efix[step] = T.efix()
        return f
    u = ranmars_stream(fc.LANGEVIN_SEED, 3 * S.n * (fc.STEPS + 1))
    if mode == "respa":
        tr = respa_trajectory(S, x0, s["v"], img0, fc.STEPS, u, T.ahead, behind)
    else:
        tr = S.trajectory(x0, s["v"], img0, fc.STEPS, u, extra=T.ahead, after=behind)
    for k, r in enumerate(tr["rows"]):          # (fix_modify energy yes on the wall, the pull and the indenter)
        r["etotal"] = r["etotal"] + efix[k] / fr.LD(S.n)
    tr["acting"] = T.acting
    return S, tr


TOGETHER_STATS = ("neigh_builds", "steps_fused", "steps_fused_thermo", "steps_unfused", "min_iterations", "min_evals")


def run_together(mode, tmp_path):
    """The run on the engine -> x, v, f, image by ID, thermo_history(), `log`: the printed thermo rows with %.17g (what the
    engine's doubles are, digit for digit), the step counters."""
    import os
    from systems import run_product
    log = os.path.join(str(tmp_path), "log.together")
    p = run_product(together_script(mode, log), system(), tmp_path)
    try:
        got = dict(x=p.gather("x"), v=p.gather("v"), image=p.gather("image"), f=p.gather("f"), rows=np.asarray(p.thermo_history()),
                   stats={k: int(p.stat(k)) for k in TOGETHER_STATS}, pe=p.get_thermo("pe"))
        got["builds"] = got["stats"]["neigh_builds"]
        p.command("log none")
    finally:
        p.close()
    ncol = 7 + len(fix_columns(mode))
    rows = []
    for ln in open(log):
        w = ln.split()
        if len(w) == ncol and w[0].isdigit():
            rows.append([float(v) for v in w])
    got["log"] = np.array(rows)
    return got


SAMPLE_EVERY = 16


def sample_beads(n):
    """The beads whose end state a record holds value by value: every sixteenth and the pinned group (indices, ID - 1)."""
    return np.array(sorted(set(range(0, n, SAMPLE_EVERY)) | set(range(PINNED[0] - 1, PINNED[1]))))


def digest(a, dtype=np.float64):
    """SHA-256 of an array's values as little-endian `dtype` in C order: equal exactly when every element is, bit for bit."""
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.dtype(dtype).newbyteorder("<")).tobytes()).hexdigest()


def together_pack(mode, got):
    """What tests/golden/postforce_together_<mode>.json holds of a run: the thermo rows and printed columns as hex floats, the
    step counters, the end state of ALL beads as the SHA-256 of positions, velocities and image flags (a record of every
    double of three runs is a megabyte of text) and of sample_beads() value by value as hex floats."""
    k = sample_beads(len(got["x"]))
    hexed = lambda a: [[float(v).hex() for v in row] for row in np.atleast_2d(a)]
    return dict(mode=mode, steps=fc.STEPS, thermo=THERMO, columns=["step", "temp", "epair", "emol", "etotal", "press", "pe"] + fix_columns(mode),
                stats=got["stats"], rows=hexed(got["rows"]), log=hexed(got["log"]),
                sha256=dict(x=digest(got["x"]), v=digest(got["v"]), image=digest(got["image"], np.int64)),
                sample=dict(beads=k.tolist(), x=hexed(got["x"][k]), v=hexed(got["v"][k]), image=np.asarray(got["image"])[k].tolist()))


def write_record(rec, path):
    """together_pack's dict as JSON with one key of the record and of its sample per line."""
    import json
    line = lambda d: ",\n".join("%s:%s" % (json.dumps(k), json.dumps(d[k], separators=(",", ":"))) for k in sorted(d) if k != "sample")
    with open(path, "w") as fh:
        fh.write("{" + line(rec) + ',\n"sample":{\n' + line(rec["sample"]) + "}}\n")


def together_record(mode):
    """tests/golden/postforce_together_<mode>.json: what the commit before the post-force fixes got one owner left on an MI355X
    (make_postforce_together.py, together_pack)."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "postforce_together_%s.json" % mode)) as fh:
        z = json.load(fh)
    unhex = lambda rows: np.array([[float.fromhex(v) for v in r] for r in rows])
    s = z["sample"]
    return dict(z, rows=unhex(z["rows"]), log=unhex(z["log"]), sample=dict(beads=np.array(s["beads"]), x=unhex(s["x"]), v=unhex(s["v"]), image=np.array(s["image"])))


def list_builds(xs):
    """The displacement rule of the reference trajectory itself (neigh_modify every 1 delay 1 check yes): a build at every step
    on which some bead is farther than half the skin from where it was at the last build.  -> (steps with a build, the
    smallest | |d|^2 - skin^2 / 4 | any step's largest displacement came to)"""
    trig = fr.LD(SKIN) ** 2 / 4
    hold, steps, margin = xs[0], [], np.inf
    for k in range(1, len(xs)):
        d2 = ((xs[k] - hold) ** 2).sum(axis=1).max()
        margin = min(margin, float(abs(d2 - trig)))
        if d2 > trig:
            steps.append(k)
            hold = xs[k]
    return steps, margin


def image_flags(S, xs, builds):
    """The image flags a run ends with: the engine wraps a coordinate into the box when it rebuilds the lists and at no other
    time (between two builds a stored coordinate may lie outside by up to half the skin), so they are those of the unwrapped
    positions at the last build - at the start where there was none.  Also the distance of the nearest coordinate from a face
    at that step."""
    xu = xs[builds[-1] if builds else 0]
    rel = (xu - S.lo) / S.prd
    img = np.floor(rel)
    off = rel - img
    return img.astype(np.int64), float((np.minimum(off, 1 - off) * S.prd).min())


def _deviation(ref, low):
    """({x, v, f, rows: deviation of the float64 run `low` of a restatement from its long-double run `ref`}, steps with a list
    build)"""
    assert low["x"][-1].dtype == np.float64 and low["f"].dtype == np.float64 and ref["x"][-1].dtype == fr.LD
    dev = dict(x=fc.relerr(low["x"][-1], ref["x"][-1]), v=fc.relerr(low["v"][-1], ref["v"][-1]), f=fc.relerr(low["f"], ref["f"]),
               rows=max(fc.relerr(low["rows"][k][key], ref["rows"][k][key]) for k in range(fc.STEPS + 1) for key in fc.ROW_KEYS))
    # no bead moved half of REACH: no pair outside candidates() came within a cutoff
    moved = max(float(np.sqrt(((xk - ref["x"][0]) ** 2).sum(axis=1).max())) for xk in ref["x"])
    assert moved < REACH / 2, moved
    builds, margin = list_builds(ref["x"])
    assert margin > 1e-6, margin          # (no step's largest displacement is at the trigger)
    return dev, builds


@functools.lru_cache(maxsize=None)
def reference(family, langevin):
    """(system, long-double trajectory, {x, v, f, rows: deviation of the float64 run of the same restatement}, steps with a
    list build)"""
    S, ref = _trajectory(family, langevin)
    with fr.precision(np.float64):
        _, low = _trajectory(family, langevin)
    return (S, ref) + _deviation(ref, low)


def required_gap(S, dev):
    """force_compare.required_gap with this run's position bound"""
    return 100.0 * 4.0 * np.sqrt(3.0) * S.cutmax * fc.bound(dev["x"], fc.TRAJ_CEILING["x"])


# ------------------------------------------------------------------------------------------------------------------
def relabelled(s, seed=77):
    """The same beads at the same places in the same file order under other IDs: bead p of `s` has the ID perm[p] + 1.  The
    reference's local index of a bead (its place in the file, `atom_modify sort 0 0`) is then no longer its ID - 1, and
    nothing else differs: the Langevin draws go by the local index.  -> (system, perm); what the engine hands out by ID is
    in the order of `s` after [perm]."""
    n = len(s["x"])
    perm = np.random.RandomState(seed).permutation(n)
    t = dict(s)
    for k in ("x", "v", "type", "mol", "image"):
        a = np.empty_like(np.asarray(s[k]))
        a[perm] = s[k]
        t[k] = a
    b = np.array(s["bonds"]).reshape(-1, 3).copy()
    b[:, 1:] = perm[b[:, 1:] - 1] + 1
    t["bonds"] = b
    if s.get("angles") is not None and len(s.get("angles", [])):
        a = np.array(s["angles"]).reshape(-1, 4).copy()
        a[:, 1:] = perm[a[:, 1:] - 1] + 1
        t["angles"] = a
    t["file_order"] = perm
    return t, perm
