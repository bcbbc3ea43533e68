"""Edits of a device-resident state through the C-ABI's subset calls (lammps_scatter_atoms_subset), and the state the reference
must see after each: the inputs, the edits and the references of test_capi_edits_cpu.py (which proves without a GPU that every
(input, edit) pair is a fair question) and test_gpu_capi_edits.py (which asks it of k_subset_scatter, k_subset_gather and the
three routes scatter_subset_impl chooses between).

An edit is a list of (property, ids, rows), applied in order through scatter_ids / scatter_atoms_subset.  What the reference
program does with one: scatter_atoms_subset writes the rows as given (src/library.cpp:2482-2614; a repeated ID keeps its last
row), and the setup of the next run wraps once per dimension with the image flag following (Domain::pbc,
src/domain.cpp:528-645): x < lo -> x += prd, image - 1; x >= hi -> x -= prd, x = max(x, lo), image + 1.  edited() restates
exactly that in float64, so the positions and image flags the engine hands back after `run 0` can be compared bit for bit.

Inputs (the smallest at which these kernels can still go wrong):
  offset+free    force_inputs.offset's 630-bead lattice (its first 630 beads are offset's, bit for bit) plus 24 unbonded beads
                 on interstitial sites, with a further list of empty interstitial sites - the targets of the moves.  No two
                 of all these sites are closer than 1.9, so whichever of them are occupied do not see each other.
  types          force_inputs.types: three types, masses 1.0 / 1.7 / 0.6, cutoffs 1.0 .. 2.5 without a shift
  types-tall     the same with 16 lattice planes along z instead of 9 (1296 beads), for the type edit on three slabs: a slab has
                 to be two pair shells of 2.7 thick, and `types` is 9.5 long
  offset-pinned  force_inputs.offset(True) under `fix nve` on `group mobile type 1`
Everything is seeded."""
import functools

import numpy as np

import force_compare as fc
import force_inputs as fi
from neigh_inputs import add_free_beads, translate
from systems import wrap_into_box

NFREE = 24
SITE_SEED = 58            # (as the seeds of force_inputs.py: not arbitrary - with another one bound() may assert; then take the next)
TALL_SEED = 37
NEAR_SEED = 9             # (as the seeds of force_inputs.py: one under which 16 x the oracle's deviation stays below 1e-12)
SITE_DEVIATION = 2.5e-14  # site_deviation(): the oracle sums in another order once more beads are there - a factor of two is left for that
SEPARATION = 1.9          # > 1.12 + 0.4: two occupied sites are in no list of each other's; > 1.83: they share none of their eight neighbours
GHOST = 2.0               # comm_modify cutoff of force_inputs.HEAD
CUT = 1.12
THREE_CELLS = 3 * (1.12 + 0.4)
K_TETHER = 0.1            # a tether one box length (5.3 .. 14.8) long pulls with 0.5 .. 1.5
PTENSOR = "thermo_style custom step temp epair emol etotal press pxx pyy pzz pxy pxz pyz\n"
WORLDS = (2, 3, 4)


def owner(z, box, world):
    """The slab that owns a (wrapped) z: the expression of Engine::upload."""
    lo, hi = box[2]
    w = np.floor((np.asarray(z, dtype=np.float64) - lo) / ((hi - lo) / world)).astype(int)
    return np.clip(w, 0, world - 1)


def pbc(x, image, box):
    """Domain::pbc on rows that lie within one period of the box: one wrap per dimension, the image flag following."""
    x, image = np.array(x, dtype=np.float64), np.array(image, dtype=np.int32)
    for d in range(3):
        lo, hi = float(box[d][0]), float(box[d][1])
        prd = hi - lo
        m = x[:, d] < lo
        x[m, d] += prd
        image[m, d] -= 1
        m = x[:, d] >= hi
        x[m, d] = np.maximum(x[m, d] - prd, lo)
        image[m, d] += 1
    assert ((x >= np.asarray(box)[:, 0]) & (x < np.asarray(box)[:, 1])).all(), "a row farther than one period from the box"
    return x, image


def rigid_shift(ename, prd):
    return np.array([0.6 * prd[0], -0.4 * prd[1], 0.0]) if ename == "rigid" else np.array([0.0, 0.0, prd[2] / 3.0])


def min_image(d, prd):
    return d - prd * np.round(d / prd)


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def site_deviation(frame=""):
    """For every interstitial site of the offset lattice: how far the FP64 oracle's forces are from the long-double reference's
    on the beads a free bead on that site (alone) touches, itself included - and the same with the bead put onto the lower z
    face (nan where the site is not on the plane just above it).
    Why sites are chosen by this: a free bead sits between eight beads 0.91 away, terms of 117 each that nearly cancel, and at
    z ~ -64 a partner across a periodic face is reached through x_j + prd, rounded to 1.4e-14 - on an unlucky site the oracle is
    1.5e-13 from the reference in a force component of order 1, and 16 x that is above the 1e-12 a single evaluation has to
    meet: by the rule of force_compare.bound such an input is the wrong input.  The choice is made by the reference's and
    the oracle's figures alone; nothing of the engine enters it.
    frame: "" - the input as it is; "rigid", "rigid-z" - after that edit's translation of everything (the free beads have to be
    quiet there as well: a translation rounds every coordinate anew)."""
    import force_reference as fr
    from systems import run_oracle
    base = translate(fi.lattice(5, 9, 14, seed=22), fi.OFFSET_ORIGIN)
    nx, ny, nz = base["lattice"]
    box = np.asarray(base["box"], dtype=np.float64)
    prd = box[:, 1] - box[:, 0]
    pts = fi.interstitial(base, np.array([(i, j, k) for k in range(nz) for j in range(ny) for i in range(nx)]))
    one = fi.hot(fi.displace(add_free_beads(base, pts[:1])), 5.0)
    n = len(one["x"])
    text = fi.script(dict(force_field=fi.FENE + fi.WCA), skin="0.2") + "fix 1 all nve\nrun 0\n"
    S = fr.System(fr.model_from_script(text, 1), one["box"], one["type"], one["mass"], one["bonds"])
    x0 = wrap_into_box(fi.offset()["system"])[0]
    shown = wrap_into_box(dict(x=pts + np.asarray(fi.DISPLACE) * prd, image=np.zeros((len(pts), 3), dtype=np.int32), box=box))[0]
    if frame:
        zero = np.zeros((len(x0), 3), dtype=np.int32)
        x0, shown = pbc(x0 + rigid_shift(frame, prd), zero, box)[0], pbc(shown + rigid_shift(frame, prd), zero, box)[0]
        f0 = fc.reference_system("offset")[0].evaluate(x0).f
    else:
        f0 = fc.reference_run0("offset").f
    out = np.full((len(pts), 2), np.nan)
    for q in range(len(pts)):
        for on_face in (0, 1):
            p = shown[q].copy()
            if on_face:
                if frame or p[2] - box[2, 0] > 0.1:
                    continue
                p[2] = box[2, 0]
            x = np.concatenate([x0, p[None, :]])
            ev = S.evaluate(x, only=n - 1)          # the terms the free bead takes part in; the rest is offset's own evaluation
            f = ev.f.copy()
            f[:n - 1] += f0
            o = run_oracle(text, dict(one, x=x, image=np.zeros((n, 3), dtype=np.int32)))
            touched = np.nonzero((np.asarray(ev.f, dtype=np.float64) != 0).any(axis=1))[0]
            out[q, on_face] = fc.relerr(o.f()[touched], f[touched])
    return out[:, 0], out[:, 1]


@functools.lru_cache(maxsize=None)
def offset_free():
    base = translate(fi.lattice(5, 9, 14, seed=22), fi.OFFSET_ORIGIN)          # what force_inputs.offset starts from
    nx, ny, nz = base["lattice"]
    box = np.asarray(base["box"], dtype=np.float64)
    prd = box[:, 1] - box[:, 0]
    # every interstitial site of the periodic lattice (index n - 1 along an axis: between the last site and the first one's image)
    sites = np.array([(i, j, k) for k in range(nz) for j in range(ny) for i in range(nx)])
    pts = fi.interstitial(base, sites)
    shown = wrap_into_box(dict(x=pts + np.asarray(fi.DISPLACE) * prd, image=np.zeros((len(pts), 3), dtype=np.int32), box=box))[0]
    depth = np.minimum(shown - box[:, 0], box[:, 1] - shown)
    rng = np.random.RandomState(SITE_SEED)
    quiet, quiet_floor = site_deviation()
    quiet, quiet_floor = quiet < SITE_DEVIATION, quiet_floor < SITE_DEVIATION
    quiet_free = quiet & (site_deviation("rigid")[0] < SITE_DEVIATION) & (site_deviation("rigid-z")[0] < SITE_DEVIATION)
    far_from = lambda q, kept: all(np.linalg.norm(min_image(pts[q] - pts[c], prd)) > SEPARATION for c in kept)
    # the free beads: quiet sites (in all three frames) in random order, each kept if it is 1.9 from every site kept before
    free = []
    for q in (int(q) for q in rng.permutation(len(pts)) if quiet_free[q]):
        if len(free) < NFREE and far_from(q, free):
            free.append(q)
    # the empty sites, 1.9 from each other and from every free bead's: first the ones the edit `outside` needs - a site within
    # one cutoff of three faces, one on the plane of sites just above the lower z face, one within one cutoff of each of the six
    # faces and of no other - then quiet sites in random order.  (The edit `far` takes every free bead away, so its targets
    # only have to keep their distance from each other; `outside` and `two-away` leave free beads where they are.)
    wanted = [np.nonzero((depth < CUT).all(axis=1) & quiet)[0],
              np.nonzero((shown[:, 2] - box[2, 0] < 0.1) & (depth[:, :2] > CUT).all(axis=1) & quiet_floor)[0]]
    for d in range(3):
        others = [k for k in range(3) if k != d]
        for near_face in (shown[:, d] - box[d, 0], box[d, 1] - shown[:, d]):
            wanted.append(np.nonzero((near_face > 0.1) & (near_face < CUT) & (depth[:, others] > CUT).all(axis=1) & quiet)[0])
    empty = []
    for ok in wanted:
        empty.append(next(int(q) for q in rng.permutation(ok) if far_from(q, free + empty)))
    corner = empty[0]
    for q in (int(q) for q in rng.permutation(len(pts)) if quiet[q]):
        if far_from(q, free + empty):
            empty.append(q)
    vacated = list(empty)          # ... and more for `far`, which may lie next to a site a free bead leaves
    for q in (int(q) for q in rng.permutation(len(pts)) if quiet[q]):
        if q not in free and far_from(q, vacated):
            vacated.append(q)
    s = add_free_beads(base, pts[free])
    n0 = len(base["x"])
    s["v"] = s["v"].copy()
    s["v"][n0:] = np.random.RandomState(52).normal(size=(NFREE, 3))
    s = fi.hot(fi.displace(s), 5.0)
    assert np.array_equal(s["x"][:n0], fi.offset()["system"]["x"]) and np.array_equal(s["v"][:n0], fi.offset()["system"]["v"])
    return dict(system=s, force_field=fi.FENE + fi.WCA, free=np.arange(n0 + 1, n0 + NFREE + 1, dtype=np.int32), empty=shown[empty], vacated=shown[vacated],
                corner=shown[corner], fixes="nve")


@functools.lru_cache(maxsize=None)
def types_tall():
    """force_inputs.types with 16 instead of 9 lattice planes along z (1296 beads): three slabs of it are 5.6 thick, two pair
    shells of 2.5 + 0.2 - `types` itself is too short to be cut at all."""
    s = fi.lattice(9, 9, 16, seed=TALL_SEED)
    n = len(s["x"])
    s["type"] = (1 + (np.arange(n) * 7 // 3) % 3).astype(np.int32)
    s["ntypes"], s["mass"] = 3, [1.0, 1.7, 0.6]
    return dict(system=fi.hot(fi.displace(s), 5.0), force_field=fi.TYPES_FF, fixes="nve")


INPUTS = {"offset+free": offset_free, "types": lambda: dict(fi.types(), fixes="nve"), "types-tall": types_tall,
          "offset-pinned": lambda: dict(fi.offset(True), fixes="group")}
EDITS = {"near": "offset+free", "far": "offset+free", "outside": "offset+free", "rigid": "offset+free", "rigid-z": "offset+free",
         "two-away": "offset+free", "v": "offset+free", "f": "offset+free", "image3": "offset+free", "image1": "offset+free",
         "retype": "types", "retype-tall": "types-tall", "retype-grouped": "offset-pinned"}
TWELVE = ("far", "outside", "rigid", "v", "retype", "retype-grouped")          # the edits that are followed for twelve steps
SLABS = [("near", 2), ("near", 3), ("near", 4), ("far", 2), ("far", 3), ("far", 4), ("outside", 2), ("outside", 3), ("outside", 4),
         ("two-away", 4), ("rigid-z", 3), ("retype-tall", 3)]
SLAB_DOWNLOADS = {"two-away": 1, "rigid-z": 1}          # every other edit stays on the device


@functools.lru_cache(maxsize=None)
def start(name):
    """(x, v, image, type) as read_data leaves them: what the device holds after the script and `run 0`."""
    s = INPUTS[name]()["system"]
    x, image = wrap_into_box(s)
    return x, s["v"].copy(), image, np.asarray(s["type"], dtype=np.int32).copy()


def box_of(name):
    return np.asarray(INPUTS[name]()["system"]["box"], dtype=np.float64)


# ------------------------------------------------------------------------------------------------
# edits
# ------------------------------------------------------------------------------------------------
def _far_targets(x, free, empty, box, want_two_away=False):
    """For every free bead (or, two slabs away, for four of them) an empty site of its own, at least three cells away: chosen
    one bead after the other so that the moves between them cross every pair of periodic faces and, on four slabs, go up and
    down out of every slab - never two slabs away (that is the edit `two-away`)."""
    prd = box[:, 1] - box[:, 0]
    need = {("x",), ("y",), ("z",)} | {(s, d) for s in range(4) for d in (1, 3)}
    used, rows, ids = set(), [], []
    for t in free:
        old = x[t - 1]
        best, gain = None, -1
        for q, new in enumerate(empty):
            if q in used or np.linalg.norm(min_image(new - old, prd)) < THREE_CELLS:
                continue
            so, sn = int(owner(old[2], box, 4)), int(owner(new[2], box, 4))
            hop = (sn - so) % 4
            if want_two_away != (hop == 2):
                continue
            # (three ranks: their slabs are other slabs - also there a move has to be to another slab for some)
            feats = {(so, hop)} | {("xyz"[d],) for d in range(3) if abs(new[d] - old[d]) > 0.5 * prd[d]}
            g = len(feats & need)
            if g > gain:
                best, gain, bf = q, g, feats
        if best is None:
            continue
        need -= bf
        used.add(best)
        ids.append(t)
        rows.append(empty[best])
        if want_two_away and len(ids) == 4:
            break
    return np.array(ids, dtype=np.int32), np.array(rows)


def _outside_rows(x, free, empty, corner, box):
    """Out-of-box images of empty sites: up to one cutoff beyond each of the six faces, one beyond a corner, one with z == hi
    exactly (the image of a site 0.02 above the lower z face, put onto the face itself).  Each goes to a free bead that is, on
    four slabs, in the target's slab or next to it."""
    prd = box[:, 1] - box[:, 0]
    targets = []
    taken = set()

    def site(cond):
        for q, p in enumerate(empty):
            if q not in taken and not np.array_equal(p, corner) and cond(p):
                taken.add(q)
                return p
        raise AssertionError("no empty site for an `outside` row")

    for d in range(3):
        others = [k for k in range(3) if k != d]
        inner = lambda p: all(min(p[k] - box[k, 0], box[k, 1] - p[k]) > CUT for k in others)
        p = site(lambda p: 0.1 < p[d] - box[d, 0] < CUT and inner(p))
        sh = np.zeros(3); sh[d] = prd[d]
        targets.append((p, p + sh))                         # beyond the upper face
        p = site(lambda p: 0.1 < box[d, 1] - p[d] < CUT and inner(p))
        targets.append((p, p - sh))                         # beyond the lower face
    sh = np.where(corner - box[:, 0] < CUT, prd, -prd)
    targets.append((corner, corner + sh))
    p = site(lambda p: p[2] - box[2, 0] < 0.1)
    targets.append((p, np.array([p[0], p[1], box[2, 1]])))
    ids, rows, used = [], [], set()
    for p, row in targets:
        for t in free:
            if t not in used and (int(owner(p[2], box, 4)) - int(owner(x[t - 1, 2], box, 4))) % 4 != 2 \
                    and np.linalg.norm(min_image(p - x[t - 1], prd)) > THREE_CELLS:
                used.add(t)
                ids.append(t)
                rows.append(row)
                break
        else:
            raise AssertionError("no free bead for an `outside` row")
    return np.array(ids, dtype=np.int32), np.array(rows)


@functools.lru_cache(maxsize=None)
def edit(ename):
    """[(property, ids, rows)] - property "image1" stands for `image` sent as the packed word."""
    name = EDITS[ename]
    case = INPUTS[name]()
    x, v, image, typ = start(name)
    n = len(x)
    box = box_of(name)
    prd = box[:, 1] - box[:, 0]
    rng = np.random.RandomState(sum(map(ord, ename)))
    pick = lambda k: rng.choice(np.arange(1, n + 1), size=k, replace=False).astype(np.int32)
    if ename == "near":
        rng = np.random.RandomState(NEAR_SEED)
        ids = pick(40)
        return [("x", ids, x[ids - 1] + rng.uniform(-0.05, 0.05, size=(40, 3)))]
    if ename == "far":
        ids, rows = _far_targets(x, case["free"], case["vacated"], box)
        return [("x", ids, rows)]
    if ename == "two-away":
        ids, rows = _far_targets(x, case["free"], case["empty"], box, want_two_away=True)
        return [("x", ids, rows)]
    if ename == "outside":
        ids, rows = _outside_rows(x, case["free"], case["empty"], case["corner"], box)
        # ... and one row alone in a call of its own (K = 1)
        return [("x", ids[:-1], rows[:-1]), ("x", ids[-1:], rows[-1:])]
    if ename == "rigid":
        return [("x", np.arange(1, n + 1, dtype=np.int32), x + rigid_shift(ename, prd))]
    if ename == "rigid-z":
        return [("x", np.arange(1, n + 1, dtype=np.int32), x + rigid_shift(ename, prd))]
    if ename == "v":
        # 50 velocity rows replaced, in a call of 257 different IDs (a full block of the scatter kernel and one row): the other 207
        # rows carry the velocities their beads have.  One of the 50 is named twice more ahead of them, with two other rows: the
        # last one stays
        ids = pick(257)
        rows = v[ids - 1].copy()
        rows[:50] = 0.5 * rows[:50] + rng.normal(0.0, 0.3, size=(50, 3))
        order = rng.permutation(257)
        ids, rows = ids[order], rows[order]
        k = int(np.nonzero(order == 7)[0][0])
        return [("v", np.concatenate([ids[k:k + 1], ids[k:k + 1], ids]), np.concatenate([rows[k:k + 1] + 1.0, rows[k:k + 1] - 2.0, rows]))]
    if ename == "f":
        ids = pick(50)
        return [("f", ids, rng.normal(0.0, 5.0, size=(50, 3)))]
    if ename in ("image3", "image1"):
        ids = tether_ids()
        ids = np.concatenate([ids[::2], np.setdiff1d(pick(40), ids)[:15]]).astype(np.int32)
        rows = rng.randint(-2, 3, size=(30, 3)).astype(np.int32)
        assert len(ids) == 30
        return [("image" if ename == "image3" else "image1", ids, rows)]
    if ename in ("retype", "retype-tall"):
        # 45 beads cycled 1 -> 2 -> 3 -> 1, fifteen of each type
        ids = rng.permutation(np.concatenate([rng.permutation(np.nonzero(typ == t)[0] + 1)[:15] for t in (1, 2, 3)])).astype(np.int32)
        return [("type", ids, (typ[ids - 1] % 3 + 1).astype(np.int32))]
    if ename == "retype-grouped":
        pinned, mobile = np.nonzero(typ == 2)[0] + 1, np.nonzero(typ == 1)[0] + 1
        ids = np.concatenate([rng.permutation(pinned)[:10], rng.permutation(mobile)[:10]]).astype(np.int32)
        return [("type", ids, np.array([1] * 10 + [2] * 10, dtype=np.int32))]
    raise KeyError(ename)


@functools.lru_cache(maxsize=None)
def tether_ids():
    """The group of the tether fix of the image edits: 30 beads of offset+free, 15 of which the edits name."""
    n = len(start("offset+free")[0])
    return np.sort(np.random.RandomState(77).choice(np.arange(1, n + 1), size=30, replace=False)).astype(np.int32)


def packed(im):
    """lammps_encode_image_flags"""
    im = np.asarray(im, dtype=np.int64)
    return (((im[:, 0] + 512) & 1023) | (((im[:, 1] + 512) & 1023) << 10) | (((im[:, 2] + 512) & 1023) << 20)).astype(np.int32)


def last_rows(ids, rows):
    """The rows a call leaves: of a repeated ID the last."""
    keep = {}
    for k, t in enumerate(ids):
        keep[int(t)] = k
    order = sorted(keep.values())
    return np.asarray(ids)[order], np.asarray(rows)[order]


def written(state, calls):
    """(x, v, image, type, f-rows) with the rows written as given - what a gather straight after the scatter returns.
    state: (x, v, image, type); f-rows: {id: row} (the forces are whatever the last evaluation left, but for these)."""
    x, v, image, typ = (a.copy() for a in state)
    frows = {}
    for prop, ids, rows in calls:
        ids, rows = last_rows(ids, rows)
        if prop == "f":
            frows.update({int(t): r for t, r in zip(ids, rows)})
        else:
            dst = {"x": x, "v": v, "image": image, "image1": image, "type": typ}[prop]
            dst[ids - 1] = rows
    return x, v, image, typ, frows


def edited_state(state, calls, box):
    """(x, v, image, type) the next run starts from: written(), then Domain::pbc."""
    x, v, image, typ, _ = written(state, calls)
    x, image = pbc(x, image, box)
    return x, v, image, typ


@functools.lru_cache(maxsize=None)
def edited(ename):
    return edited_state(start(EDITS[ename]), edit(ename), box_of(EDITS[ename]))


def send(lmp, calls):
    """The calls of an edit through the C-ABI."""
    import ctypes as C
    for prop, ids, rows in calls:
        if prop == "image1":
            w = packed(rows)
            lmp.scatter_atoms_subset("image", 0, 1, len(ids), [int(t) for t in ids], (C.c_int * len(ids))(*[int(q) for q in w]))
        else:
            lmp.scatter_ids(prop, ids, rows)


def edited_ids(calls):
    return np.unique(np.concatenate([ids for _, ids, _ in calls]))


# ------------------------------------------------------------------------------------------------
# scripts
# ------------------------------------------------------------------------------------------------
def tether_lines():
    return "group tether id %s\nfix tether tether spring/self %.17g\n" % (" ".join(str(t) for t in tether_ids()), K_TETHER)


def script(ename, name=None):
    """Everything up to the first run command: neighbor 0.2 and thermo 4, as the twelve-step runs of force_compare have them."""
    name = name or EDITS[ename]
    case = INPUTS[name]()
    text = fi.script(case, skin="0.2") + fc.FIXES[case["fixes"]]
    if ename in ("image3", "image1"):
        text += tether_lines()
    return text + PTENSOR + "thermo 4\n"


def system_at(name, state):
    """The input with (x, v, image, type) replaced: what a fresh oracle run - or a data file - starts from."""
    s = dict(INPUTS[name]()["system"])
    s["x"], s["v"], s["image"], s["type"] = (np.array(a) for a in state)
    return s


def oracle_script(ename, name, steps):
    """script() for the oracle started fresh from an edited system: the group of `fix nve` by ID - membership is what it was
    when the group was defined, as in the reference, not what `type 1` would select after the edit.  (No tether: the oracle has
    no fix spring/self.)"""
    case = INPUTS[name]()
    text = fi.script(case, skin="0.2") + fc.FIXES[case["fixes"]]
    if case["fixes"] == "group":
        members = np.nonzero(start(name)[3] == 1)[0] + 1
        text = text.replace("group mobile type 1", "group mobile id " + " ".join(str(t) for t in members))
    return text + "thermo 1\nrun %d\n" % steps


# ------------------------------------------------------------------------------------------------
# references (long double, force_reference.py) and the oracle's deviation from them, from any state
# ------------------------------------------------------------------------------------------------
def reference_system(name, typ):
    """force_reference.System of an input with the types `typ`; fix nve's group is the one the ORIGINAL types defined."""
    import force_reference as fr
    case = INPUTS[name]()
    s = case["system"]
    model = fr.model_from_script(fi.script(case, skin="0.2") + fc.FIXES[case["fixes"]], s["ntypes"])
    S = fr.System(model, s["box"], typ, s["mass"], s["bonds"], s.get("angles"))
    if model.nve_types is not None:
        S.mobile = np.isin(start(name)[3], model.nve_types)
    return S


def thermo_keywords(S, ev, v):
    return S.thermo(ev, v, True)


def oracle_keywords(S, o):
    """force_compare.oracle_thermo for any system (norm yes)."""
    n = S.n
    vol = float(np.prod(S.box[:, 1] - S.box[:, 0]))
    t = o.thermo()
    m = np.asarray([float(q) for q in S.m])
    v = o.v()
    k6 = [(m * v[:, a] * v[:, b]).sum() for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
    out = dict(evdwl=t[6] / n, ebond=t[7] / n, eangle=0.0, pe=(t[6] + t[7]) / n, ke=t[5], temp=t[0], press=t[4])
    out.update({k: (k6[c] + t[8 + c]) / vol for c, k in enumerate(fc.THERMO_KEYS[7:])})
    return out


def run0_from(ename, name, state):
    """(System, Eval, {quantity: the oracle's deviation}) of one evaluation at a state."""
    from systems import run_oracle
    x, v, image, typ = state
    S = reference_system(name, typ)
    ev = S.evaluate(x)
    o = run_oracle(oracle_script(ename, name, 0), system_at(name, state))
    assert np.array_equal(o.x(), x) and np.array_equal(o.types(), typ)
    dev = {"f": fc.relerr(o.f(), ev.f)}
    ref, got = thermo_keywords(S, ev, v), oracle_keywords(S, o)
    for k in fc.THERMO_KEYS:
        dev[k] = fc.relerr(got[k], ref[k])
    return S, ev, dev


def trajectory_from(ename, name, state, steps):
    """(System, reference trajectory, {x, v, f, rows: the oracle's deviation}, the oracle's list builds) of `steps` steps from
    a state."""
    from systems import run_oracle
    x, v, image, typ = state
    S = reference_system(name, typ)
    ref = S.trajectory(x, v, image, steps)
    o = run_oracle(oracle_script(ename, name, steps), system_at(name, state))
    h = o.thermo_history()
    assert len(h) == steps + 1
    dev = dict(x=fc.relerr(S.unwrapped(o.x(), o.image()), ref["x"][-1]), v=fc.relerr(o.v(), ref["v"][-1]), f=fc.relerr(o.f(), ref["f"]),
               rows=max(fc.relerr(h[k, 1 + c], ref["rows"][k][key]) for k in range(steps + 1) for c, key in enumerate(fc.ROW_KEYS)))
    return S, ref, dev, int(o.neigh_builds())


@functools.lru_cache(maxsize=None)
def run0(ename):
    return run0_from(ename, EDITS[ename], edited(ename))


@functools.lru_cache(maxsize=None)
def trajectory(ename):
    return trajectory_from(ename, EDITS[ename], edited(ename), fc.STEPS)


@functools.lru_cache(maxsize=None)
def mid_trajectory(first=6):
    """The stand-in for the state of the mid-trajectory test, without an engine: the oracle's state after `first` steps of
    offset+free with `far` applied, and the steps that follow, up to the twelfth (trajectory_from); whether the oracle rebuilt its lists on
    step `first` (the engine's builds are held to the oracle's: after 6 steps the run ends on a rebuild, after 7 it does not)."""
    from systems import run_oracle
    name = "offset+free"
    o = run_oracle(oracle_script("far", name, first), system_at(name, start(name)))
    before = run_oracle(oracle_script("far", name, first - 1), system_at(name, start(name)))
    state = edited_state((o.x(), o.v(), o.image().astype(np.int32), start(name)[3]), edit("far"), box_of(name))
    return trajectory_from("far", name, state, fc.STEPS - first) + (int(o.neigh_builds()), int(o.neigh_builds()) > int(before.neigh_builds()))


def required_gap(S, dev):
    """force_compare.required_gap for any trajectory."""
    return 100.0 * 4.0 * np.sqrt(3.0) * S.cutmax * fc.bound(dev["x"], fc.TRAJ_CEILING["x"])


# ------------------------------------------------------------------------------------------------
# the tether of the image edits: long double (extforce_reference.py) and its float64 restatement
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tether(ename):
    """(force with the tethers' (n, 3) long double, the fix's energy, {f, energy: deviation of the float64 restatement}) at
    the edited state.  The origins are the unwrapped positions at the time the fix was defined: the input's."""
    import extforce_reference as xr
    name = EDITS[ename]
    box = box_of(name)
    x0, _, image0, _ = start(name)
    x, v, image, typ = edited(ename)
    S, ev, dev = run0(ename)
    member = xr.members(len(x), tether_ids())
    origin = xr.unwrapped(x0, image0, box)
    f, out = xr.apply([xr.spring(K_TETHER, member, origin)], x, image, box, ev.f)
    # the same in float64, in the reference program's operation order (fix_spring_self.cpp: unmap, d = unwrap - origin, f -= k d)
    prd = box[:, 1] - box[:, 0]
    o64 = x0 + image0 * prd
    d = (x + image * prd) - o64
    d[~member] = 0.0
    f64 = np.asarray(ev.f, dtype=np.float64) - K_TETHER * d
    e64 = 0.5 * K_TETHER * (d * d).sum()
    return f, out[0]["energy"], dict(f=fc.relerr(f64, f), energy=fc.relerr(e64, out[0]["energy"]))
