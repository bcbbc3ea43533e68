"""Input generators of the neighbor-list tests (test_gpu_neigh.py) - shared with test_neigh_reference_cpu.py, which proves
without a GPU that none of them holds an undecided pair (neigh_reference.py) and that the cutoff ladder straddles the FP32
band of the list build.  Everything is seeded: the systems are the same in every process."""
import functools

import numpy as np

from neigh_reference import LD, delta, fp32_band, sep2_ld
from systems import CHAIN_SCRIPT, lattice_chain

CUTNEIGH = 1.12 + 0.4          # pair cutoff + skin of CHAIN_SCRIPT, added the way the engine adds them
ORIGINS = [(0.0, 0.0, 0.0), (-37.25, 1000.5, -2048.125), (4000.0, -4000.0, 4000.75)]
# pair_style zero: the list is built, no pair force is computed (for geometries an LJ force could not take)
ZERO_SCRIPT = CHAIN_SCRIPT.replace("pair_style lj/cut 1.12\npair_modify shift yes\npair_coeff * * 1.0 1.0 1.12",
                                   "pair_style zero 1.12\npair_coeff * *")
assert "pair_style zero" in ZERO_SCRIPT


def cell_counts(box, cutneigh=CUTNEIGH):
    """Cells of the list build as dev_alloc counts them: y and z cells at least cutneigh wide, x cells a quarter of that."""
    box = np.asarray(box, dtype=np.float64)
    return tuple(max(1, int((box[k, 1] - box[k, 0]) / (cutneigh / 4 if k == 0 else cutneigh))) for k in range(3))


def initial_maxneigh(n, box, cutneigh=CUTNEIGH):
    """Rows of the list table before any regrow (dev_alloc)."""
    box = np.asarray(box, dtype=np.float64)
    vol = float(np.prod(box[:, 1] - box[:, 0]))
    return int(n / vol * 4.18879020478639 * cutneigh ** 3 * 1.5) + 24


def translate(s, lo):
    s = dict(s)
    lo = np.asarray(lo, dtype=np.float64)
    s["x"] = s["x"] + lo
    s["box"] = np.asarray(s["box"], dtype=np.float64) + lo[:, None]
    return s


def serpentine(nx, ny, nz, density=0.85, seed=1, jitter=0.03, temp=1.0):
    """lattice_chain's geometry in a non-cubic box: one chain along a serpentine path through an nx x ny x nz lattice."""
    rng = np.random.RandomState(seed)
    n = nx * ny * nz
    a = (1.0 / density) ** (1.0 / 3.0)
    k = np.arange(n)
    iz = k // (nx * ny)
    yy = (k % (nx * ny)) // nx
    col = k % nx
    iy = np.where(iz % 2 == 0, yy, ny - 1 - yy)
    ix = np.where((k // nx) % 2 == 0, col, nx - 1 - col)
    x = np.stack([ix, iy, iz], axis=1).astype(np.float64) * a + 0.5 * a + rng.uniform(-jitter, jitter, size=(n, 3))
    v = rng.normal(0.0, np.sqrt(temp), size=(n, 3))
    v -= v.mean(axis=0)
    bonds = np.array([(1, i + 1, i + 2) for i in range(n - 1)], dtype=np.int32)
    return dict(box=np.array([[0.0, nx * a], [0.0, ny * a], [0.0, nz * a]]), x=x, v=v, type=np.ones(n, dtype=np.int32),
                mol=np.ones(n, dtype=np.int32), image=np.zeros((n, 3), dtype=np.int32), bonds=bonds, ntypes=1, nbondtypes=2,
                mass=[1.0], extra_bond=1, extra_special=20, atom_style="bond")


def add_free_beads(s, pts):
    """Unbonded beads of type 1 behind the chain's (tags n+1 ..), at rest."""
    s = dict(s)
    m = len(pts)
    s["x"] = np.concatenate([s["x"], np.asarray(pts, dtype=np.float64).reshape(m, 3)])
    s["v"] = np.concatenate([s["v"], np.zeros((m, 3))])
    s["type"] = np.concatenate([s["type"], np.ones(m, dtype=np.int32)])
    s["mol"] = np.concatenate([s["mol"], np.zeros(m, dtype=np.int32)])
    s["image"] = np.concatenate([s["image"], np.zeros((m, 3), dtype=np.int32)])
    return s


# ------------------------------------------------------------------------------------------------
# scenarios 1 and 2: the chain, translated, and in a box with three different cell counts
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_at(origin):
    return translate(lattice_chain(4096), ORIGINS[origin])


NONCUBIC = (6, 25, 28)          # lattice sites: cells (16, 17, 19) - one full 16-row tile and a partial one in y and in z
NONCUBIC_CELLS = (16, 17, 19)


@functools.lru_cache(maxsize=None)
def noncubic_chain(origin=1, nz=NONCUBIC[2], seed=4):
    return translate(serpentine(NONCUBIC[0], NONCUBIC[1], nz, seed=seed), ORIGINS[origin])


# ------------------------------------------------------------------------------------------------
# scenario 3: the cutoff ladder
# ------------------------------------------------------------------------------------------------
DELTA_RUNGS = (4.0, 64.0, 1e3, 1e5, 1e7)          # gap = m * delta
BAND_RUNGS = (0.25, 0.5, 0.9, 1.1, 2.0)           # gap = f * FP32 band


def _unit(rng, kind, d):
    """Direction of a probe pair: `axis` = along dimension d, `toward` = random with a component >= 0.7 along d,
    `edge` / `corner` = pointing out through two / three faces, `any` = uniform on the sphere."""
    if kind == "axis":
        u = np.zeros(3); u[d] = 1.0
        return u
    if kind == "any":
        u = rng.normal(size=3)
        return u / np.linalg.norm(u)
    if kind == "toward":
        w = rng.uniform(0.7, 0.98)
        t = rng.normal(size=2); t *= np.sqrt(1.0 - w * w) / np.linalg.norm(t)
        u = np.zeros(3); u[d] = w; u[[k for k in range(3) if k != d]] = t
        return u
    if kind == "edge":          # out through the faces of the two dimensions other than d
        a, b = rng.uniform(0.55, 0.7, size=2)
        u = np.zeros(3); u[[k for k in range(3) if k != d]] = (a, b); u[d] = rng.choice([-1.0, 1.0]) * np.sqrt(1.0 - a * a - b * b)
        return u
    u = 1.0 + rng.uniform(-0.1, 0.1, size=3)      # corner
    return u / np.linalg.norm(u)


def _probe(rng, box, place, dirkind, d, side, target, accept, plane=None, tries=200):
    """One probe pair (p, q) at separation^2 = cutneigh^2 + side * target, realised on doubles: q is rounded and wrapped the
    way the engine wraps (one addition of the box length), then the pair is measured in long double; a pair whose gap has
    the wrong sign or lies outside `accept` x target (e.g. because a coordinate's ulp is wider than the rung) is drawn
    again.  None if no draw succeeds."""
    lo, hi = box[:, 0], box[:, 1]
    prd = hi - lo
    c = CUTNEIGH
    dl = delta(box, c)
    c2 = LD(c) * LD(c)
    for _ in range(tries):
        if (prd > 4.3 * c).all():
            p = lo + 2.1 * c + rng.uniform(size=3) * (prd - 4.2 * c)          # deep inside: both beads interior
        else:                                    # (a box narrower than four cutoffs has no such place)
            assert place == "plane"
            p = lo + rng.uniform(0.02, 0.98, size=3) * prd
        if place == "face":                      # q leaves through the upper face of dimension d
            p[d] = hi[d] - rng.uniform(0.05, 0.6) * c
        elif place == "edge":
            for k in range(3):
                if k != d:
                    p[k] = hi[k] - rng.uniform(0.05, 0.4) * c
        elif place == "corner":
            p = hi - rng.uniform(0.05, 0.3, size=3) * c
        elif place == "nearface":                # p within the margin of the lower face, q interior
            p[d] = lo[d] + rng.uniform(0.4, 0.9) * c
        elif place == "plane":                   # q on the other side of the plane z = plane
            p[2] = plane - rng.uniform(0.05, 0.6) * c
        u = _unit(rng, dirkind, d)
        r = np.sqrt(c2 + LD(side) * LD(target))
        q = np.array([float(LD(p[k]) + r * LD(u[k])) for k in range(3)])
        for k in range(3):
            if q[k] >= hi[k]:
                q[k] -= prd[k]
            if q[k] < lo[k]:
                q[k] += prd[k]
        if not ((q >= lo).all() and (q < hi).all() and (p >= lo).all() and (p < hi).all()):
            continue
        g = sep2_ld(p, q, box) - c2
        if (g > 0) != (side > 0) or abs(g) <= LD(dl):
            continue
        if not (accept[0] * target <= abs(float(g)) <= accept[1] * target):
            continue
        return p, q, float(g)
    return None


def _ladder_probes(rng, box, combos, reps):
    dl, band = delta(box, CUTNEIGH), fp32_band(box, CUTNEIGH)
    rungs = [("delta", m, m * dl, (0.5, 2.0)) for m in DELTA_RUNGS] + [("band", f, f * band, (0.97, 1.03)) for f in BAND_RUNGS]
    pts, meta = [], []
    for place, dirkind, d, plane in combos:
        for _ in range(reps):
            for rk, rv, target, accept in rungs:
                for side in (-1, 1):
                    got = _probe(rng, box, place, dirkind, d, side, target, accept, plane)
                    if got is None:
                        continue
                    p, q, g = got
                    meta.append(dict(place=place, direction=dirkind, dim=d, rung=(rk, rv), side=side, gap=g, row=len(pts)))
                    pts += [p, q]
    return np.array(pts), meta


@functools.lru_cache(maxsize=None)
def ladder(origin):
    """The chain of scenario 1 at ORIGINS[origin] plus probe pairs at separations cutneigh * sqrt(1 + s * t): returns
    (system, meta); meta[k]["row"] = index of the pair's first bead among the added beads (tags n + 1 + row, + 2 + row)."""
    base = chain_at(origin)
    box = np.asarray(base["box"])
    rng = np.random.RandomState(100 + origin)
    combos = [("deep", "axis", 0, None), ("deep", "axis", 1, None), ("deep", "axis", 2, None), ("deep", "any", 0, None),
              ("deep", "any", 1, None), ("deep", "any", 2, None)]
    for d in range(3):
        combos += [("face", "axis", d, None), ("face", "toward", d, None), ("nearface", "axis", d, None),
                   ("nearface", "toward", d, None)]
    combos += [("edge", "edge", 2, None), ("edge", "edge", 0, None), ("corner", "corner", 0, None)]
    pts, meta = _ladder_probes(rng, box, combos, 1)
    return add_free_beads(base, pts), meta


# ------------------------------------------------------------------------------------------------
# scenario 4: a dense cluster
# ------------------------------------------------------------------------------------------------
CLUSTER_BEADS, CLUSTER_RADIUS = 300, 0.3


@functools.lru_cache(maxsize=None)
def dense_cluster(origin=1):
    base = translate(lattice_chain(4096, seed=2), ORIGINS[origin])
    box = np.asarray(base["box"])
    ncx, ncy, ncz = cell_counts(box)
    prd = box[:, 1] - box[:, 0]
    centre = box[:, 0] + np.array([0.5 * prd[0], (ncy // 2 + 0.5) * prd[1] / ncy, (ncz // 2 + 0.5) * prd[2] / ncz])
    rng = np.random.RandomState(7)
    u = rng.normal(size=(CLUSTER_BEADS, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    pts = centre + u * (CLUSTER_RADIUS * rng.uniform(size=(CLUSTER_BEADS, 1)) ** (1.0 / 3.0))
    return add_free_beads(base, pts)


# ------------------------------------------------------------------------------------------------
# scenario 5: faces and cell boundaries
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def faces(origin):
    base = chain_at(origin)
    box = np.asarray(base["box"])
    lo, hi = box[:, 0], box[:, 1]
    prd = hi - lo
    nc = cell_counts(box)
    rng = np.random.RandomState(300 + origin)
    inside = lambda: lo + rng.uniform(0.1, 0.9, size=3) * prd
    pts = []
    for d in range(3):
        cellinv = nc[d] / prd[d]
        special = [lo[d], np.nextafter(hi[d], lo[d]), hi[d], np.nextafter(hi[d], np.inf), hi[d] + 1e-7,
                   np.nextafter(lo[d], -np.inf), lo[d] - 1e-7]
        for k in (1, 2, nc[d] // 2, nc[d] - 1):
            b = lo[d] + k / cellinv
            special += [b, np.nextafter(b, -np.inf), np.nextafter(b, np.inf)]
        for val in special:
            p = inside()
            p[d] = val
            pts.append(p)
    pts += [lo.copy(), hi.copy(), np.nextafter(hi, lo), np.array([lo[0], hi[1], np.nextafter(hi[2], lo[2])])]
    return add_free_beads(base, np.array(pts))


# ------------------------------------------------------------------------------------------------
# scenario 6: special neighbors
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def special_chain(hub):
    """Chain with a few (i, i+2) bonds of type 2; `hub`: one bead is also bonded to four beads that are close in space but
    far along the chain (six partners in all - more relevant special entries than the list build keeps in registers)."""
    s = dict(lattice_chain(3000, seed=5, jitter=0.08))
    n = len(s["x"])
    extra = [(2, i, i + 2) for i in range(10, n - 10, 37)]
    if hub:
        busy = set()
        for _, a, b in extra:
            busy.update(range(a - 4, b + 5))
        h = next(t for t in range(n // 2, n) if not (set(range(t - 8, t + 9)) & busy))
        d = np.linalg.norm(s["x"] - s["x"][h - 1], axis=1)
        picked = []
        for j in np.argsort(d):
            t = int(j) + 1
            if abs(t - h) <= 8 or d[j] > 2.5 or set(range(t - 4, t + 5)) & busy:
                continue
            if all(abs(t - q) > 8 for q in picked):
                picked.append(t)
            if len(picked) == 4:
                break
        assert len(picked) == 4
        extra += [(2, h, t) for t in picked]
        s["hub"] = h
        s["extra_bond"], s["extra_special"] = 0, 0
    s["bonds"] = np.concatenate([s["bonds"], np.array(extra, dtype=np.int32)])
    return s


SPECIAL_CASES = {          # name: (special_bonds arguments, lj weights, coul weights, system with the hub)
    "fene-bond-table": ("fene", (0.0, 1.0, 1.0), (0.0, 1.0, 1.0), False),
    "fene-hub": ("fene", (0.0, 1.0, 1.0), (0.0, 1.0, 1.0), True),
    "lj-0-0-0": ("lj 0.0 0.0 0.0", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), True),
    "lj-fractional": ("lj 0.0 0.3 0.7", (0.0, 0.3, 0.7), (0.0, 0.0, 0.0), True),
    "lj-0-1-1-coul-1-1-1": ("lj 0.0 1.0 1.0 coul 1.0 1.0 1.0", (0.0, 1.0, 1.0), (1.0, 1.0, 1.0), True),
    "lj-1-1-1": ("lj 1.0 1.0 1.0", (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), True),
}


# ------------------------------------------------------------------------------------------------
# scenarios 8 and 9: rebuilds inside a run; z slabs
# ------------------------------------------------------------------------------------------------
def rebuild_chain():
    return noncubic_chain(origin=2)


DD_NZ = 30          # lattice layers: the box is 31.7 tall - three slabs of at least two ghost cutoffs (2 x 5.0) each


@functools.lru_cache(maxsize=None)
def slab_ladder():
    """Non-cubic chain at ORIGINS[1], tall enough for three z slabs, plus ladder probes across the slab boundaries of a
    2-rank and a 3-rank run and across the periodic z face."""
    base = noncubic_chain(origin=1, nz=DD_NZ, seed=6)
    box = np.asarray(base["box"])
    lo, prd = box[2, 0], box[2, 1] - box[2, 0]
    rng = np.random.RandomState(900)
    combos = []
    for plane in (box[2, 1], lo + prd / 2, lo + prd / 3, lo + 2 * (prd / 3)):
        combos += [("plane", "axis", 2, plane), ("plane", "toward", 2, plane)]
    pts, meta = _ladder_probes(rng, box, combos, 1)
    return add_free_beads(base, pts), meta


# ------------------------------------------------------------------------------------------------
# scenario 8b: the rebuild trigger at the edge of its FP32 band
# ------------------------------------------------------------------------------------------------
TRIGGER_STEPS = 10
TRIGGER_BUILDS = {+1: 0, -1: 1}          # rebuilds within a run of TRIGGER_STEPS steps (see trigger_probe)
# lj/cut with epsilon 0: the pair list of CHAIN_SCRIPT, no pair force, and a script the oracle can run too
EPS0_SCRIPT = CHAIN_SCRIPT.replace("pair_coeff * * 1.0 1.0 1.12", "pair_coeff * * 0.0 1.0 1.12")
assert EPS0_SCRIPT != CHAIN_SCRIPT


@functools.lru_cache(maxsize=None)
def trigger_probe(sign):
    """The chain at ORIGINS[2], at rest, plus ONE free bead that flies along x (EPS0_SCRIPT: no pair force acts on it).  The
    step kernel tests |x - x_build|^2 > (skin/2)^2 against the FLOAT copy of x_build first and repeats the test in FP64
    inside an error band.  The bead starts 0.4 float-ulps (1e-4 at |x| ~ 4000) above (sign +1) or below (-1) a float, so the
    float copy is off by that much, and its speed puts the true displacement of the tenth step 5e-5 below (+1) or above
    (-1) the threshold 0.2, while the float copy alone says the opposite.  In FP64 a run of TRIGGER_STEPS steps therefore
    ends with TRIGGER_BUILDS[sign] rebuilds; test_neigh_reference_cpu.py pins that to the oracle, and shows that one step
    less / more gives 0 / 1 for both signs (the chain itself, pushed by its bonds, has moved 0.1 by then)."""
    base = dict(chain_at(2))
    base["v"] = np.zeros_like(base["v"])
    box = np.asarray(base["box"])
    centre = 0.5 * (box[:, 0] + box[:, 1])
    f = np.float32(centre[0])
    ulp = float(np.spacing(f))
    p = np.array([float(f) + sign * 0.4 * ulp, centre[1], centre[2]])
    assert float(np.float32(p[0])) == float(f)
    s = add_free_beads(base, [p])
    s["v"][-1, 0] = (0.2 - sign * 5e-5) / 10 / 0.005
    return s


# ------------------------------------------------------------------------------------------------
# scenario 3b: wavefronts that are wholly interior - and wavefronts that only a halved margin would call interior
# ------------------------------------------------------------------------------------------------
ALIGNED_BOX = (10.0, 4.6, 4.6)          # cells 26 x 3 x 3
# x zones of 64 beads each in every (y, z) row of cells, no two zones in one x cell: a row holds 5 x 64 beads, so every
# wavefront of the list build (64 consecutive beads of the cell order) is one zone of one row
ALIGNED_ZONES = ((0.02, 0.70), (0.80, 1.45), (1.60, 8.40), (8.55, 9.20), (9.30, 9.98))


@functools.lru_cache(maxsize=None)
def aligned_rows(origin=1):
    """Free beads only (no bonds).  In the row of cells in the middle of the box the beads of zone 3 are farther than cutneigh
    from every face: their wavefront skips the minimum image.  Zones 2 and 4 lie between cutneigh / 2 and cutneigh from an
    x face: their wavefronts must NOT skip it - their beads have neighbors in zones 5 and 1 across the face."""
    rng = np.random.RandomState(77)
    L = np.array(ALIGNED_BOX)
    ncy, ncz = cell_counts(np.stack([0 * L, L], axis=1))[1:]
    pts = []
    for cz in range(ncz):
        for cy in range(ncy):
            for lo, hi in ALIGNED_ZONES:
                p = np.empty((64, 3))
                p[:, 0] = rng.uniform(lo, hi, size=64)
                p[:, 1] = (cy + rng.uniform(0.01, 0.99, size=64)) * L[1] / ncy
                p[:, 2] = (cz + rng.uniform(0.01, 0.99, size=64)) * L[2] / ncz
                pts.append(p)
    pts = np.concatenate(pts)
    pts = pts[rng.permutation(len(pts))]          # tags carry no order
    n = len(pts)
    s = dict(box=np.stack([0 * L, L], axis=1), x=pts, v=np.zeros((n, 3)), type=np.ones(n, dtype=np.int32),
             mol=np.zeros(n, dtype=np.int32), image=np.zeros((n, 3), dtype=np.int32), bonds=np.zeros((0, 3), dtype=np.int32),
             ntypes=1, nbondtypes=2, mass=[1.0], extra_bond=1, extra_special=2, atom_style="bond")
    return translate(s, ORIGINS[origin])
