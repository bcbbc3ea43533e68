"""Inputs of the force tests (test_gpu_force.py) - shared with test_force_reference_cpu.py, which proves without a GPU that
none of them holds a pair the cutoff test could judge either way, and measures how far the FP64 oracle is from the
long-double reference (force_reference.py) on each: the GPU tolerances are 16 x those figures (force_compare.py).

The smallest shapes at which the force kernels can still go wrong: at most ~800 beads (one brute-force evaluation in long
double costs about a second), bead counts that are no multiple of 64, boxes of three cells per edge and boxes with three
different cell counts, coordinates far from the origin.

WHOEVER CHANGES A SEED: the seeds are not arbitrary.  The bound of a GPU test is 16 x the oracle's own deviation from the
reference and must not exceed 1e-12 for one evaluation (force_compare.bound asserts it: an input that needs more is the wrong
input).  The oracle's deviation of the run-0 forces is the maximum over ~2000 force components of sums of terms of size
50 - 100 and varies between 3e-14 and 1e-13 from seed to seed, so 16 x it lies between 5e-13 and 1.6e-12 - at the edge of
the ceiling.  The seeds here are ones under it: the force bounds in use are 2.6e-13 (aligned) to 8.9e-13 (angles-cosine).  With
another seed bound() may assert in test_force_reference_cpu.py and in every GPU test of that input; then take the next seed,
the rule stays.

Every chain is displaced by a fraction of the box WITHOUT moving the box, so
read_data wraps it and bonds and angles cross all three pairs of faces at setup.  Everything is seeded."""
import functools

import numpy as np

from neigh_inputs import ORIGINS, add_free_beads, serpentine, translate

DISPLACE = (0.37, 0.61, 0.43)          # fractions of the box edges


def displace(s, frac=DISPLACE):
    s = dict(s)
    box = np.asarray(s["box"], dtype=np.float64)
    s["x"] = s["x"] + np.asarray(frac) * (box[:, 1] - box[:, 0])
    return s


def hot(s, temp):
    """Maxwell velocities of serpentine() (temperature 1) scaled: fast enough for three list rebuilds in twelve steps."""
    s = dict(s)
    s["v"] = s["v"] * np.sqrt(temp)
    return s


def interstitial(s, sites):
    """Points in the middle of lattice cubes of an undisplaced serpentine() system (sites: integer triples): 0.91 from the
    eight beads around them."""
    a = (np.asarray(s["box"])[:, 1] - np.asarray(s["box"])[:, 0]) / np.asarray(s["lattice"])
    return np.asarray(s["box"])[:, 0] + (np.asarray(sites, dtype=np.float64) + 1.0) * a


def lattice(nx, ny, nz, **kw):
    s = serpentine(nx, ny, nz, **kw)
    s["lattice"] = (nx, ny, nz)
    return s


HEAD = """
units lj
atom_style %(atom_style)s
newton off
atom_modify sort 0 0
special_bonds %(special)s
read_data data.force
neighbor %(skin)s bin
neigh_modify every 1 delay 1 check yes
comm_modify cutoff 2.0
"""
FENE = "bond_style fene\nbond_coeff 1 30.0 1.5 1.0 1.0\nbond_coeff 2 30.0 4.0 1.0 1.0\n"
WCA = "pair_style lj/cut 1.12\npair_modify shift yes\npair_coeff * * 1.0 1.0 1.12\n"


def script(case, skin="0.4", norm=None):
    """The script of an input up to (not including) the fixes and the run command."""
    text = HEAD % dict(atom_style=case.get("atom_style", "bond"), special=case.get("special", "fene"), skin=skin)
    text += case["force_field"] + "timestep 0.005\n"
    if norm is not None:
        text += "thermo_modify norm %s\n" % norm
    return text


# ------------------------------------------------------------------------------------------------
# tiny: three cells per edge - every cell is a boundary cell, the middle third of each axis is interior by `margin`
# ------------------------------------------------------------------------------------------------
TINY_EDGE = 1.01 * 3 * (1.12 + 0.4)


@functools.lru_cache(maxsize=None)
def tiny():
    s = lattice(4, 4, 5, seed=11)
    scale = TINY_EDGE / np.asarray(s["box"])[:, 1]          # 80 sites in a cube of 4.6: spacings 1.15, 1.15, 0.92
    s["x"], s["box"] = s["x"] * scale, np.asarray(s["box"]) * scale[:, None]
    s = add_free_beads(s, interstitial(s, [(0, 0, 0), (2, 1, 3), (1, 2, 1)]))          # 83 beads
    return dict(system=hot(displace(s), 6.0), force_field=FENE + WCA)


# ------------------------------------------------------------------------------------------------
# offset: three different cell counts, coordinates far from the origin, interior and non-interior wavefronts.
# The origin is ORIGINS[1] / 32 = (-1.16, 31.3, -64.0), not ORIGINS[1] itself: at |z| ~ 2048 the reference program's own
# arithmetic (x_j + prd for a partner across a face, rounded to an ulp of 4.5e-13) puts the FP64 oracle 1.5e-12 from the
# long-double forces at run 0, and 16 x that is above the 1e-12 every single evaluation has to meet - by the rule of
# bound() below such an input is the wrong input.  At 64 the oracle is within 6e-14.
# ------------------------------------------------------------------------------------------------
OFFSET_ORIGIN = tuple(c / 32.0 for c in ORIGINS[1])

@functools.lru_cache(maxsize=None)
def offset(pinned=False):
    s = translate(lattice(5, 9, 14, seed=22), OFFSET_ORIGIN)
    if pinned:          # every seventh bead is of type 2: outside the group fix nve acts on
        n = len(s["x"])
        s["type"] = 1 + (np.arange(n) % 7 == 0).astype(np.int32)
        s["ntypes"], s["mass"] = 2, [1.0, 1.0]
    return dict(system=hot(displace(s), 5.0), force_field=FENE + WCA)


# ------------------------------------------------------------------------------------------------
# census: the geometry of offset at 2145 beads (33 wavefronts and 33 beads: with one lane per bead nine workgroups, a count
# the launch grid pads; far under the 50000 beads up to which four lanes share a bead) - the input of the launch-census rows
# that carry a wall, an indenter, a tether or another pair style (census_runs.py, whose reference prunes the candidate pairs:
# at this size the plain brute force costs seven seconds an evaluation)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def census():
    s = translate(lattice(11, 13, 15, seed=23), OFFSET_ORIGIN)
    return dict(system=hot(displace(s), 5.0), force_field=FENE + WCA)


# ------------------------------------------------------------------------------------------------
# types: three atom types, per-pair cutoffs 1.0 .. 2.5 without a shift - a pair on the wrong side of a cutoff shows
# ------------------------------------------------------------------------------------------------
TYPES_FF = FENE + """pair_style lj/cut 2.5
pair_modify shift no mix arithmetic
pair_coeff 1 1 1.0 1.0 2.5
pair_coeff 2 2 0.8 1.05 1.6
pair_coeff 3 3 1.2 0.95 1.12
pair_coeff 1 2 0.0 1.0 1.0
pair_coeff 2 3 0.6 0.97 1.0
"""          # 1-3 is mixed: eps sqrt(1.2), sigma 0.975, cutoff 1.81


@functools.lru_cache(maxsize=None)
def types():
    s = lattice(9, 9, 9, seed=30)
    n = len(s["x"])
    s["type"] = (1 + (np.arange(n) * 7 // 3) % 3).astype(np.int32)
    s["ntypes"], s["mass"] = 3, [1.0, 1.7, 0.6]
    return dict(system=hot(displace(s), 5.0), force_field=TYPES_FF)


# ------------------------------------------------------------------------------------------------
# hubs: hybrid bonds, fractional special weights, beads with 0 to 6 bonds, free beads, a bead without any neighbor, a
# FENE bond inside the clamp
# ------------------------------------------------------------------------------------------------
HUBS_FF = """bond_style hybrid fene harmonic morse
bond_coeff 1 fene 30.0 1.5 1.0 1.0
bond_coeff 2 harmonic 10.0 1.2
bond_coeff 3 morse 5.0 2.0 1.1
""" + WCA
# bond morse lives in the unfused force kernel only (a system with a morse bond never takes the step kernel): the same
# geometry with a second harmonic type in its place is what the step-kernel shapes run
HUBS_HARMONIC_FF = HUBS_FF.replace("hybrid fene harmonic morse", "hybrid fene harmonic").replace("bond_coeff 3 morse 5.0 2.0 1.1", "bond_coeff 3 harmonic 8.0 1.1")
assert "morse" not in HUBS_HARMONIC_FF
HOLE_RADIUS = 1.12 + 0.4 + 0.25          # cutneigh plus the most two beads are jittered towards each other, with a margin


@functools.lru_cache(maxsize=None)
def hubs():
    base = lattice(5, 6, 8, seed=22)
    x0 = base["x"]
    n0 = len(x0)
    lone = 5 * 6 * 4 + 5 * 3 + 2          # a site in the middle of the lattice: it keeps its place, the sites around it go
    d = np.linalg.norm(x0 - x0[lone], axis=1)
    keep = (d > HOLE_RADIUS) | (np.arange(n0) == lone)
    new = np.cumsum(keep) - 1          # row after the removal
    x = x0[keep]
    n = len(x)
    # chain bonds between sites that were consecutive and both stay (the lone bead has none)
    bonds = [(1, new[k] + 1, new[k + 1] + 1) for k in range(n0 - 1) if keep[k] and keep[k + 1] and lone not in (k, k + 1)]
    # hubs: beads bonded (harmonic / morse) to beads next to them in space (lattice neighbors and face diagonals, up to 1.6)
    rng = np.random.RandomState(140)
    hubs_at, taken = {}, {int(new[lone])}
    for extra in (4, 3, 2, 1):          # 6, 5, 4, 3 bonds with the two chain bonds
        for h in rng.permutation(n):
            near = [int(j) for j in np.argsort(np.linalg.norm(x - x[h], axis=1))[1:12]
                    if abs(int(j) - int(h)) > 3 and np.linalg.norm(x[j] - x[h]) < 1.6]
            zone = set(range(int(h) - 8, int(h) + 9))
            if len(near) >= extra and not (zone & taken) and not any(set(range(j - 2, j + 3)) & taken for j in near[:extra]):
                hubs_at[int(h) + 1] = [j + 1 for j in near[:extra]]
                taken |= zone
                for j in near[:extra]:
                    taken |= set(range(j - 2, j + 3))
                break
        else:
            raise AssertionError("no place for a hub with %d extra bonds" % extra)
    for h, partners in hubs_at.items():
        bonds += [(2 + k % 2, h, p) for k, p in enumerate(partners)]
    s = dict(base)
    s.update(x=x, v=base["v"][keep], type=np.ones(n, dtype=np.int32), mol=np.ones(n, dtype=np.int32),
             image=np.zeros((n, 3), dtype=np.int32), nbondtypes=3, extra_bond=0, extra_special=0)
    # free beads among the chain's, and a dimer of two more, a face diagonal apart: a FENE bond of 1.493 - rlogarg 0.009
    free = interstitial(base, [(0, 0, 0), (3, 4, 6), (1, 1, 1), (2, 0, 5), (0, 4, 2)])
    dimer = interstitial(base, [(3, 1, 0), (3, 2, 1)])
    assert min(np.linalg.norm(p - x[new[lone]]) for p in np.concatenate([free, dimer])) > HOLE_RADIUS
    s = add_free_beads(s, np.concatenate([free, dimer]))
    s["v"][n:n + 5] = np.random.RandomState(141).normal(size=(5, 3))
    bonds.append((1, n + 6, n + 7))
    s["bonds"] = np.array(bonds, dtype=np.int32)
    return dict(system=hot(displace(s), 5.0), force_field=HUBS_FF, special="lj 0.0 0.3 0.7", lone=int(new[lone]) + 1,
                hubs=hubs_at, clamped=(n + 6, n + 7))


# ------------------------------------------------------------------------------------------------
# angles: the offset geometry with an angle on every backbone triple, a hub of angles and an exactly straight triple
# ------------------------------------------------------------------------------------------------
ANGLE_FF = {"harmonic": "angle_style harmonic\nangle_coeff 1 3.0 170.0\nangle_coeff 2 1.0 120.0\n",
            "cosine": "angle_style cosine\nangle_coeff 1 2.5\nangle_coeff 2 0.5\n"}
STRAIGHT = 5 * 9 * 6 + 5 * 4 + 2          # row of the middle bead of the straight triple: the middle of a lattice row along x


@functools.lru_cache(maxsize=None)
def angles(style):
    s = translate(lattice(5, 9, 14, seed=29), OFFSET_ORIGIN)
    n = len(s["x"])
    # the lattice rows are bent into a zigzag (every other bead 0.07 off in y and z: backbone angles near 159 degrees): left
    # nearly straight, the harmonic style's 1 / sin(theta)^3 would amplify the FP64 rounding of cos(theta) beyond what a single
    # evaluation is allowed to be off by
    x = s["x"] + ((-1.0) ** np.arange(n))[:, None] * np.array([0.0, 0.07, 0.07])
    # exactly straight along x, one apart: cos(theta) comes out as -1 in every precision (sqrt(fl(d * d)) = |d|), so the clamp
    # of the harmonic style is entered and the angle is not at the mercy of acos near -1
    k = STRAIGHT
    x[k - 1] = x[k] - np.array([1.0, 0.0, 0.0])
    x[k + 1] = x[k] + np.array([1.0, 0.0, 0.0])
    s["x"] = x
    ang = [(1, i, i + 1, i + 2) for i in range(1, n - 1)]
    # a hub: one bead is the vertex of an angle (type 2) between every two of the five beads nearest to it off its own
    # stretch of chain - 10 angles on top of the three backbone angles it is listed in
    h = 5 * 9 * 3 + 5 * 4 + 2
    near = [int(j) for j in np.argsort(np.linalg.norm(x - x[h], axis=1))[1:] if abs(int(j) - h) > 2][:5]
    ang += [(2, near[a] + 1, h + 1, near[b] + 1) for a in range(5) for b in range(a + 1, 5)]
    s.update(nangletypes=2, angles=np.array(ang, dtype=np.int32), extra_angle=24, atom_style="molecular")
    return dict(system=hot(displace(s), 5.0), force_field=FENE + WCA + ANGLE_FF[style], atom_style="molecular",
                hub=h + 1, straight=(k, k + 1, k + 2))


# ------------------------------------------------------------------------------------------------
# all-FENE in a box large enough for the per-step minimum image of the bonds (Engine: bond_minimg) - and hubs, which is not
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fene_large():
    s = lattice(6, 7, 9, seed=21)          # shortest edge 6.33 > 4 R0 = 6
    return dict(system=hot(displace(s), 5.0), force_field=FENE.replace("30.0 4.0", "30.0 1.5") + WCA)


# ------------------------------------------------------------------------------------------------
# aligned: wavefronts that are wholly interior - and wavefronts that only a halved margin would call interior.
# neigh_inputs.aligned_rows' zones in the ONE row of cells in the middle of its box (interior in y and z): five zones of 64 free
# beads, no two zones in one x cell, so every wavefront of 64 consecutive beads of the cell order is one zone.  Zone 3 is
# farther than cutneigh from every face: its wavefront skips the minimum image of the pair terms.  Zones 2 and 4 lie between
# cutneigh / 2 and cutneigh from an x face and have neighbors in zones 5 and 1 across it: theirs must not.  The beads sit on a
# 4 x 4 x 4 grid per zone (0.16 apart at the least) under lj/cut with sigma 0.08: forces of order 10, nothing singular (sigma 0.12 - terms of order 100 - puts the oracle 1.4e-13 from the reference: too much by the rule of bound()).
# ------------------------------------------------------------------------------------------------
ALIGNED_CONTRACTION = 6.6
ALIGNED_FF = FENE + "pair_style lj/cut 1.12\npair_modify shift no\npair_coeff * * 1.0 0.08 1.12\n"


@functools.lru_cache(maxsize=None)
def aligned():
    from neigh_inputs import ALIGNED_BOX, ALIGNED_ZONES, cell_counts
    rng = np.random.RandomState(78)
    L = np.array(ALIGNED_BOX)
    box = np.stack([0 * L, L], axis=1)
    ncy, ncz = cell_counts(box)[1:]
    assert (ncy, ncz) == (3, 3)
    g = (np.arange(4) + 0.5) / 4
    pts = []
    for lo, hi in ALIGNED_ZONES:
        gx, gy, gz = np.meshgrid(lo + g * (hi - lo), (1 + g) * L[1] / ncy, (1 + g) * L[2] / ncz, indexing="ij")
        pts.append(np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1) + rng.uniform(-0.01, 0.01, size=(64, 3)))
    pts = np.concatenate(pts)
    pts = pts[rng.permutation(len(pts))]          # tags carry no order
    n = len(pts)
    # velocities: the row of cells contracts towards its axis (up to 5.4 at the corners of the grids: more than half the skin in
    # four steps, three list builds after the first in twelve) with a little noise on top.  Nothing moves more than 0.05 along x or leaves the
    # row of cells: after every rebuild the wavefronts are still the zones, zone 3 is still interior, zones 2 and 4 still not
    v = rng.normal(scale=0.2, size=(n, 3))
    v[:, 1:] -= ALIGNED_CONTRACTION * (pts[:, 1:] - 0.5 * L[1:])
    s = dict(box=box, x=pts, v=v, type=np.ones(n, dtype=np.int32), mol=np.zeros(n, dtype=np.int32),
             image=np.zeros((n, 3), dtype=np.int32), bonds=np.zeros((0, 3), dtype=np.int32), ntypes=1, nbondtypes=2, mass=[1.0],
             extra_bond=1, extra_special=2, atom_style="bond")
    return dict(system=translate(s, OFFSET_ORIGIN), force_field=ALIGNED_FF)


INPUTS = {"tiny": tiny, "aligned": aligned, "offset": offset, "census": census, "offset-pinned": lambda: offset(True), "types": types, "hubs": hubs,
          "hubs-harmonic": lambda: dict(hubs(), force_field=HUBS_HARMONIC_FF),
          "angles-harmonic": lambda: angles("harmonic"), "angles-cosine": lambda: angles("cosine"), "fene-large": fene_large}
# which bond-image path the engine takes (stat bond_minimg): the frozen image words unless every bond style is FENE and the
# shortest box edge exceeds four times the largest R0
BOND_MINIMG = {"tiny": 0, "offset": 0, "census": 0, "offset-pinned": 0, "types": 0, "hubs": 0, "hubs-harmonic": 0, "aligned": 0, "angles-harmonic": 0, "angles-cosine": 0,
               "fene-large": 1}
