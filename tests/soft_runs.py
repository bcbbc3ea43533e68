"""The scenarios of the recorded reference runs with pair_style soft and fix adapt (tests/golden/soft_*.npz, soft_runs.json) and
what the tests need to read them.  tests/golden/make_soft_runs.py runs the reference binary on each and stores numbers only;
test_soft_cpu.py holds the conditions on the fixtures, test_gpu_soft.py the HIP path.

(a) `run 0`: the 343-bead compressed lattice chain of wall_runs.a_system with 20 beads moved onto random points 0.1 to 0.3 from
    another, non-bonded bead, one bead placed exactly on another, two types with their own A and rc (the 1-2 pair mixed) and
    special_bonds lj 0.0 0.5 1.0.  The FENE bonds get R0 = 3 so that the bonds of a moved bead (up to ~1.8 long) stay far
    from their limit.
(b) 48 steps from the (a) system without the coincident pair, thermo every 4: the scenarios of SCENARIOS.
(c) the push-off: a phantom walk of 2000 beads under soft with ramp(0,60), then lj/cut; only the step count the reference
    needed and its closest pair are recorded.
"""
import json
import os

import numpy as np

import wall_runs as wl
from systems import CHAIN_SCRIPT

GOLDEN = wl.GOLDEN
SEED = 17
NMOVED = 20
SPECIAL = (0.0, 0.5, 1.0)
STEPS, THERMO_EVERY = 48, 4
THERMO = ("step", "temp", "epair", "emol", "etotal", "press")
A_THERMO = ("step", "evdwl", "press", "pxx", "pyy", "pzz", "pxy", "pxz", "pyz")
LANGEVIN_SEED = 48611

HEAD = (CHAIN_SCRIPT.replace("special_bonds fene", "special_bonds lj %g %g %g" % SPECIAL)
        .replace("bond_coeff 1 30.0 1.5 1.0 1.0", "bond_coeff 1 30.0 3.0 1.0 1.0")
        .replace("pair_style lj/cut 1.12\npair_modify shift yes\npair_coeff * * 1.0 1.0 1.12\n", "%s"))
assert HEAD.count("%s") == 1
SOFT_TYPED = "pair_style soft 1.12246\npair_coeff 1 1 12.0 1.0\npair_coeff 2 2 25.0 1.3\n"
SOFT_TYPED_ROWS = dict(cut=1.12246, rows=[(1, 1, 12.0, 1.0), (2, 2, 25.0, 1.3)])
FIXES = "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 %d\n" % LANGEVIN_SEED


def soft_system(coincident=True):
    """-> (system dict, moved [(bead, partner)], coincident (bead, partner) or None); rows are tags - 1"""
    s = wl.a_system()
    rng = np.random.RandomState(SEED)
    n = len(s["x"])
    x = s["x"].copy()
    s["type"] = (1 + (rng.rand(n) < 0.4)).astype(np.int32)
    s["ntypes"], s["mass"] = 2, [1.0, 1.0]
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2))
    moved, used = [], set()
    order = rng.permutation(np.arange(4, n - 4))
    for i in order:
        if len(moved) == NMOVED + (1 if coincident else 0):
            break
        if any(abs(i - u) <= 4 for u in used):
            continue
        # a lattice neighbor that is not within three bonds of i (its weight is 1) and is itself left where it is
        cand = [j for j in np.nonzero(d[i] < 1.2)[0] if abs(j - i) > 3 and all(abs(j - u) > 1 for u in used)]
        if len(moved) < 6:          # the first six: onto the second (1-3, weight 0.5) and the third (1-4, weight 1) bead along the chain,
            k = 2 if len(moved) < 3 else 3          # at a turn of the serpentine, where that bead is a lattice neighbor or nearly one
            cand = [int(i) + k] if d[i, i + k] < (1.6 if k == 2 else 1.2) and all(abs(i + k - u) > 1 for u in used) else []
        if not cand:
            continue
        j = int(cand[rng.randint(len(cand))])
        if len(moved) < NMOVED:
            u = rng.normal(size=3)
            x[i] = s["x"][j] + u / np.sqrt((u * u).sum()) * rng.uniform(0.1, 0.3)
        else:
            x[i] = s["x"][j]
        moved.append((int(i), j))
        used.update((int(i), j))
    assert len(moved) == NMOVED + (1 if coincident else 0)
    s["x"] = x
    box = np.asarray(s["box"])
    assert (x >= box[:, 0]).all() and (x < box[:, 1]).all()
    return s, moved[:NMOVED], (moved[NMOVED] if coincident else None)


def a_script():
    return HEAD % SOFT_TYPED + "fix 1 all nve\nthermo_style custom %s\nrun 0\n" % " ".join(A_THERMO)


def a_model(ntypes=2):
    import force_reference as fr
    import soft_reference as sr
    m = fr.model_from_script(HEAD % "", ntypes)
    m.pair = sr.soft_model_pair(SOFT_TYPED_ROWS["cut"], SOFT_TYPED_ROWS["rows"])
    return m


def a_reference():
    """(SoftSystem, evaluation of the (a) input, the input)"""
    import soft_reference as sr
    s, moved, same = soft_system(True)
    S = sr.SoftSystem(a_model(), s["box"], s["type"], s["mass"], s["bonds"])
    return S, S.evaluate(s["x"]), s


def a_counts(S, ev, s, same):
    """What the (a) input holds, as the fixture states it (soft_runs.json "conditions"): interacting pairs below half their
    cutoff, coincident pairs, interacting pairs two and three bonds apart (special weights 0.5 and 1) and farther, bonded
    pairs within their soft cutoff (weight 0: not in the list)."""
    iu, ju, d, fv = ev.terms["pair"]
    r = np.sqrt((d * d).sum(axis=1)).astype(np.float64)
    types = np.asarray(s["type"])
    cut = np.array([float(S.pair_coeffs[2][types[i], types[j]]) for i, j in zip(iu, ju)])
    x = np.asarray(s["x"])
    sep = np.abs(iu - ju)
    b = np.sqrt(((x[1:] - x[:-1]) ** 2).sum(axis=1))
    bcut = np.array([float(S.pair_coeffs[2][types[i], types[i + 1]]) for i in range(len(x) - 1)])
    return dict(below_half_cutoff=int((r < 0.5 * cut).sum()), coincident=int((r == 0.0).sum()), level_1_3=int((sep == 2).sum()),
                level_1_4=int((sep == 3).sum()), unweighted=int((sep > 3).sum()), bonded_within_cutoff=int((b < bcut).sum()))


def a_conditions(S, ev, s, moved, same):
    """'' when the (a) input holds what it is for"""
    iu, ju, d, fv = ev.terms["pair"]
    r = np.sqrt((d * d).sum(axis=1)).astype(np.float64)
    types = np.asarray(s["type"])
    cut = np.array([float(S.pair_coeffs[2][types[i], types[j]]) for i, j in zip(iu, ju)])
    if (r < 0.5 * cut).sum() < 15:
        return "only %d pairs below half their cutoff" % (r < 0.5 * cut).sum()
    if same is None or not np.array_equal(s["x"][same[0]], s["x"][same[1]]) or not (r == 0.0).any():
        return "no coincident pair among the interacting pairs"
    # special levels among the pairs within their cutoff: 1-2 (weight 0: dropped from the list - checked on all pairs), 1-3, 1-4
    x = np.asarray(s["x"])
    sep = np.abs(iu - ju)
    if not ((sep == 2).any() and (sep == 3).any() and (sep > 3).any()):
        return "a special level without an interacting pair"
    b = np.sqrt(((x[1:] - x[:-1]) ** 2).sum(axis=1))
    bcut = np.array([float(S.pair_coeffs[2][types[i], types[i + 1]]) for i in range(len(x) - 1)])
    if not (b < bcut).any():
        return "no bonded (1-2) pair within its soft cutoff"
    if len(set(types[[i for i, _ in moved]])) < 2 and len(set(types)) < 2:
        return "one type only"
    return ""


# ------------------------------------------------------------------------------------------------------------------
# (b): 48 steps with fix adapt
# ------------------------------------------------------------------------------------------------------------------
def _scn(name, pair, adapt, tail="run %d\n" % STEPS, fused=True):
    return dict(name=name, script=HEAD % pair + FIXES + adapt + "thermo %d\n" % THERMO_EVERY + tail, fused=fused)


UNIFORM = "pair_style soft 1.12246\npair_coeff * * 0.0\n"
RAMP = "variable A equal ramp(0,30)\n"
SCENARIOS = [
    _scn("adapt1", UNIFORM, RAMP + "fix push all adapt 1 pair soft a * * v_A\n"),
    _scn("adapt5", UNIFORM, RAMP + "fix push all adapt 5 pair soft a * * v_A\n"),
    _scn("scale", "pair_style soft 1.12246\npair_coeff 1 1 8.0\npair_coeff 2 2 12.0 1.2\n",
         "variable S equal ramp(0.5,2.5)\nfix push all adapt 1 pair soft a * * v_S scale yes\n"),
    _scn("reset", UNIFORM.replace("0.0", "4.0"), RAMP + "fix push all adapt 1 pair soft a * * v_A reset yes\n",
         tail="run %d\nrun 8\n" % STEPS),
    _scn("typed", "pair_style soft 1.12246\npair_coeff 1 1 0.0 1.0\npair_coeff 2 2 0.0 1.3\n",
         RAMP + "variable B equal ramp(0,45)\nfix push all adapt 1 pair soft a 1 1 v_A pair soft a 2 2 v_B\n"),
    # (lj/cut on beads 0.1 apart: sigma 0.1 and cutoff 0.3, only the 1-2 pairs interact and their epsilon grows from nothing)
    _scn("ljeps", "pair_style lj/cut 0.3\npair_modify shift yes\npair_coeff * * 0.0 0.1\npair_coeff 1 2 0.0 0.1\n",
         "variable E equal ramp(0,0.5)\nfix push all adapt 1 pair lj/cut epsilon 1 2 v_E\n", fused=False),
    _scn("respa", UNIFORM, RAMP + "fix push all adapt 1 pair soft a * * v_A\nrun_style respa 2 2\n", fused=False),
]
BY_NAME = {s["name"]: s for s in SCENARIOS}
NAMES = [s["name"] for s in SCENARIOS]


def b_system():
    return soft_system(False)[0]


def last_step(scn):
    return STEPS + (8 if scn["name"] == "reset" else 0)


def meta():
    with open(os.path.join(GOLDEN, "soft_runs.json")) as fh:
        return json.load(fh)


def fixture(name):
    with np.load(os.path.join(GOLDEN, "soft_%s.npz" % name)) as z:
        return {k: z[k] for k in z.files}


def b_conditions(fx, scn):
    """'' when a recorded run holds what it is for: the soft term did work (epair rose from its start and moved the beads),
    the rows are those of every fourth step, nothing blew up."""
    rows = fx["thermo"]
    want = list(range(0, STEPS + 1, THERMO_EVERY)) + ([STEPS] + list(range(STEPS + THERMO_EVERY, STEPS + 9, THERMO_EVERY)) if scn["name"] == "reset" else [])
    if [int(r[0]) for r in rows] != want:
        return "thermo rows at %r" % [int(r[0]) for r in rows]
    if not np.isfinite(rows).all() or not np.isfinite(fx["x"]).all():
        return "a non-finite value"
    if not np.abs(rows[:, 2]).max() > 0:
        return "epair is zero in every row"
    return ""


# ------------------------------------------------------------------------------------------------------------------
# (c): the push-off
# ------------------------------------------------------------------------------------------------------------------
PUSH_N, PUSH_DENSITY, PUSH_SEED = 2000, 0.85, 5
PUSH_CLOSEST_REFERENCE = 0.85      # the generator lengthens the ramp until the reference's closest pair is at least this
PUSH_CLOSEST = 0.8                 # ... and the engine must reach this: at A = 60, kT = 1 a pair at 0.8 costs 23 kT


def push_system():
    from lammps_le_amd.synth import phantom_chains
    s = phantom_chains(PUSH_N, 1, PUSH_DENSITY, seed=PUSH_SEED)
    s["nbondtypes"] = 2
    return s


PUSH_HEAD = """units lj
atom_style bond
newton off
atom_modify sort 0 0
special_bonds fene
read_data data.chain
neighbor 0.4 bin
neigh_modify every 1 delay 0 check yes
comm_modify cutoff 5.0
bond_style fene
bond_coeff 1 30.0 1.5 1.0 1.0
bond_coeff 2 30.0 4.0 1.0 1.0
timestep 0.005
fix 1 all nve
fix 2 all langevin 1.0 1.0 1.0 904297
thermo 100
"""


def push_stage1(steps):
    return (PUSH_HEAD + "pair_style soft 1.12246\npair_coeff * * 0.0\nvariable A equal ramp(0,60)\n"
            "fix push all adapt 1 pair soft a * * v_A\nrun %d\nunfix push\n" % steps)


PUSH_STAGE2 = "pair_style lj/cut 1.12246\npair_modify shift yes\npair_coeff * * 1.0 1.0 1.12246\nrun 200\n"
PUSH_CONTROL = PUSH_HEAD + "pair_style lj/cut 1.12246\npair_modify shift yes\npair_coeff * * 1.0 1.0 1.12246\nrun 0\n"


def closest_nonbonded(x, box, bonds):
    """Smallest minimum-image distance between two beads that share no bond"""
    from scipy.spatial import cKDTree
    box = np.asarray(box, dtype=np.float64)
    prd = box[:, 1] - box[:, 0]
    y = np.mod(np.asarray(x) - box[:, 0], prd)
    y = np.where(y >= prd, 0.0, y)
    t = cKDTree(y, boxsize=prd)
    pairs = t.query_pairs(1.2, output_type="ndarray")
    bonded = set((min(a, b) - 1, max(a, b) - 1) for _, a, b in np.asarray(bonds))
    keep = np.array([(int(i), int(j)) not in bonded for i, j in pairs], dtype=bool)
    pairs = pairs[keep]
    if not len(pairs):
        return 1.2
    d = y[pairs[:, 0]] - y[pairs[:, 1]]
    d -= prd * np.round(d / prd)
    return float(np.sqrt((d * d).sum(axis=1)).min())
