"""Expected rows of the local pair computes (compute property/local natom* / patom*, compute pair/local), without any of
the engine's machinery: every candidate pair comes from `neigh_reference.reference_pairs` (long double, all N^2 candidates,
minimum image), the exclusions from `reference_specials` / `expected_code`, cutoffs, energy and force from
`force_reference.pair_matrix` / `lj_terms`.

What a row is (compute_property_local.cpp count_pairs, compute_pair_local.cpp compute_pairs of the reference program at
one rank, restated): an unordered pair of the list, both beads in the compute's group, minus the special levels whose lj and
coul weights are both 0.
  NEIGH kind   every pair within cutneigh (the largest pair cutoff plus the skin) at the positions of the list build;
  PAIR kind    every such pair with rsq < cutsq[itype][jtype] at the CURRENT positions.  Between two rebuilds no bead has moved
               more than half the skin, so every pair inside its cutoff now was inside cutneigh at the build: the reference
               takes the pairs from the current positions alone and needs nothing of the list.
Orientation and order are the engine's: atom1 is the lower ID, rows are sorted by (atom1, atom2).

A pair is UNDECIDED when its squared separation lies within `neigh_reference.delta` of the cutoff that decides it.  The states
the GPU tests compare hold no such pair; test_pair_rows_cpu.py asserts that for every one of them without a GPU."""
import collections
import functools

import numpy as np

import force_compare as FC
import force_inputs as FI
import force_reference as FR
import neigh_inputs as NI
import neigh_reference as R
from neigh_reference import LD

Rows = collections.namedtuple("Rows", "ids vals undecided")      # ids [R, 4] atom1 atom2 type1 type2; vals [R, 6] long double
COLUMNS = ("dist", "eng", "force", "fx", "fy", "fz")
STEPS = 5          # `a few steps`: see states()
DD_STEPS = 4


# ------------------------------------------------------------------------------------------------
# inputs: name -> dict(system, head(skin) -> script up to the fixes, lj, coul, cutoffs)
# ------------------------------------------------------------------------------------------------
def _force_input(name):
    case = FI.INPUTS[name]()
    s = case["system"]
    model = FR.model_from_script(FI.script(case), s["ntypes"])
    coul = (0.0, 1.0, 1.0) if case.get("special", "fene") == "fene" else (0.0, 0.0, 0.0)
    return dict(system=s, head=lambda skin: FI.script(case, skin=skin), lj=model.special_lj, coul=coul,
                coeffs=FR.pair_matrix(model, s["ntypes"]), oracle_head=lambda skin: FI.script(case, skin=skin))


def _zero_matrix(ntypes, cut):
    z = np.zeros((ntypes + 1, ntypes + 1), dtype=LD)
    return z, z + 1, z + LD(cut), z


def _neigh_input(system, engine_script):
    """The chain scripts of the list tests: pair_style zero on the engine (rows by its cutoff, eng and force 0), lj/cut with
    epsilon 0 on the oracle (the same list)."""
    skinned = lambda text: (lambda skin: text.replace("neighbor 0.4 bin", "neighbor %s bin" % skin))
    return dict(system=system, head=skinned(engine_script), lj=(0.0, 1.0, 1.0), coul=(0.0, 1.0, 1.0),
                coeffs=_zero_matrix(system["ntypes"], 1.12), oracle_head=skinned(NI.EPS0_SCRIPT))


@functools.lru_cache(maxsize=None)
def thin_slabs():
    """A chain of 200 beads in a box 5.3 x 5.3 x 8.4: under `comm_modify cutoff 2.0` and a skin of 0.2 two slabs of 4.2 and
    three of 2.8, the thinnest the slab rule admits (two ghost cutoffs for two ranks, two pair shells of 1.32 for three)."""
    s = FI.lattice(5, 5, 8, seed=12)
    return dict(system=FI.hot(FI.displace(s), 4.0), force_field=FI.FENE + FI.WCA)


def _thin_input():
    case = thin_slabs()
    s = case["system"]
    model = FR.model_from_script(FI.script(case), s["ntypes"])
    return dict(system=s, head=lambda skin: FI.script(case, skin=skin), lj=model.special_lj, coul=(0.0, 1.0, 1.0),
                coeffs=FR.pair_matrix(model, s["ntypes"]), oracle_head=lambda skin: FI.script(case, skin=skin))


LE_FIXES = "fix 1 all nve\nfix loading all ex_load 10 1 1 1.12 2 prob 0.5 684474 iparam 1 1 jparam 1 1\n"
LE_STEPS = 6          # fix ex_load fires at step 3 (and forces a rebuild there); three more steps on that list


def _le_input():
    """The small loop-extrusion system of the LE tests (le_state.py: 600 beads in two chains, relaxed so that second neighbors
    are within the loading distance) with fix ex_load alone."""
    import le_state
    s = le_state.system_of("wca-fene", relaxed=True)
    model = FR.model_from_script(le_state.SOFT, s["ntypes"])
    head = lambda skin: le_state.SOFT.replace("neighbor 0.4 bin", "neighbor %s bin" % skin)
    return dict(system=s, head=head, lj=model.special_lj, coul=(0.0, 1.0, 1.0), coeffs=FR.pair_matrix(model, s["ntypes"]),
                oracle_head=head, fixes=LE_FIXES)


INPUTS = {
    "le_small": _le_input,
    "tiny": lambda: _force_input("tiny"), "types": lambda: _force_input("types"),
    "hubs-harmonic": lambda: _force_input("hubs-harmonic"), "offset": lambda: _force_input("offset"),
    "dense_cluster": lambda: _neigh_input(NI.dense_cluster(), NI.ZERO_SCRIPT),
    "slab_ladder": lambda: _neigh_input(NI.slab_ladder()[0], NI.ZERO_SCRIPT),
    "thin_slabs": _thin_input,
}
TABLE_INPUTS = ("tiny", "types", "hubs-harmonic", "offset", "dense_cluster", "slab_ladder")
FORCE_INPUTS = ("tiny", "types", "hubs-harmonic", "offset")      # the ones that move (check 2)
DD_INPUTS = {"slab_ladder": 0, "thin_slabs": DD_STEPS}          # name -> steps before the tables are compared (check 5)
NVE = "fix 1 all nve\n"


@functools.lru_cache(maxsize=None)
def get(name):
    return INPUTS[name]()


def cutneigh(name, skin):
    return float(get(name)["coeffs"][2].max()) + float(skin)


def run0_script(name, oracle=False):
    return get(name)["oracle_head" if oracle else "head"]("0.4") + "run 0\n"


def steps_script(name, steps, oracle=False, extra=""):
    """`steps` steps of fix nve under a skin of 0.2 (le_small: of its fixes under the chain script's 0.4), a thermo line at
    every step (the last one carries evdwl)."""
    inp = get(name)
    skin = "0.4" if "fixes" in inp else "0.2"
    return inp["oracle_head" if oracle else "head"](skin) + inp.get("fixes", NVE) + extra + "thermo 1\nrun %d\n" % steps


# ------------------------------------------------------------------------------------------------
# the rows
# ------------------------------------------------------------------------------------------------
def levels_of(n, bonds):
    return R.reference_specials(n, np.asarray(bonds).reshape(-1, 3))


def reference_rows(name, x, kind, skin="0.4", bonds=None, member=None):
    """Rows of `kind` ("neigh" | "pair") of input `name` at the positions x (by tag; for "neigh" the positions of the list
    build).  bonds: the bond table the special levels follow, if not the input's; member: boolean by tag - 1."""
    inp = get(name)
    s = inp["system"]
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = len(x)
    box = np.asarray(s["box"], dtype=np.float64)
    types = np.asarray(s["type"], dtype=np.int64)
    eps, sig, cut, off = inp["coeffs"]
    c = cutneigh(name, skin) if kind == "neigh" else float(cut.max())
    ref = R.reference_pairs(x, box, c)
    undecided = [u for u in R.undecided(ref) if u[0] < u[1]]
    keep = ref.i < ref.j
    i, j = ref.i[keep], ref.j[keep]
    sp = levels_of(n, s["bonds"] if bonds is None else bonds)
    level = np.array([sp.get(a + 1, {}).get(b + 1, 0) for a, b in zip(i.tolist(), j.tolist())], dtype=np.int64).reshape(-1)
    listed = np.array([R.expected_code(int(lv), inp["lj"], inp["coul"]) is not None for lv in level], dtype=bool).reshape(-1)
    if member is not None:
        member = np.asarray(member, dtype=bool)
        listed &= member[i] & member[j]
    i, j, level = i[listed], j[listed], level[listed]
    ti, tj = types[i], types[j]
    vals = np.zeros((len(i), 6), dtype=LD)
    if kind == "pair":
        prd = FR.ld(box[:, 1]) - FR.ld(box[:, 0])
        d = FR.min_image(FR.ld(x[i]) - FR.ld(x[j]), prd)
        rsq = (d * d).sum(axis=1)
        assert np.array_equal(rsq, R.sep2_ld(x[i], x[j], box))
        cutsq = cut[ti, tj] * cut[ti, tj]
        gap = np.abs(rsq - cutsq)
        dl = np.array([R.delta(box, float(cc)) for cc in cut[ti, tj]], dtype=LD).reshape(-1)
        undecided += [(int(a), int(b), float(g)) for a, b, g in zip(i[gap <= dl], j[gap <= dl], gap[gap <= dl])]
        inside = rsq < cutsq
        i, j, level, ti, tj, d, rsq = i[inside], j[inside], level[inside], ti[inside], tj[inside], d[inside], rsq[inside]
        w = FR.ld([1.0 if lv == 0 else inp["lj"][lv - 1] for lv in level.tolist()]).reshape(-1)
        fp, e = FR.lj_terms(rsq, eps[ti, tj], sig[ti, tj], off[ti, tj])
        fp, e = fp * w, e * w
        dist = np.sqrt(rsq)
        vals = np.stack([dist, e, dist * fp, d[:, 0] * fp, d[:, 1] * fp, d[:, 2] * fp], axis=1) if len(i) else np.zeros((0, 6), dtype=LD)
    ids = np.stack([i + 1, j + 1, ti, tj], axis=1) if len(i) else np.zeros((0, 4), dtype=np.int64)
    order = np.lexsort((ids[:, 1], ids[:, 0]))
    return Rows(ids[order], vals[order], undecided)


def columns(rows, names):
    """The columns `names` of reference rows as a long-double array [R, len(names)]."""
    idcol = {"natom1": 0, "natom2": 1, "ntype1": 2, "ntype2": 3, "patom1": 0, "patom2": 1, "ptype1": 2, "ptype2": 3}
    out = [FR.ld(rows.ids[:, idcol[k]]) if k in idcol else rows.vals[:, COLUMNS.index(k)] for k in names]
    return np.stack(out, axis=1)


# ------------------------------------------------------------------------------------------------
# the states the GPU tests compare, as the oracle reaches them (test_pair_rows_cpu.py: none holds an undecided pair)
# ------------------------------------------------------------------------------------------------
def states():
    """[(input, kind, skin, steps)]: `run 0` for the NEIGH rows of every input and the PAIR rows of the two that do not move;
    STEPS (DD_STEPS) steps for the PAIR rows of the others."""
    out = [(name, "neigh", "0.4", 0) for name in TABLE_INPUTS]
    out += [("dense_cluster", "pair", "0.4", 0), ("slab_ladder", "pair", "0.4", 0)]
    out += [(name, "pair", "0.2", STEPS) for name in FORCE_INPUTS]
    out += [("thin_slabs", "pair", "0.2", DD_STEPS), ("le_small", "pair", "0.4", LE_STEPS)]
    return out


@functools.lru_cache(maxsize=None)
def oracle_state(name, steps):
    """(positions by tag, list builds, bonds as rows (type, tag, tag)) of the oracle after `steps` steps (0: what read_data
    leaves)."""
    from systems import run_oracle, wrap_into_box
    s = get(name)["system"]
    if steps == 0:
        return wrap_into_box(s)[0], 1, np.asarray(s["bonds"]).reshape(-1, 3)
    o = run_oracle(steps_script(name, steps, oracle=True), s)
    return o.x(), int(o.neigh_builds()), np.array(sorted(o.bond_set()), dtype=np.int64).reshape(-1, 3)


def relerr(a, b):
    return FC.relerr(a, b, floor=1.0)


def nudge(name, x, by=0.15):
    """(tag, new position): the lower-ID bead of the PAIR row with the largest separation at the positions x, moved `by`
    straight away from its partner - less than half the skin of the run-0 scripts, so the list built at x still holds every
    pair inside its cutoff, and that row leaves the table."""
    rows = reference_rows(name, x, "pair")
    r = int(np.argmax(rows.vals[:, 0]))
    a, b = int(rows.ids[r, 0]), int(rows.ids[r, 1])
    box = np.asarray(get(name)["system"]["box"], dtype=np.float64)
    d = FR.min_image(FR.ld(x[a - 1]) - FR.ld(x[b - 1]), FR.ld(box[:, 1]) - FR.ld(box[:, 0]))
    u = np.asarray(d / np.sqrt((d * d).sum()), dtype=np.float64)
    return a, b, np.asarray(x[a - 1], dtype=np.float64) + by * u
