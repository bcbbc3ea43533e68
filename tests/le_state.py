"""The state the three LE fixes leave behind, checked against references that know nothing of the fixes (no GPU here).

fix extrusion, fix ex_load and fix ex_unload decide which bonds move, appear and go; those decisions are held against the CPU
oracle elsewhere (test_gpu_le.py).  Everything that FOLLOWS from the bond set they leave is derivable from that set alone:
the special lists (breadth-first search, neigh_reference.reference_specials), the angle tables under `ex_load ... atype`
(a rule over the bonds), and the forces, energies and pressure (force_reference.System built from the gathered topology).
This module has the accessor that reads an end state from either side (engine handle, oracle object), the invariants of
that state, the reference built from it, and the small seeded inputs on which a wrong table changes a force.

Run lengths: every fix of the inputs has the period 10 and fires on the steps with step % 10 = 1 (extrusion), 2 (ex_unload)
and 3 (ex_load).  120 ends on a step where nothing fires, 121 on an extrusion step, 123 on a loading step (the force of a
firing step already sees the new tables: the fixes ask for a reneighbor on the step they fire).  The chains start on a
lattice, where no bead is within the loading distance of its second neighbor along the chain: the first extruder loads at
step 33, and each fix has fired with a nonzero count at least five times by step 120 (asserted in
test_le_state_cpu.py); much later an extruder bond or a stale angle's leg outgrows half the 9.5 box, which the reference's
minimum image cannot follow (it asserts that none does).

Force metric of an end state: max |f - f_ref| over max |f_ref| (the largest force component, 150 - 300 here), not the per-component
metric of force_compare.relerr.  On a thermalised state in a 9.5 box the FP64 oracle is 1e-13 to 4e-13 from the reference on
components of ANY size (up to 9.5e-13 on the inputs here; the engine, which rounds the same way, up to 8.7e-13): it rounds x_i - x_j of a pair across a face to an ulp of
the box edge (1.8e-15) before it subtracts the edge, and a contact has a stiffness of ~1e3.  Sixteen times that is above
the project's 1e-12 for one evaluation on every such state, whatever the seed, so force_compare.bound would call every such
input wrong; relative to the force scale the same errors are 2.5e-15 to 6.2e-15, and the bound is 1e-13 of that scale."""
import collections
import functools

import numpy as np

import force_compare as fc
import force_reference as fr
import neigh_reference as R
from systems import CHAIN_SCRIPT, lattice_chain, run_oracle, wrap_into_box

KEYWORDS = ("evdwl", "ebond", "eangle", "pe", "press", "pxx", "pyy", "pzz", "pxy", "pxz", "pyz")
EXTRUDER = 2                                   # the bond type of every extruder bond in the inputs
PTENSOR = "thermo_style custom step temp epair emol etotal press pxx pyy pzz pxy pxz pyz\n"

State = collections.namedtuple("State", "x image v f types num_bond bond_type bond_atom nspecial special num_angle angle_type "
                                        "angle_atom1 angle_atom2 angle_atom3 thermo")


# ------------------------------------------------------------------------------------------------
# the accessor
# ------------------------------------------------------------------------------------------------
def engine_state(lmp):
    """End state of an engine handle (every call is a gather or a keyword: collective on a decomposed run)."""
    g = lmp.gather
    two = lambda a: np.asarray(a).reshape(lmp.get_natoms(), -1)
    ang = [None] * 5
    if lmp.extract_setting("angle_per_atom") > 0:
        ang = [g("num_angle")] + [two(g(k)) for k in ("angle_type", "angle_atom1", "angle_atom2", "angle_atom3")]
    thermo = {k: lmp.get_thermo(k) for k in KEYWORDS + ("bonds", "angles")}
    return State(g("x"), g("image"), g("v"), g("f"), g("type"), g("num_bond"), two(g("bond_type")), two(g("bond_atom")),
                 g("nspecial"), two(g("special")), *ang, thermo)


def oracle_state(o, system):
    """End state of an oracle object; the keywords as the engine's thermo prints them (lj units: per bead)."""
    n = o.n
    box = np.asarray(system["box"], dtype=np.float64)
    vol = float(np.prod(box[:, 1] - box[:, 0]))
    t, v, eangle = o.thermo(), o.v(), o.angle_energy()
    m = np.asarray(system["mass"])[o.types() - 1]
    k6 = [(m * v[:, a] * v[:, b]).sum() for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))]
    thermo = dict(evdwl=t[6] / n, ebond=t[7] / n, eangle=eangle / n, pe=(t[6] + t[7] + eangle) / n, press=t[4], bonds=float(o.nbonds()),
                  angles=float(o.nangles()))
    thermo.update({k: (k6[c] + t[8 + c]) / vol for c, k in enumerate(KEYWORDS[5:])})
    ang = list(o.angle_table()) if system.get("nangletypes") else [None] * 5
    ns, sp = o.special_table()
    return State(o.x(), o.image(), v, o.f(), o.types(), *o.bond_table(), ns, sp, *ang, thermo)


def state_of(handle, system=None):
    from oracle import Oracle
    return oracle_state(handle, system) if isinstance(handle, Oracle) else engine_state(handle)


# ------------------------------------------------------------------------------------------------
# invariants of a state
# ------------------------------------------------------------------------------------------------
def check_bonds(st, extruder=EXTRUDER):
    """The per-atom bond tables: within their width, every bond on both ends with one type, at most one extruder bond per
    bead, the keyword `bonds` their count.  Returns the bonds as a sorted list of (type, a, b), a < b, one row per bond."""
    n, bpa = st.bond_atom.shape
    assert (st.num_bond >= 0).all() and (st.num_bond <= bpa).all(), "num_bond exceeds bond_per_atom"
    stored = collections.Counter()
    for i in np.nonzero(st.num_bond)[0]:
        for m in range(st.num_bond[i]):
            t, j = int(st.bond_type[i, m]), int(st.bond_atom[i, m])
            assert 1 <= j <= n and j != i + 1 and t >= 1, "bead %d stores bond (%d, %d)" % (i + 1, t, j)
            stored[(int(i) + 1, t, j)] += 1
    for (a, t, b), c in stored.items():
        assert stored[(b, t, a)] == c, "bond %d-%d of type %d: %d on %d, %d on %d" % (a, b, t, c, a, stored[(b, t, a)], b)
    per_bead = collections.Counter(a for (a, t, b), c in stored.items() for _ in range(c) if t == extruder)
    assert not per_bead or max(per_bead.values()) == 1, "a bead carries more than one extruder bond: %s" % per_bead.most_common(3)
    bonds = sorted((t, a, b) for (a, t, b), c in stored.items() if a < b for _ in range(c))
    assert 2 * len(bonds) == sum(stored.values()) and st.thermo["bonds"] == len(bonds), (len(bonds), st.thermo["bonds"])
    return bonds


def special_blocks(st):
    """Per bead (row) the three blocks of its special list, as lists."""
    return [[st.special[i, lo:hi].tolist() for lo, hi in ((0, a), (a, b), (b, c))] for i, (a, b, c) in enumerate(st.nspecial.tolist())]


def check_specials(st, bonds, weights):
    """The special lists against the breadth-first search over `bonds`.  weights = the three lj weights of special_bonds.  Where
    no weight is 1 every block has to be the search's level, as a set and in size (no duplicate survived dedup).  Where the
    1-3 or 1-4 weight is 1 the reference program trims those blocks of the beads whose lists it rebuilds from scratch and
    keeps what the incremental edits left on the others: the 1-2 block is compared in full, every 1-3 / 1-4 entry
    must be a partner of that level."""
    n = len(st.nspecial)
    want = R.reference_specials(n, bonds)
    full = all(w != 1.0 for w in weights)
    assert st.nspecial.shape == (n, 3) and (np.diff(st.nspecial, axis=1) >= 0).all() and (st.nspecial[:, 0] >= 0).all()
    assert (st.nspecial[:, 2] <= st.special.shape[1]).all(), "nspecial exceeds maxspecial"
    bad = []
    for i, blocks in enumerate(special_blocks(st)):
        levels = want.get(i + 1, {})
        for lv, got in enumerate(blocks, start=1):
            expect = sorted(p for p, l in levels.items() if l == lv)
            if lv == 1 or full:
                if sorted(got) != expect:
                    bad.append("bead %d level %d: stored %s, search %s" % (i + 1, lv, sorted(got), expect))
            elif not set(got) <= set(expect) or len(set(got)) != len(got):
                bad.append("bead %d level %d: stored %s is no subset of the search's %s" % (i + 1, lv, sorted(got), expect))
    assert not bad, "%d special blocks differ:\n%s" % (len(bad), "\n".join(bad[:12]))


def check_angles(st):
    """The per-atom angle tables as a multiset {(type, a1, a2, a3): copies} with a1 < a3 (the fixes store an angle they create
    from its other end on the third atom: the ends carry no order): every angle on each of its three atoms equally often, the
    keyword `angles` = copies / 3.  No angle tables: an empty multiset."""
    if st.num_angle is None:
        assert st.thermo["angles"] == 0
        return collections.Counter()
    n, apa = st.angle_type.shape
    assert (st.num_angle >= 0).all() and (st.num_angle <= apa).all(), "num_angle exceeds angle_per_atom"
    on = collections.Counter()
    for i in np.nonzero(st.num_angle)[0]:
        for m in range(st.num_angle[i]):
            a1, a3 = int(st.angle_atom1[i, m]), int(st.angle_atom3[i, m])
            key = (int(st.angle_type[i, m]), min(a1, a3), int(st.angle_atom2[i, m]), max(a1, a3))
            assert len(set(key[1:])) == 3 and min(key[1:]) >= 1 and max(key[1:]) <= n, "bead %d stores angle %s" % (i + 1, key)
            assert int(i) + 1 in key[1:], "bead %d stores angle %s it is no part of" % (i + 1, key)
            on[(int(i) + 1, key)] += 1
    angles = collections.Counter()
    for (i, key), c in on.items():
        for a in key[1:]:
            assert on[(a, key)] == c, "angle %s: %d copies on bead %d, %d on bead %d" % (key, c, i, on[(a, key)], a)
        if i == key[2]:
            angles[key] = c
    assert 3 * sum(angles.values()) == sum(on.values()) and st.thermo["angles"] == sum(angles.values()), (sum(angles.values()), st.thermo["angles"])
    return angles


def unoriented(angles):
    """An angle multiset with the ends of every angle ordered (a1 < a3)."""
    out = collections.Counter()
    for (t, a, b, c), k in angles.items():
        out[(t, min(a, c), b, max(a, c))] += k
    return out


def angle_rule(system, bonds, atype, extruder=EXTRUDER):
    """What `ex_load ... atype T` and ex_unload leave while no extruder moves: the data file's angles plus, at every bead, one
    angle of type T for every pair of its bonds of which exactly one is an extruder bond - the bead as the vertex."""
    out = unoriented(collections.Counter(tuple(int(v) for v in row) for row in np.asarray(system["angles"]).tolist()))
    ext, other = collections.defaultdict(list), collections.defaultdict(list)
    for t, a, b in bonds:
        for p, q in ((a, b), (b, a)):
            (ext if t == extruder else other)[p].append(q)
    for v, partners in ext.items():
        for p in partners:
            for q in other[v]:
                out[(atype, min(p, q), v, max(p, q))] += 1
    return out


def check_state(st, weights, extruder=EXTRUDER):
    """Every invariant; returns (bonds, angle multiset)."""
    bonds = check_bonds(st, extruder)
    check_specials(st, bonds, weights)
    return bonds, check_angles(st)


# ------------------------------------------------------------------------------------------------
# the reference of a gathered topology
# ------------------------------------------------------------------------------------------------
def reference_for(script, system, bonds, angles=None, types=None, special_from=None):
    """force_reference.System of the script's force field on a gathered topology (bonds: rows (type, a, b); angles: a multiset,
    a duplicate is evaluated twice)."""
    model = fr.model_from_script(script, system["ntypes"])
    return fr.System(model, system["box"], system["type"] if types is None else types, system["mass"], bonds,
                     angles if angles is not None and len(angles) else None, special_from)


def reference_keywords(S, ev, v):
    t = S.thermo(ev, v)
    return {k: t[k] for k in KEYWORDS}


def force_error(f, ref):
    """max |f - ref| / max(max |ref|, 1), in long double (the module docstring says why not per component)."""
    f, ref = fr.ld(f), fr.ld(ref)
    return float(np.abs(f - ref).max() / max(np.abs(ref).max(), 1))


def deviations(S, ev, st):
    """{f, keyword: relative deviation of a state's forces and thermo keywords from a reference evaluation}; f_each: the
    per-component figure, for the record."""
    ref = reference_keywords(S, ev, st.v)
    dev = {"f": force_error(st.f, ev.f), "f_each": fc.relerr(st.f, ev.f)}
    dev.update({k: fc.relerr(st.thermo[k], ref[k]) for k in KEYWORDS})
    return dev


def changed_level_pairs(system, x, cut, bonds):
    """Pairs within `cut` at the positions x whose special level under `bonds` is not the one the data file's bonds give."""
    n = len(x)
    now, then = R.reference_specials(n, bonds), R.reference_specials(n, system["bonds"])
    iu, ju = np.triu_indices(n, 1)
    near = R.sep2_ld(x[iu], x[ju], system["box"]) < R.LD(cut) ** 2
    return sum(1 for i, j in zip(iu[near].tolist(), ju[near].tolist())
               if now.get(i + 1, {}).get(j + 1, 0) != then.get(i + 1, {}).get(j + 1, 0))


# ------------------------------------------------------------------------------------------------
# inputs: 600 beads in 2 chains (not a multiple of 64; a 9.5 box), fix nve on the data file's velocities, no thermostat
# ------------------------------------------------------------------------------------------------
LENGTHS = (120, 121, 123)
PHASE = {"loop": 1, "loading": 3, "unloading": 2}          # a fix fires on the steps with step % period == its phase
SOFT = CHAIN_SCRIPT.replace("bond_coeff 2 30.0 4.0 1.0 1.0", "bond_coeff 2 5.0 10.0 1.0 1.0")
# every 1-3 and 1-4 partner within the pair cutoff, the weights fractional, no shift: a wrong level is a wrong force
LEVELS = SOFT.replace("special_bonds fene", "special_bonds lj 0.0 0.3 0.7").replace("pair_style lj/cut 1.12", "pair_style lj/cut 2.5") \
    .replace("pair_modify shift yes", "pair_modify shift no").replace("pair_coeff * * 1.0 1.0 1.12", "pair_coeff * * 1.0 1.0 2.5")
ANGLES = SOFT.replace("atom_style bond", "atom_style molecular") + "angle_style harmonic\nangle_coeff 1 1.5 150.0\nangle_coeff 2 1.0 100.0\n"
assert SOFT != CHAIN_SCRIPT and LEVELS.count("2.5") == 2 and "shift no" in LEVELS and "lj 0.0 0.3 0.7" in LEVELS and "molecular" in ANGLES
FIXES = """fix 1 all nve
fix loop all extrusion {ne} 1 {left} {right} {tp} 2 {lr}
fix loading all ex_load {nl} 1 1 1.12 2 prob 0.5 684474 iparam 1 1 jparam 1 1{atype}
fix unloading all ex_unload {nu} 2 0.5 prob 0.3 456456
"""
FENE_W, LEVELS_W = (0.0, 1.0, 1.0), (0.0, 0.3, 0.7)
# `levels` for two z slabs: a ghost cutoff of 3.5 (above cutneigh 2.9 and every extruder bond of the run, asserted on the CPU)
# and the box stretched along z to four of them, the least two slabs may have (csrc/device.h slab_rule): the beads fill
# z < 9.5, both slabs own some
SLAB_GHOST, SLAB_LZ = 3.5, 14.2
LEVELS_SLAB = LEVELS.replace("comm_modify cutoff 5.0", "comm_modify cutoff %.1f" % SLAB_GHOST)
assert LEVELS_SLAB != LEVELS
# name: (head, weights, barriers, fix ids present, atype)
INPUTS = {
    "levels-slab": (LEVELS_SLAB, LEVELS_W, False, ("loop", "loading", "unloading"), 0),
    "wca-fene": (SOFT, FENE_W, False, ("loop", "loading", "unloading"), 0),
    "levels": (LEVELS, LEVELS_W, False, ("loop", "loading", "unloading"), 0),
    "barriers": (LEVELS, LEVELS_W, True, ("loop", "loading", "unloading"), 0),
    "angles-load": (ANGLES, FENE_W, False, ("loading", "unloading"), 2),
    "angles-all": (ANGLES, FENE_W, False, ("loop", "loading", "unloading"), 2),
}
NAMES = sorted(INPUTS)
SEED = 3


@functools.lru_cache(maxsize=None)
def system_of(name, relaxed=False):
    """relaxed: after RELAX steps of Langevin dynamics under the input's force field (oracle MD from the lattice start), so that
    beads are within the loading distance of their second neighbors from the first firing on."""
    if relaxed:
        s = dict(system_of(name))
        o = run_oracle(INPUTS[name][0] + "fix 1 all nve\nfix 2 all langevin 1.0 1.0 1.0 7774\nrun %d\n" % RELAX, s)
        s["x"], s["v"], s["image"] = o.x(), o.v(), o.image()
        return s
    head, weights, barriers, fids, atype = INPUTS[name]
    n = 600
    types = None
    if barriers:          # 15 % of the beads are barriers of the three kinds (left, right, roadblock)
        rng = np.random.RandomState(17)
        types = np.ones(n, dtype=np.int32)
        pick = rng.rand(n) < 0.15
        types[pick] = rng.randint(2, 5, size=pick.sum())
        types[0] = types[-1] = 1
    s = lattice_chain(n, nchains=2, seed=SEED, types=types)
    if head is LEVELS_SLAB:
        s["box"] = np.array([s["box"][0], s["box"][1], [0.0, SLAB_LZ]])
    if barriers:
        s["ntypes"], s["mass"] = 4, [1.0] * 4
    if atype:
        per = n // 2
        ang = [(1, i, i + 1, i + 2) for i in range(1, n - 1) if (i - 1) // per == (i + 1) // per]
        s.update(nangletypes=2, angles=np.array(ang, dtype=np.int32), extra_angle=24, atom_style="molecular")
    return s


def script_of(name, steps, periods=(10, 10, 10), thermo=10, ptensor=True):
    head, weights, barriers, fids, atype = INPUTS[name]
    fixes = FIXES.format(ne=periods[0], nl=periods[1], nu=periods[2], left=2 if barriers else 1, right=3 if barriers else 1,
                         tp=0.5 if barriers else 1.0, lr="4" if barriers else "", atype=" atype %d" % atype if atype else "")
    if "loop" not in fids:
        fixes = "".join(ln + "\n" for ln in fixes.split("\n") if ln and not ln.startswith("fix loop"))
    return head + fixes + (PTENSOR if ptensor else "") + "thermo %d\nrun %d\n" % (thermo, steps)


def cutoff_of(name):
    return 2.5 if INPUTS[name][0] in (LEVELS, LEVELS_SLAB) else 1.12


@functools.lru_cache(maxsize=None)
def oracle_end(name, steps, periods=(10, 10, 10), thermo=10):
    """(oracle object, its end state) of an input after `steps` steps (the trajectory periods: from the relaxed start)."""
    s = system_of(name, periods == PERIODS)
    o = run_oracle(script_of(name, steps, periods, thermo), s)
    return o, oracle_state(o, s)


@functools.lru_cache(maxsize=None)
def oracle_events(name, steps):
    """{fix id: [count of every firing]} from fresh oracle runs that end on each firing step, and the unloads in total."""
    fired = {fid: [int(oracle_end(name, t)[0].fix_vector(fid)[0]) for t in range(PHASE[fid], steps + 1, 10)] for fid in INPUTS[name][3]}
    return fired, int(oracle_end(name, steps)[0].fix_vector("unloading")[1])


@functools.lru_cache(maxsize=None)
def oracle_reference(name, steps):
    """(reference system of the oracle's end topology, its evaluation at the oracle's end positions, the oracle's deviations
    from it): what the bound of the GPU test is 16 x of."""
    s = system_of(name)
    o, st = oracle_end(name, steps)
    bonds, angles = check_state(st, INPUTS[name][1])
    S = reference_for(script_of(name, steps), s, bonds, angles, st.types)
    ev = S.evaluate(st.x)
    return S, ev, deviations(S, ev, st)


# ------------------------------------------------------------------------------------------------
# a trajectory through firings: K steps with periods 4 / 5 / 6, the topology of every step from fresh oracle runs
# ------------------------------------------------------------------------------------------------
K, PERIODS, TRAJ_THERMO, RELAX = 24, (4, 5, 6), 8, 1500


def traj_script(name, steps=K):
    return script_of(name, steps, PERIODS, TRAJ_THERMO, ptensor=False)


@functools.lru_cache(maxsize=None)
def schedule(name):
    """[(bonds, angle multiset) the oracle holds after k steps, k = 0 .. K]: integer data, from a fresh run per k."""
    out = []
    for k in range(K + 1):
        st = oracle_end(name, k, PERIODS, TRAJ_THERMO)[1]
        out.append(check_state(st, INPUTS[name][1]))
    return out


@functools.lru_cache(maxsize=None)
def reference_trajectory(name):
    s = system_of(name, True)
    sched = schedule(name)
    S = reference_for(traj_script(name), s, *sched[0])
    x, img = wrap_into_box(s)
    return S, S.trajectory(x, s["v"], img, K, topology=lambda step: sched[step])


@functools.lru_cache(maxsize=None)
def oracle_trajectory(name):
    """Deviations of the oracle from the reference trajectory: after the last step (x, v, f, rows) and after each step 1 .. K-1
    (x, v), as force_compare.oracle_trajectory / oracle_states give them for the static inputs."""
    S, ref = reference_trajectory(name)
    o, st = oracle_end(name, K, PERIODS, TRAJ_THERMO)
    h = o.thermo_history()
    steps = list(range(0, K + 1, TRAJ_THERMO))
    assert [int(r[0]) for r in h] == steps
    last = dict(x=fc.relerr(S.unwrapped(st.x, st.image), ref["x"][-1]), v=fc.relerr(st.v, ref["v"][-1]), f=fc.relerr(st.f, ref["f"]),
                rows=max(fc.relerr(h[q, 1 + c], ref["rows"][k][key]) for q, k in enumerate(steps) for c, key in enumerate(fc.ROW_KEYS)))
    states = []
    for k in range(1, K):
        sk = oracle_end(name, k, PERIODS, TRAJ_THERMO)[1]
        states.append(dict(x=fc.relerr(S.unwrapped(sk.x, sk.image), ref["x"][k]), v=fc.relerr(sk.v, ref["v"][k])))
    return last, states, int(o.neigh_builds())


def traj_required_gap(name):
    """force_compare.required_gap's rule for these trajectories."""
    pos_bound = fc.bound(oracle_trajectory(name)[0]["x"], fc.TRAJ_CEILING["x"])
    return 100.0 * 4.0 * np.sqrt(3.0) * cutoff_of(name) * pos_bound
