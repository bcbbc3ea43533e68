"""Without a GPU: the inputs of test_gpu_le_state.py are the inputs they claim to be, the checks of le_state.py hold on the CPU
oracle's end states and object to states that break them, and the oracle's own deviation from the long-double reference - the
figure every GPU bound is 16 x of - stays under the project's ceilings.

What the references are independent of: the special lists come from a breadth-first search over the end bonds, the angle set
of the runs without fix extrusion from a rule over the end bonds, forces and thermo from force_reference.System built from the
gathered tables alone.  What they do not cover: WHICH bonds the fixes move, create and break - that stays with the oracle."""
import collections

import numpy as np
import pytest

import force_compare as fc
import le_state as ls
import neigh_reference as R
from systems import wrap_into_box

CASES = [(name, steps) for name in ls.NAMES for steps in ls.LENGTHS]


@pytest.mark.parametrize("name,steps", CASES)
def test_end_state(name, steps):
    """The conditions on an input (every fix fired with a nonzero count at least three times, at least 8 extruders at the end,
    an unload, no FENE warning, every bond and angle leg below half the box - asserted inside the evaluation -, no pair the
    cutoff test could judge either way), every invariant of le_state on the oracle's end state, and the oracle's forces and
    thermo keywords against the reference of its own gathered topology.
    Figures of the 15 cases: 12 - 34 extruder bonds, 18 - 52 unloads, 5 - 9 nonzero firings per fix; forces 2.5e-15 to 6.2e-15 of the
    largest force component (1.3e-13 to 9.5e-13 per component, see le_state), keywords at most 4.4e-15; the smallest
    |r^2 - cut^2| 3.2e-05."""
    head, weights, barriers, fids, atype = ls.INPUTS[name]
    s = ls.system_of(name)
    assert len(s["x"]) % 64 and 500 <= len(s["x"]) <= 700
    o, st = ls.oracle_end(name, steps)
    fired, unloads = ls.oracle_events(name, steps)
    for fid in fids:
        assert sum(1 for c in fired[fid] if c > 0) >= 3, (fid, fired[fid])
    bonds, angles = ls.check_state(st, weights)
    extruders = [b for b in bonds if b[0] == ls.EXTRUDER]
    assert len(extruders) >= 8 and unloads >= 1 and o.fene_warnings() == 0
    S, ev, dev = ls.oracle_reference(name, steps)
    assert ev.fene_clamped == [] and float(ev.gap) > R.delta(S.box, S.cutmax)
    print("%s %d: extruders %d, unloads %d, firings %s, min |r^2 - cut^2| %.2e, longest bond or leg %.2f of half the box" %
          (name, steps, len(extruders), unloads, {k: sum(1 for c in v if c) for k, v in fired.items()}, float(ev.gap), ev.max_bond_frac))
    for k in ("f",) + ls.KEYWORDS:
        print("  oracle %-6s %.2e -> GPU bound %.2e" % (k, dev[k], fc.bound(dev[k], fc.RUN0_CEILING)))          # (asserts the ceiling)
    print("  oracle f per component %.2e" % dev["f_each"])
    if atype:
        assert any(t == atype for t, _, _, _ in angles) and abs(st.thermo["eangle"]) > 0.1
        if "loop" not in fids:          # no extruder ever moved: the angle set is a function of the bonds, without duplicates
            assert angles == ls.angle_rule(s, bonds, atype) and max(angles.values()) == 1
    else:
        assert not angles
    if name == "levels-slab":          # two slabs are allowed, and every bond partner is inside the ghost shell
        from test_dd_slab_rule_cpu import OK, _rule
        assert _rule()(ls.SLAB_LZ, 2, ls.cutoff_of(name) + 0.4, ls.SLAB_GHOST) == (OK, "")
        assert _rule()(ls.SLAB_LZ - 0.3, 2, ls.cutoff_of(name) + 0.4, ls.SLAB_GHOST)[0] != OK
        assert ev.max_bond_frac * float(S.prd.min()) / 2 < ls.SLAB_GHOST - 0.4
        z = st.x[:, 2]
        assert min((z < ls.SLAB_LZ / 2).sum(), (z >= ls.SLAB_LZ / 2).sum()) > 50


def test_levels_changed_where_a_force_feels_it():
    """On `levels` (and `barriers`) a pair whose special level the fixes changed carries another weight: at the end state at
    least 20 pairs within the cutoff have a level the data file's topology does not give them.  Counted: levels 245 / 303 / 251 pairs
    after 120 / 121 / 123 steps, barriers 155 / 194 / 170."""
    for name in ("levels", "barriers", "levels-slab"):
        for steps in ls.LENGTHS:
            st = ls.oracle_end(name, steps)[1]
            count = ls.changed_level_pairs(ls.system_of(name), st.x, ls.cutoff_of(name), ls.check_bonds(st))
            print(name, steps, "pairs with a changed level:", count)
            assert count >= 20


def test_fene_weights_trim_the_outer_blocks():
    """Under `special_bonds fene` the 1-3 and 1-4 blocks are only ever a subset of the search's levels: beads no fix touched
    hold their 1-2 partners alone (the reference program trims the outer levels when their weights are 1, special.cpp
    Special::trim), beads whose lists were rebuilt hold more.  Both kinds exist at the end of `wca-fene`."""
    st = ls.oracle_end("wca-fene", ls.LENGTHS[0])[1]
    bonds = ls.check_bonds(st)
    ls.check_specials(st, bonds, ls.FENE_W)
    want = R.reference_specials(len(st.x), bonds)
    blocks = ls.special_blocks(st)
    trimmed = sum(1 for i, b in enumerate(blocks) if not b[1] and any(l == 2 for l in want[i + 1].values()))
    kept = sum(1 for b in blocks if b[1] or b[2])
    print("beads with a trimmed 1-3 block %d, with outer entries %d" % (trimmed, kept))
    assert trimmed > 100 and kept > 20


@pytest.mark.parametrize("name", ls.NAMES)
def test_a_stale_topology_shows(name):
    """The checks have teeth: the same reference built from the data file's bonds (and angles) misses the oracle's forces by more
    than 1e-3 of the largest force on every input; on `levels` so does a reference with the end bonds whose special levels
    are still the data file's.  Measured: 0.035 (angles-load) to 0.47 (levels) of the largest force for the stale bonds, 0.53 for the stale levels."""
    steps = ls.LENGTHS[1]
    s = ls.system_of(name)
    st = ls.oracle_end(name, steps)[1]
    bonds, angles = ls.check_state(st, ls.INPUTS[name][1])
    stale = ls.reference_for(ls.script_of(name, steps), s, s["bonds"], s.get("angles"), st.types)
    miss = ls.force_error(st.f, stale.evaluate(st.x).f)
    print("%s: forces of the data file's topology miss by %.3e" % (name, miss))
    assert miss > 1e-3
    if name == "levels":
        stale = ls.reference_for(ls.script_of(name, steps), s, bonds, angles, st.types, special_from=s["bonds"])
        miss = ls.force_error(st.f, stale.evaluate(st.x).f)
        print("levels: forces under the data file's special levels miss by %.3e" % miss)
        assert miss > 1e-3
    if angles and "loop" in ls.INPUTS[name][3]:          # stale and duplicate copies count: as a set the angles miss
        as_set = ls.reference_for(ls.script_of(name, steps), s, bonds, collections.Counter(dict.fromkeys(angles, 1)), st.types)
        if max(angles.values()) > 1:
            assert ls.force_error(st.f, as_set.evaluate(st.x).f) > 1e-3


@pytest.mark.parametrize("name", ["levels", "angles-all"])
def test_trajectory_through_firings(name):
    """24 steps from a relaxed start with periods 4 / 5 / 6: the reference trajectory whose topology follows the oracle's
    step by step (integer data from fresh oracle runs of 1 .. 24 steps), and the oracle's deviation from it under the
    project's ceilings for short trajectories.  The tables change on 11 of the 24 steps.
    Measured (levels / angles-all): x 4.0e-15 / 4.3e-15, v 1.1e-13 / 1.1e-13, f 2.9e-12 / 4.8e-12, thermo rows 5.7e-15 / 6.7e-15;
    after the steps 1 .. 23 x at most 5.0e-15, v 1.4e-13; min |r^2 - cut^2| 7.9e-06 / 2.7e-05 (required 1.7e-10 / 7.8e-11); 54 and 12
    extruder bonds at the end."""
    sched = ls.schedule(name)
    changes = [k for k in range(1, ls.K + 1) if sched[k] != sched[k - 1]]
    print(name, "topology changes on steps", changes)
    assert len(changes) >= 8 and sum(1 for b in sched[-1][0] if b[0] == ls.EXTRUDER) >= 8
    for fid in ls.INPUTS[name][3]:          # every fix fired with a nonzero count on at least three of its steps
        period = ls.PERIODS[("loop", "loading", "unloading").index(fid)]
        counts = [int(ls.oracle_end(name, t, ls.PERIODS, ls.TRAJ_THERMO)[0].fix_vector(fid)[0]) for t in range(ls.PHASE[fid], ls.K + 1, period)]
        assert sum(1 for c in counts if c > 0) >= 3, (fid, counts)
    S, ref = ls.reference_trajectory(name)
    last, states, builds = ls.oracle_trajectory(name)
    print(name, last, "builds", builds, "states x %.2e v %.2e" % (max(d["x"] for d in states), max(d["v"] for d in states)))
    for k in ("x", "v", "f", "rows"):
        fc.bound(last[k], fc.TRAJ_CEILING[k])
    for d in states:
        fc.bound(d["x"], fc.TRAJ_CEILING["x"]), fc.bound(d["v"], fc.TRAJ_CEILING["v"])
    print("min gap %.3e, required %.3e" % (float(min(ref["gaps"])), ls.traj_required_gap(name)))
    assert float(min(ref["gaps"])) > ls.traj_required_gap(name)
    assert o_fene(name) == 0 and builds >= len(changes)          # (a firing that changes a table asks for a list build)


def o_fene(name):
    return ls.oracle_end(name, ls.K, ls.PERIODS, ls.TRAJ_THERMO)[0].fene_warnings()


def test_a_changing_topology_is_not_the_static_one():
    """The callback matters: the trajectory of `levels` under the data file's topology throughout is another trajectory, and a
    callback that always answers the same is the static behaviour, bit for bit."""
    name = "angles-all"
    s = ls.system_of(name, True)
    S = ls.reference_for(ls.traj_script(name), s, s["bonds"], collections.Counter(tuple(r) for r in s["angles"].tolist()))
    x, img = wrap_into_box(s)
    static = S.trajectory(x, s["v"], img, 6)
    same = S.trajectory(x, s["v"], img, 6, topology=lambda step: (s["bonds"], s["angles"]))
    assert all(np.array_equal(a, b) for a, b in zip(static["x"], same["x"])) and np.array_equal(static["f"], same["f"])
    moving = ls.reference_trajectory(name)[1]
    assert np.array_equal(static["x"][2], moving["x"][2])          # nothing fired yet
    assert fc.relerr(static["x"][6], moving["x"][6]) > 1e-7          # the loads of step 3 and the moves of step 5 are felt


# ------------------------------------------------------------------------------------------------
# the helpers object to broken states
# ------------------------------------------------------------------------------------------------
def broken(st, **arrays):
    return st._replace(**{k: v for k, v in arrays.items()})


def test_the_helpers_object_to_broken_states():
    st = ls.oracle_end("levels", ls.LENGTHS[0])[1]
    ls.check_state(st, ls.LEVELS_W)
    bonds = ls.check_bonds(st)
    want = R.reference_specials(len(st.x), bonds)
    # an extra 1-3 entry: a bead with room in its list gets a bead that is no partner of any level
    i = next(i for i in range(len(st.x)) if st.nspecial[i, 2] < st.special.shape[1] and st.nspecial[i, 1] > st.nspecial[i, 0])
    stranger = next(t for t in range(1, len(st.x) + 1) if t != i + 1 and t not in want[i + 1])
    ns, sp = st.nspecial.copy(), st.special.copy()
    a, b, c = ns[i]
    sp[i, b + 1:c + 1] = sp[i, b:c].copy()
    sp[i, b] = stranger
    ns[i] = (a, b + 1, c + 1)
    with pytest.raises(AssertionError, match="level 2"):
        ls.check_specials(broken(st, nspecial=ns, special=sp), bonds, ls.LEVELS_W)
    # ... a duplicate of an entry that is there (same set, another size)
    sp2 = st.special.copy()
    sp2[i, b + 1:c + 1] = st.special[i, b:c]
    sp2[i, b] = st.special[i, a]
    with pytest.raises(AssertionError, match="level 2"):
        ls.check_specials(broken(st, nspecial=ns, special=sp2), bonds, ls.LEVELS_W)
    # under FENE weights an outer entry must still be a partner of its level
    fene = ls.oracle_end("wca-fene", ls.LENGTHS[0])[1]
    fb = ls.check_bonds(fene)
    fwant = R.reference_specials(len(fene.x), fb)
    j = next(i for i in range(len(fene.x)) if fene.nspecial[i, 2] < fene.special.shape[1])
    ns, sp = fene.nspecial.copy(), fene.special.copy()
    sp[j, ns[j, 2]] = next(t for t in range(1, len(fene.x) + 1) if t != j + 1 and t not in fwant[j + 1])
    ns[j, 2] += 1
    with pytest.raises(AssertionError, match="no subset"):
        ls.check_specials(broken(fene, nspecial=ns, special=sp), fb, ls.FENE_W)
    # a one-sided bond: the last bond of one bead goes
    k = int(np.nonzero(st.num_bond)[0][5])
    nb = st.num_bond.copy()
    nb[k] -= 1
    with pytest.raises(AssertionError, match="of type"):
        ls.check_bonds(broken(st, num_bond=nb))
    # two extruder bonds on one bead (stored on both ends): a chain bond of a bead with an extruder takes the extruder type
    p = next(b for b in bonds if b[0] == ls.EXTRUDER)[1]
    q = next(b for b in bonds if b[0] == 1 and p in b[1:])
    q = q[1] + q[2] - p
    nb, bt, ba = st.num_bond.copy(), st.bond_type.copy(), st.bond_atom.copy()
    for u, w in ((p, q), (q, p)):
        m = next(m for m in range(nb[u - 1]) if ba[u - 1, m] == w and bt[u - 1, m] == 1)
        bt[u - 1, m] = ls.EXTRUDER
    with pytest.raises(AssertionError, match="more than one extruder"):
        ls.check_bonds(broken(st, num_bond=nb, bond_type=bt, bond_atom=ba))
    # the keyword `bonds` off by one
    with pytest.raises(AssertionError):
        ls.check_bonds(broken(st, thermo=dict(st.thermo, bonds=st.thermo["bonds"] + 1)))
    # an angle missing from one of its atoms
    ang = ls.oracle_end("angles-all", ls.LENGTHS[0])[1]
    ls.check_angles(ang)
    k = int(np.nonzero(ang.num_angle)[0][7])
    na = ang.num_angle.copy()
    na[k] -= 1
    with pytest.raises(AssertionError, match="copies on bead"):
        ls.check_angles(broken(ang, num_angle=na))
    with pytest.raises(AssertionError):
        ls.check_angles(broken(ang, thermo=dict(ang.thermo, angles=ang.thermo["angles"] - 1)))
    # the rule objects to an angle the bonds do not explain
    load = ls.oracle_end("angles-load", ls.LENGTHS[0])[1]
    lb, la = ls.check_bonds(load), ls.check_angles(load)
    assert la == ls.angle_rule(ls.system_of("angles-load"), lb, 2)
    assert la != ls.angle_rule(ls.system_of("angles-load"), [b for b in lb if b != [x for x in lb if x[0] == ls.EXTRUDER][0]], 2)
