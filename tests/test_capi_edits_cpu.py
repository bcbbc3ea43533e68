"""The inputs and edits of test_gpu_capi_edits.py (capi_edits.py), without a GPU: for every (input, edit) pair the long-double
reference alone shows that the edited state is a fair question - no candidate pair the cutoff test could judge either way, at
the evaluation after the edit and in each of the twelve steps that follow; no FENE bond inside the clamp; every position
finite and within one period of the box, every type in range - and that the edit does what its name says: which faces its rows
leave the box by, which slab owners change in which direction on 2, 3 and 4 slabs, which type changes it makes.  The deviation
of the FP64 oracle, started fresh from the edited system, from the reference is printed: the bounds of the GPU tests are 16 x
those figures (force_compare.bound, which fails here already if a figure needs more than the project's ceilings).
And on the host copies: a type outside 1 .. ntypes is refused before anything is written."""
import numpy as np
import pytest

import capi_edits as ce
import force_compare as fc
from neigh_reference import delta
from systems import write_data

ALL = sorted(ce.EDITS)
TWELVE = sorted(set(ce.TWELVE) | {e for e, _ in ce.SLABS})


@pytest.mark.parametrize("ename", ALL)
def test_edited_state_is_decided(ename):
    """Measured (oracle deviation of the forces at the edited state): between 3.9e-14 (far, outside) and 5.3e-14 (retype) over the
    thirteen edits, GPU bounds 6.3e-13 to 8.5e-13; the largest thermo keyword 1.9e-14 (press after far)."""
    name = ce.EDITS[ename]
    box = ce.box_of(name)
    prd = box[:, 1] - box[:, 0]
    ntypes = ce.INPUTS[name]()["system"]["ntypes"]
    for prop, ids, rows in ce.edit(ename):
        assert np.isfinite(np.asarray(rows, dtype=np.float64)).all() and ids.min() >= 1 and ids.max() <= len(ce.start(name)[0])
        if prop == "x":
            assert ((rows >= box[:, 0] - prd) & (rows <= box[:, 1] + prd)).all()
        if prop == "type":
            assert rows.min() >= 1 and rows.max() <= ntypes
        if prop.startswith("image"):
            assert rows.min() == -2 and rows.max() == 2
    S, ev, dev = ce.run0(ename)
    assert float(ev.gap) > delta(S.box, S.cutmax), (ev.gap_pair, float(ev.gap))
    assert ev.fene_clamped == []
    for k, v in dev.items():
        print("%s run 0: oracle deviation of %s = %.2e -> GPU bound %.2e" % (ename, k, v, fc.bound(v, fc.RUN0_CEILING)))


@pytest.mark.parametrize("ename", TWELVE)
def test_no_undecided_pair_in_the_twelve_steps_after(ename):
    """Measured (x / v / f / thermo rows, the oracle from the edited system against the reference): at most 5.9e-15 (far) / 7.8e-13
    (two-away) / 3.3e-11 (v) / 3.4e-14 (v: the largest over the edits - the GPU file quotes the oracle's figure of the case where
    the engine's is largest); four list builds in each; min |r^2 - cut^2| at least 3.6e-7 against 1.7e-10 required."""
    S, ref, dev, builds = ce.trajectory(ename)
    for k, v in dev.items():
        print("%s: oracle deviation of %s after %d steps = %.2e -> GPU bound %.2e" % (ename, k, fc.STEPS, v, fc.bound(v, fc.TRAJ_CEILING[k])))
    need = ce.required_gap(S, dev)
    print("%s: min |r^2 - cut^2| over %d evaluations = %.3e, required %.3e; %d list builds" % (ename, len(ref["gaps"]), float(min(ref["gaps"])), need, builds))
    assert len(ref["gaps"]) == fc.STEPS + 1 and float(min(ref["gaps"])) > need
    assert max(ref["fracs"]) < 1.0 and builds >= 3
    assert ref["last"].fene_clamped == []
    if ename == "retype-grouped":
        ids = ce.edit(ename)[0][1]
        x0 = ce.edited(ename)[0]
        xe = np.asarray(ref["xw"], dtype=np.float64)
        assert np.array_equal(xe[ids[:10] - 1], x0[ids[:10] - 1]) and (xe[ids[10:] - 1] != x0[ids[10:] - 1]).any(axis=1).all()


@pytest.mark.parametrize("first", [6, 7])
def test_no_undecided_pair_after_an_edit_in_the_middle(first):
    """`first` steps, `far`, the steps up to the twelfth (beyond it a FENE bond of this hot input enters the clamp): the state the mid-trajectory GPU test edits is the engine's own - its stand-in here is the
    oracle's, 4e-15 from it.  The same conditions: no pair near a cutoff in the evaluations after the edit, no FENE bond in
    the clamp, the oracle's deviations under the ceilings.  And what the two lengths are there for: step 6 rebuilds the lists,
    step 7 does not - a run of seven steps ends with the positions its last step-kernel launch wrote (and, with one lane per bead
    and the look-ahead, binned) still in place.
    Measured (x / v / f / rows): after 6 steps 4.0e-15 / 7.0e-13 / 1.2e-11 / 6.3e-15, min |r^2 - cut^2| 5.0e-5 against 7.8e-11
    required, 3 list builds; after 7 steps 3.7e-15 / 4.1e-13 / 2.8e-11 / 4.5e-15, 4.0e-5, 4 list builds."""
    S, ref, dev, builds, before, rebuilt = ce.mid_trajectory(first)
    for k, v in dev.items():
        print("far after %d steps: oracle deviation of %s at step 12 = %.2e -> GPU bound %.2e" % (first, k, v, fc.bound(v, fc.TRAJ_CEILING[k])))
    need = ce.required_gap(S, dev)
    print("min |r^2 - cut^2| over %d evaluations = %.3e, required %.3e; %d list builds" % (len(ref["gaps"]), float(min(ref["gaps"])), need, builds))
    assert len(ref["gaps"]) == fc.STEPS - first + 1 and float(min(ref["gaps"])) > need and max(ref["fracs"]) < 1.0 and builds >= 1
    assert ref["last"].fene_clamped == [] and S.evaluate(np.asarray(ref["xw"], dtype=np.float64)).fene_clamped == []
    assert rebuilt == (first == 6) and before == 2


def _hops(ename, world):
    """{(old owner, hop)}: hop = (new owner - old owner) mod world, over the rows of an x edit after Domain::pbc."""
    name = ce.EDITS[ename]
    box = ce.box_of(name)
    ids = ce.edited_ids(ce.edit(ename))
    so = ce.owner(ce.start(name)[0][ids - 1, 2], box, world)
    sn = ce.owner(ce.edited(ename)[0][ids - 1, 2], box, world)
    return so, (sn - so) % world


def test_the_input_spreads_over_every_slab():
    c = ce.offset_free()
    s = c["system"]
    box = ce.box_of("offset+free")
    x = ce.start("offset+free")[0]
    assert len(x) == 654 and len(c["free"]) == 24 and len(c["empty"]) >= 20 and len(c["vacated"]) >= 40
    assert (s["type"] == 1).all() and not np.isin(c["free"], s["bonds"][:, 1:]).any()
    prd = box[:, 1] - box[:, 0]
    pts = np.concatenate([x[c["free"] - 1], c["empty"]])
    d = ce.min_image(pts[:, None, :] - pts[None, :, :], prd)
    r = np.sqrt((d * d).sum(axis=2)) + 10.0 * np.eye(len(pts))
    assert r.min() > ce.SEPARATION - 1e-9
    w = prd[2] / 4
    for pts in (x[c["free"] - 1], c["vacated"]):
        own = ce.owner(pts[:, 2], box, 4)
        off = (pts[:, 2] - box[2, 0]) - own * w          # height above the slab's lower face
        for r in range(4):
            assert (own == r).sum() >= 3
            assert ((own == r) & (off < ce.GHOST)).any() and ((own == r) & (w - off < ce.GHOST)).any()
        assert (pts[:, 2] - box[2, 0] < ce.GHOST).any() and (box[2, 1] - pts[:, 2] < ce.GHOST).any()      # the periodic face


def test_the_edits_do_what_their_names_say():
    box = ce.box_of("offset+free")
    prd = box[:, 1] - box[:, 0]
    x0 = ce.start("offset+free")[0]
    n = len(x0)
    free = ce.offset_free()["free"]

    def rows_of(ename):
        calls = ce.edit(ename)
        return np.concatenate([c[1] for c in calls]), np.concatenate([c[2] for c in calls])

    def leaving(rows):
        """rows below the lower / at or above the upper face, per dimension"""
        return (rows < box[:, 0]).sum(axis=0).tolist(), (rows >= box[:, 1]).sum(axis=0).tolist()

    # near: the control - 40 rows, none farther than 0.05 in any coordinate
    ids, rows = rows_of("near")
    assert len(ids) == 40 and np.abs(rows - x0[ids - 1]).max() <= 0.05
    for world in ce.WORLDS:
        assert set(_hops("near", world)[1].tolist()) <= {0, 1, world - 1}
    # far: every free bead, inside the box, three cells away, across all three pairs of periodic faces; on slabs up and down
    # out of every slab (0 <-> W - 1 across the periodic face among them), on four never two slabs away
    ids, rows = rows_of("far")
    assert sorted(ids) == sorted(free) and leaving(rows) == ([0, 0, 0], [0, 0, 0])
    d = ce.min_image(rows - x0[ids - 1], prd)
    assert np.sqrt((d * d).sum(axis=1)).min() >= ce.THREE_CELLS
    assert ((np.abs(rows - x0[ids - 1]) > 0.5 * prd).sum(axis=0) >= 2).all()
    for world in ce.WORLDS:
        so, hop = _hops("far", world)
        got = set(zip(so.tolist(), hop.tolist()))
        assert got >= {(s, h) for s in range(world) for h in {1, world - 1}}, (world, got)
    assert 2 not in _hops("far", 4)[1]
    # outside: one row beyond each face, one beyond a corner, one on the upper z face itself; within one cutoff of the box
    ids, rows = rows_of("outside")
    assert len(ids) == 8 and len(set(ids.tolist())) == 8 and np.isin(ids, free).all() and [len(c[1]) for c in ce.edit("outside")] == [7, 1]
    below, above = rows < box[:, 0], rows >= box[:, 1]
    assert [int((below[k] | above[k]).sum()) for k in range(8)] == [1, 1, 1, 1, 1, 1, 3, 1]
    assert all(below[:6][:, d].any() and above[:6][:, d].any() for d in range(3))
    assert ((rows >= box[:, 0] - ce.CUT) & (rows <= box[:, 1] + ce.CUT)).all()
    assert rows[7, 2] == box[2, 1]
    xe, ie = ce.edited("outside")[0], ce.edited("outside")[2]
    assert xe[ids[7] - 1, 2] == box[2, 0] and ie[ids[7] - 1, 2] == ce.start("offset+free")[2][ids[7] - 1, 2] + 1
    for world in ce.WORLDS:
        so, hop = _hops("outside", world)
        assert (hop != 0).any() and (world < 4 or 2 not in hop)
    # rigid: every bead in one call of several blocks of 256 and a partial one.  A translation by (0.6 Lx, -0.4 Ly, 0) takes the
    # beads of the upper 0.6 of the box in x out by the upper x face and those of the lower 0.4 in y out by the lower y face
    # (not every bead: the ones it leaves inside are the ones a wrap applied to every row would move by a box length)
    ids, rows = rows_of("rigid")
    assert len(ids) == n == 654 and n > 2 * 256 and n % 256
    ie, i0 = ce.edited("rigid")[2], ce.start("offset+free")[2]
    up, down = rows[:, 0] >= box[0, 1], rows[:, 1] < box[1, 0]
    assert np.array_equal(ie[:, 0], i0[:, 0] + up) and np.array_equal(ie[:, 1], i0[:, 1] - down) and np.array_equal(ie[:, 2], i0[:, 2])
    assert leaving(rows) == ([0, int(down.sum()), 0], [int(up.sum()), 0, 0])
    assert 0.5 * n < up.sum() < 0.7 * n and 0.3 * n < down.sum() < 0.5 * n and (up & down).sum() > 100 and (~up & ~down).sum() > 100
    # rigid-z: every bead one slab of three up - every row leaves its slab, far more than half the migration buffer takes
    ids, rows = rows_of("rigid-z")
    so, hop = _hops("rigid-z", 3)
    assert len(ids) == n and (hop == 1).all()
    # two-away: four free beads whose new owner on four slabs is neither neighbour; on three slabs every other rank is one
    ids, rows = rows_of("two-away")
    assert len(ids) == 4 and np.isin(ids, free).all() and (_hops("two-away", 4)[1] == 2).all()
    assert set(_hops("two-away", 3)[1].tolist()) <= {0, 1, 2}
    # v: 257 different IDs (a block and one row), 50 of them with new rows; one ID three times, its last row another than the first two
    (prop, ids, rows), = ce.edit("v")
    v0 = ce.start("offset+free")[1]
    assert len(ids) == 259 and len(set(ids.tolist())) == 257 and ids[0] == ids[1] and (ids[2:] == ids[0]).sum() == 1
    k = 2 + int(np.nonzero(ids[2:] == ids[0])[0][0])
    assert not np.array_equal(rows[0], rows[k]) and not np.array_equal(rows[1], rows[k]) and not np.array_equal(rows[0], rows[1])
    ve = ce.edited("v")[1]
    assert ((ve != v0).any(axis=1)).sum() == 50 and np.array_equal(ve[ids[0] - 1], rows[k])
    assert len(ce.edit("f")[0][1]) == 50
    # image3 / image1: 30 rows with components -2 .. 2, half of the beads tethered
    for ename in ("image3", "image1"):
        (prop, ids, rows), = ce.edit(ename)
        assert len(ids) == 30 == len(set(ids.tolist())) and np.isin(ids, ce.tether_ids()).sum() == 15
        assert set(rows.ravel().tolist()) == {-2, -1, 0, 1, 2}
        assert np.array_equal(ce.edited(ename)[2][ids - 1], rows) and np.array_equal(ce.edited(ename)[0], x0)
        f, energy, dev = ce.tether(ename)
        S, ev, _ = ce.run0(ename)
        pull = np.sqrt(((np.asarray(f - ev.f, dtype=np.float64)) ** 2).sum(axis=1))
        print("%s: tether forces up to %.2f, energy %.3f; float64 restatement off by %.2e (f) %.2e (energy)" % (ename, pull.max(), float(energy), dev["f"], dev["energy"]))
        assert 0.5 < pull.max() < 10.0 and (pull > 0).sum() <= 15
    # retype: every ordered change of the cycle, fifteen times; retype-grouped: ten pinned beads to 1, ten mobile ones to 2
    for ename in ("retype", "retype-tall"):
        (prop, ids, rows), = ce.edit(ename)
        t0 = ce.start(ce.EDITS[ename])[3]
        assert sorted(zip(t0[ids - 1].tolist(), rows.tolist())) == sorted([(1, 2), (2, 3), (3, 1)] * 15)
    box = ce.box_of("types-tall")
    assert (box[2, 1] - box[2, 0]) / 3 >= 2 * (2.5 + 0.2) > (ce.box_of("types")[2, 1] - ce.box_of("types")[2, 0]) / 2
    assert len(set(ce.owner(ce.start("types-tall")[0][ids - 1, 2], box, 3).tolist())) == 3          # edited beads on every slab
    (prop, ids, rows), = ce.edit("retype-grouped")
    t0 = ce.start("offset-pinned")[3]
    assert (t0[ids[:10] - 1] == 2).all() and (rows[:10] == 1).all() and (t0[ids[10:] - 1] == 1).all() and (rows[10:] == 2).all()
    S = ce.reference_system("offset-pinned", ce.edited("retype-grouped")[3])
    assert (~S.mobile).sum() == 90 and not S.mobile[ids[:10] - 1].any() and S.mobile[ids[10:] - 1].all()
    # the row counts the scatter kernel has to meet: one row, a block and one row, several blocks, a repeated ID
    sizes = {len(set(c[1].tolist())) for e in ce.EDITS for c in ce.edit(e)}
    assert {1, 257, 654} <= sizes


def test_a_type_out_of_range_is_refused_on_the_host_copies(tmp_path):
    """Before the first run the host copies are the state.  The check stands ahead of everything scatter_subset_impl writes and
    ahead of its device branch (capi.cpp: it follows check_ids directly), so the same call on a device-resident state is refused
    by the same lines - no test sends one there."""
    from lammps_le_amd import LammpsError, lammps
    name = "types"
    path = str(tmp_path / "data.force")
    write_data(path, ce.INPUTS[name]()["system"])
    lmp = lammps(cmdargs=["-screen", "none"])
    for ln in ce.script("retype").split("\n"):
        w = ln.split("#")[0].split()
        lmp.command("read_data " + path if w and w[0] == "read_data" else ln)
    before = lmp.gather("type")
    for bad in (0, 4, -1):
        with pytest.raises(LammpsError, match="lammps_scatter_atoms_subset: invalid atom type %d for atom ID 9" % bad):
            lmp.scatter_ids("type", [5, 9, 11], [2, bad, 3])
        assert np.array_equal(lmp.gather("type"), before)          # nothing was written, not even the valid row ahead of it
    lmp.scatter_ids("type", [5, 9, 11], [2, 3, 3])
    after = lmp.gather("type")
    assert after[[4, 8, 10]].tolist() == [2, 3, 3] and (after != before).sum() <= 3
    assert lmp.stat("host_downloads") == 0
    lmp.close()
