"""Edits of the device-resident state through the C-ABI's subset calls, held to the long-double reference (capi_edits.py;
test_capi_edits_cpu.py proves the conditions on its inputs without a GPU): k_subset_scatter / k_subset_gather of
kernels_capi.hip and the three routes scatter_subset_impl (capi.cpp) chooses between - the device write, the device write plus
the host write that keeps current host copies current, and the whole-system download with a re-upload at the next run.

One protocol: the script and `run 0` (the device holds the input, exactly), optionally a whole gather (the host copies are
current) or none (they are stale), the edit, then what follows - a gather, `run 0`, twelve steps.  host_downloads is read
immediately before and after the subset calls only.

Bounds: force_compare.bound of the deviation of the FP64 oracle, started fresh from the edited system, from the reference on
that system (16 x, floor 1e-13, the project's ceilings); for the tether quantities of the image edits, which the oracle does
not have, 16 x the deviation of the float64 restatement of the same reference.  What was written, the wrapped positions and
image flags after `run 0`, pinned beads and restarts are compared bit for bit."""
import os

import numpy as np
import pytest

import capi_edits as ce
import force_compare as fc
from neigh_reference import delta
from systems import run_product, write_data
from test_gpu_force import report

pytestmark = pytest.mark.gpu

WHOLE = ("x", "v", "f", "image", "type")
HOST = ["stale", "current"]
SWITCHES = ("LAMMPS_LE_LPB", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO", "LAMMPS_LE_NO_FUSED_BIN",
            "LAMMPS_LE_NO_FUSED_GROUPS")
# the route an edit takes on one GPU: whole-system downloads across its subset calls, by the state of the host copies.  The
# fallback downloads while the host copies are stale; with current ones there is nothing to fetch (Engine::download returns),
# it edits them and the next run uploads
DOWNLOADS = {"retype-grouped": {"stale": 1, "current": 0}}


def whole(p):
    return {q: p.gather(q) for q in WHOLE}


def begin(tmp_path, ename, host, monkeypatch, env=None):
    """-> (handle, the whole gather before the edit): the script, `run 0`, and the host copies stale or current."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    name = ce.EDITS[ename]
    p = run_product(ce.script(ename) + "run 0\n", ce.INPUTS[name]()["system"], tmp_path)
    before = whole(p)
    whole_f = before["f"]
    x, v, image, typ = ce.start(name)
    assert np.array_equal(before["x"], x) and np.array_equal(before["v"], v) and np.array_equal(before["image"], image)
    assert np.array_equal(before["type"], typ)
    if host == "stale":
        p.command("run 0")          # the same state once more: the host copies are behind again.  (The forces of this
        before["f"] = p.gather_ids("f", np.arange(1, len(x) + 1, dtype=np.int32))      # evaluation, through a subset gather of K = N)
        assert fc.relerr(before["f"], whole_f) < 1e-13
    return p, before


def apply(p, ename, host):
    """The edit, with the downloads its subset calls (and nothing else) caused checked against the route it has to take."""
    d0 = p.stat("host_downloads")
    ce.send(p, ce.edit(ename))
    d1 = p.stat("host_downloads")
    assert d1 - d0 == DOWNLOADS.get(ename, {}).get(host, 0), (ename, host, d1 - d0)
    # the fallback leaves the host copies as the state (the next run uploads), the device paths leave the device current -
    # which tells the two apart also where the host copies were current and the fallback had nothing to download
    assert p.stat("device_current") == (0 if ename in DOWNLOADS else 1), (ename, host)


def compare_run0(label, p, S, ev, dev, v, f_ref=None, f_dev=None):
    bad = report(label + " f", p.gather("f"), ev.f if f_ref is None else f_ref, dev["f"] if f_dev is None else f_dev, fc.RUN0_CEILING)
    ref = ce.thermo_keywords(S, ev, v)
    for k in fc.THERMO_KEYS:
        bad += report("%s %s" % (label, k), p.get_thermo(k), ref[k], dev[k], fc.RUN0_CEILING)
    return bad


def compare_steps(label, S, ref, dev, obuilds, got, first=0):
    """test_gpu_force.compare_trajectory for a reference that starts at the engine's step `first`."""
    assert float(min(ref["gaps"])) > ce.required_gap(S, dev)
    bad = report(label + " x", S.unwrapped(got["x"], got["image"]), ref["x"][-1], dev["x"], fc.TRAJ_CEILING["x"])
    bad += report(label + " v", got["v"], ref["v"][-1], dev["v"], fc.TRAJ_CEILING["v"])
    bad += report(label + " f", got["f"], ref["f"], dev["f"], fc.TRAJ_CEILING["f"])
    rows = np.asarray(got["rows"])
    rows = rows[len(rows) - [int(r[0]) for r in rows][::-1].index(first) - 1:]          # the rows of the last run
    steps = [int(r[0]) for r in rows]
    last = first + len(ref["x"]) - 1
    assert steps == sorted({s for s in range(first, last + 1) if s % 4 == 0} | {first, last}), steps
    want = [[ref["rows"][s - first][key] for key in fc.ROW_KEYS] for s in steps]
    bad += report(label + " thermo rows", rows[:, 1:6], want, dev["rows"], fc.TRAJ_CEILING["rows"])
    assert not bad, "\n".join(bad)
    assert obuilds >= (3 if last - first == fc.STEPS else 1) and got["builds"] == obuilds, (got["builds"], obuilds)


def state_of(p):
    return dict(x=p.gather("x"), v=p.gather("v"), image=p.gather("image"), f=p.gather("f"), type=p.gather("type"),
                rows=np.asarray(p.thermo_history()), builds=int(p.stat("neigh_builds")))


# ------------------------------------------------------------------------------------------------
# (a) what was written is what is there
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOST)
@pytest.mark.parametrize("ename", sorted(ce.EDITS))
def test_what_was_written_is_what_is_there(tmp_path, ename, host, monkeypatch):
    """Straight after the scatter, before any run: gather_ids of the edited IDs returns the rows sent, bit for bit (of a repeated
    ID the last; image also as the packed word through gather_atoms_subset("image", 0, 1, ...)), and the whole gather of x, v, f,
    image and type differs from the one before the edit in the edited rows and columns and in nothing else - a wrong slot, a wrong
    stride in the image words or a type table that disagrees with pos.w shows here.  Row counts: 1 (`outside`), 257 different IDs
    with one of them three times (`v`), 654 (`rigid`: two blocks and a partial one).  No device-path edit downloads;
    retype-grouped (a fix acts on a group) downloads once while the host copies are stale."""
    p, before = begin(tmp_path, ename, host, monkeypatch)
    calls = ce.edit(ename)
    d0 = p.stat("host_downloads")
    ce.send(p, calls)
    for prop, ids, rows in calls:
        uid, urows = ce.last_rows(ids, rows)
        if prop.startswith("image"):
            got = np.ctypeslib.as_array(p.gather_atoms_subset("image", 0, 1, len(uid), [int(t) for t in uid])).copy()
            assert np.array_equal(got, ce.packed(urows))
            prop = "image"
        got = p.gather_ids(prop, uid)
        assert got.dtype == np.asarray(urows).dtype and np.array_equal(got, urows), (prop, np.nonzero(got != urows))
        if len(uid) < len(ids):          # in the caller's order, repeats included: every copy of a repeated ID shows its last row
            want = {int(t): r for t, r in zip(uid, urows)}
            assert np.array_equal(p.gather_ids(prop, ids), np.array([want[int(t)] for t in ids]))
    d1 = p.stat("host_downloads")
    assert d1 - d0 == DOWNLOADS.get(ename, {}).get(host, 0), (ename, host, d1 - d0)
    assert p.stat("device_current") == (0 if ename in DOWNLOADS else 1), (ename, host)
    after = whole(p)
    x, v, image, typ, frows = ce.written((before["x"], before["v"], before["image"], before["type"]), calls)
    f = before["f"].copy()
    for t, r in frows.items():
        f[t - 1] = r
    for q, want in zip(WHOLE, (x, v, f, image, typ)):
        diff = np.nonzero(after[q] != want)
        assert len(diff[0]) == 0, "%s: %d entries are not what was written, first at row %d" % (q, len(diff[0]), diff[0][0])
    changed = {q for q in WHOLE if not np.array_equal(after[q], before[q])}
    assert changed == {c[0].replace("image1", "image") for c in calls}, changed
    p.close()


# ------------------------------------------------------------------------------------------------
# (b) `run 0` after the edit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", HOST)
@pytest.mark.parametrize("ename", sorted(e for e in ce.EDITS if e not in ("rigid-z", "two-away")))
def test_run0_after_the_edit(tmp_path, ename, host, monkeypatch):
    """`run 0` after the edit: the gathered x and image are the wrapped edited state bit for bit (Domain::pbc once per dimension;
    the row of `outside` with z == hi comes back as lo with the image one higher); per-bead forces, evdwl, ebond, pe, ke, temp,
    press and the six tensor components against force_reference on the edited state; after `f` the forces are the reference's
    (setup recomputes them); after image3 / image1 the forces carry the tethers of extforce_reference and the fix reports its
    energy; after retype the new coefficients, cutoffs and masses are in force.
    Measured on an MI355X: see MEASURED at the end of this file."""
    name = ce.EDITS[ename]
    p, before = begin(tmp_path, ename, host, monkeypatch)
    apply(p, ename, host)
    p.command("run 0")
    x, v, image, typ = ce.edited(ename)
    got = whole(p)
    for q, want in (("x", x), ("image", image), ("v", v), ("type", typ)):
        assert np.array_equal(got[q], want), (q, int((got[q] != want).sum()))
    S, ev, dev = ce.run0(ename)
    assert float(ev.gap) > delta(S.box, S.cutmax)
    label = "%s %s" % (ename, host)
    if ename.startswith("image"):
        f, energy, tdev = ce.tether(ename)
        # the tether adds k d to a force the oracle is dev["f"] off in: the two deviations add up (both relative, floor 1)
        bad = compare_run0(label, p, S, ev, dev, v, f_ref=f, f_dev=dev["f"] + tdev["f"])
        bad += report(label + " tether energy", p.extract_fix("tether", 0, 0), energy, tdev["energy"], fc.RUN0_CEILING)
        ids = ce.edit(ename)[0][1]
        pull = np.asarray(f - ev.f, dtype=np.float64)
        assert (np.abs(pull[ids[:15] - 1]).max(axis=1) > 0.05).sum() >= 10 and not pull[ids[15:] - 1].any()
    else:
        bad = compare_run0(label, p, S, ev, dev, v)
    assert not bad, "\n".join(bad)
    if ename == "outside":
        t = int(ce.edit(ename)[1][1][0])
        assert got["x"][t - 1, 2] == S.box[2, 0] and got["image"][t - 1, 2] == before["image"][t - 1, 2] + 1
    p.close()


# ------------------------------------------------------------------------------------------------
# (c) twelve steps after the edit
# ------------------------------------------------------------------------------------------------
# one lane per bead (LAMMPS_LE_LPB=1; by default systems of this size take four): the shape in which the step kernel bins the
# positions it writes, so that the rebuild after it finds them binned (RB_PREBINNED) - unless an x scatter came in between,
# which has to say so (note_positions_replaced)
PLAIN = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}
AHEAD = {"LAMMPS_LE_LPB": "1"}          # ... with the look-ahead (by default up to 64000 beads): its thermo steps are unfused
TWELVE = [(e, {}) for e in ce.TWELVE] + [("far", {"LAMMPS_LE_NO_FUSE": "1"}), ("far", PLAIN), ("far", AHEAD)]
SHAPE = lambda env: "-unfused" if "LAMMPS_LE_NO_FUSE" in env else "-plain" if env == PLAIN else "-ahead" if env else ""


@pytest.mark.parametrize("host", HOST)
@pytest.mark.parametrize("ename,env", TWELVE, ids=[e + SHAPE(env) for e, env in TWELVE])
def test_twelve_steps_after_the_edit(tmp_path, ename, env, host, monkeypatch):
    """`run 12` straight after the edit (its setup has to wrap, bin, migrate nothing and build the lists for beads that are
    three cells from where the last build saw them): unwrapped x, v, f after the last step, every thermo row (thermo 4) and the
    list builds against the reference and the oracle started from the edited system, as test_gpu_force.compare_trajectory does.
    retype: the new masses drive the integration.  retype-grouped: the ten pinned beads that are of type 1 now keep their
    positions bit for bit (the group is what it was when it was defined), the ten mobile ones that are of type 2 now keep moving;
    its subset call downloads once (the fallback), every other edit's not at all.
    Measured on an MI355X: see MEASURED at the end of this file."""
    p, before = begin(tmp_path, ename, host, monkeypatch, env)
    apply(p, ename, host)
    p.command("run %d" % fc.STEPS)
    got = state_of(p)
    S, ref, dev, obuilds = ce.trajectory(ename)
    compare_steps("%s %s%s" % (ename, host, SHAPE(env)), S, ref, dev, obuilds, got)
    if "LAMMPS_LE_NO_FUSE" in env:
        assert int(p.stat("steps_unfused")) == fc.STEPS
    elif env == PLAIN:
        assert int(p.stat("steps_fused")) == 9 and int(p.stat("steps_fused_thermo")) == 3
    elif env:
        assert int(p.stat("steps_fused")) == 9 and int(p.stat("steps_unfused")) == 3
    if ename == "retype-grouped":
        ids = ce.edit(ename)[0][1]
        x0 = ce.edited(ename)[0]
        assert (~S.mobile).sum() == 90 and np.array_equal(got["x"][~S.mobile], x0[~S.mobile])
        assert (got["type"][ids[:10] - 1] == 1).all() and (got["x"][ids[10:] - 1] != x0[ids[10:] - 1]).any(axis=1).all()
    p.close()


# ------------------------------------------------------------------------------------------------
# (d) an edit in the middle of a trajectory
# ------------------------------------------------------------------------------------------------
# shape: (switches, steps before the edit).  thermo 4 and list builds on the steps 3, 6, 9, 12: a first run of seven steps ends
# on a step that neither rebuilds nor follows a thermo step
MID = {"default": ({}, 6), "plain": (PLAIN, 6), "ahead": (AHEAD, 7), "ahead-unfused-thermo": (dict(AHEAD, LAMMPS_LE_NO_FUSED_THERMO="1"), 7)}


@pytest.mark.parametrize("shape", sorted(MID))
def test_edit_in_the_middle_of_a_trajectory(tmp_path, shape, monkeypatch):
    """run 6 (or 7); a whole gather; `far`; on to step 12.  The reference continues from the gathered state with the edit applied - only
    its start is the engine's, every force and step after that its own; the oracle likewise.  (The oracle's own state after as many
    steps with the edit applied is proved a fair question without a GPU, test_capi_edits_cpu.py; the engine's, 4e-15 from it,
    is checked here before the second run.)
    ahead: one lane per bead with the look-ahead, and a first run of SEVEN steps, whose last does not rebuild (step 6 does).  The
    launch of step 6 carries the first half of step 7 and bins the positions it writes; step 7, the thermo step of a
    look-ahead shape, goes through the unfused kernels, which leave those bins and their flag alone: the run ends with
    bins_ready set and bins that match the positions.  The setup of the second run takes them (RB_PREBINNED) unless the scatter
    said that positions were replaced (note_positions_replaced) - without that the moved beads are sorted into the cells they
    left.  plain (no look-ahead): the thermo step is the energy variant of the step kernel, which clears the flag itself.
    Measured on an MI355X: see MEASURED at the end of this file."""
    env, first = MID[shape]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    name = "offset+free"
    p = run_product(ce.script("far") + "run %d\n" % first, ce.INPUTS[name]()["system"], tmp_path)
    paths = {k: int(p.stat(k)) for k in ("steps_fused", "steps_fused_thermo", "steps_unfused")}
    print(shape, paths)
    if shape == "plain":
        assert paths["steps_unfused"] == 0 and paths["steps_fused_thermo"] >= 1 and sum(paths.values()) == first, paths
    elif shape.startswith("ahead"):          # the thermo steps (4 and the last) unfused, every other step through the step kernel
        assert paths == dict(steps_fused=first - 2, steps_fused_thermo=0, steps_unfused=2), paths
    assert int(p.stat("neigh_builds")) == 2          # (steps 3 and 6: a run of seven steps does not end on a rebuild)
    mid = whole(p)
    state = ce.edited_state((mid["x"], mid["v"], mid["image"], mid["type"]), ce.edit("far"), ce.box_of(name))
    S, ref, dev, obuilds = ce.trajectory_from("far", name, state, fc.STEPS - first)
    assert float(min(ref["gaps"])) > ce.required_gap(S, dev) and ref["last"].fene_clamped == []
    apply(p, "far", "current")
    p.command("run %d" % (fc.STEPS - first))
    compare_steps("far after %d steps, %s" % (first, shape), S, ref, dev, obuilds, state_of(p), first=first)
    p.close()


# ------------------------------------------------------------------------------------------------
# (e) slabs: ranks as threads over the in-process transport
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ename,world", ce.SLABS, ids=["%s-%d" % c for c in ce.SLABS])
def test_edit_on_slabs(tmp_path, ename, world, monkeypatch):
    """The edit on `world` z slabs (ghost cutoff 2.0): near, far and outside stay on the device on 2, 3 and 4 ranks - far and
    outside leave their slabs through k_dd_leave, up, down and across the periodic face; two-away (4 ranks: a new owner that is no
    neighbour) and rigid-z (3 ranks: every bead leaves, more than half the migration buffer) take the whole-system route, one
    download on every rank; retype-tall (3 ranks; `types` is too short to be cut) stays on the device.  Then `run 0` (wrapped x and image bit for bit, forces and thermo)
    and twelve steps against the same references under the same bounds as on one GPU; every rank reports the same state, and a
    subset gather of the edited IDs returns the whole gather's rows.
    Measured on an MI355X: see MEASURED at the end of this file."""
    from test_gpu_capi import _lines, _run_local_ranks
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LAMMPS_LE_COMM_TIMEOUT", "30")          # (a rank that fails leaves the others waiting for this long)
    name = ce.EDITS[ename]
    path = str(tmp_path / "data.force")
    write_data(path, ce.INPUTS[name]()["system"])
    calls = ce.edit(ename)
    ids = ce.edited_ids(calls)

    def body(lmp, rank):
        out = dict(ranks=lmp.stat("comm_nranks"), nlocal=lmp.stat("nlocal"))
        d0 = lmp.stat("host_downloads")
        ce.send(lmp, calls)
        out["downloads"] = lmp.stat("host_downloads") - d0
        lmp.command("run 0")
        out["run0"] = dict(whole(lmp), keywords={k: lmp.get_thermo(k) for k in fc.THERMO_KEYS})
        lmp.command("run %d" % fc.STEPS)
        out["end"] = state_of(lmp)
        out["subset"] = {q: lmp.gather_ids(q, ids) for q in ("x", "v", "image", "type")}
        out["nlocal_end"] = lmp.stat("nlocal")
        return out

    res = _run_local_ranks(world, _lines(ce.script(ename) + "run 0\n", path), body)
    x, v, image, typ = ce.edited(ename)
    S, ev, dev = ce.run0(ename)
    St, ref, tdev, obuilds = ce.trajectory(ename)
    keys = ce.thermo_keywords(S, ev, v)
    for rank, r in enumerate(res):
        assert r["ranks"] == world and 0 < r["nlocal"] < S.n and 0 < r["nlocal_end"] < S.n
        assert r["downloads"] == ce.SLAB_DOWNLOADS.get(ename, 0), (ename, world, rank, r["downloads"])
        for q in ("x", "v", "f", "image", "type"):
            assert np.array_equal(r["run0"][q], res[0]["run0"][q]) and np.array_equal(r["end"][q], res[0]["end"][q]), (rank, q)
        for q in ("x", "v", "image", "type"):
            assert np.array_equal(r["subset"][q], r["end"][q][ids - 1]), (rank, q)
    assert sum(r["nlocal"] for r in res) == S.n == sum(r["nlocal_end"] for r in res)
    r = res[0]
    for q, want in (("x", x), ("image", image), ("v", v), ("type", typ)):
        assert np.array_equal(r["run0"][q], want), (q, int((r["run0"][q] != want).sum()))
    label = "%s %d ranks" % (ename, world)
    bad = report(label + " f", r["run0"]["f"], ev.f, dev["f"], fc.RUN0_CEILING)
    for k in fc.THERMO_KEYS:
        bad += report("%s %s" % (label, k), r["run0"]["keywords"][k], keys[k], dev[k], fc.RUN0_CEILING)
    assert not bad, "\n".join(bad)
    compare_steps(label, St, ref, tdev, obuilds, r["end"])


# ------------------------------------------------------------------------------------------------
# (f) a type edit meeting the LE fixes
# ------------------------------------------------------------------------------------------------
def test_retype_meets_the_le_fixes(tmp_path):
    """The scenario of test_gpu_capi.py (20000 beads, barriers of types 2 and 3, loading, unloading and extrusion): 100 steps, then
    20 neutral beads become barriers (ten left, ten right) and 10 barrier beads neutral through the subset call, then 300 steps.
    Bond set, the three fix vectors and the local order equal the oracle's (Oracle.set_type) exactly, x within the 1e-9 of that
    file; the scatter downloads nothing (the LE fixes act on `all`)."""
    from test_gpu_capi import N1, _compare, _result, _script, _system
    from systems import OracleScript
    s = _system(N1)
    script0 = _script() + "run 100\n"
    o = OracleScript(s).run(script0)
    typ = o.types().astype(np.int32)
    rng = np.random.RandomState(21)
    neutral = rng.permutation(np.nonzero(typ == 1)[0] + 1)[:20]
    barrier = rng.permutation(np.nonzero(typ > 1)[0] + 1)[:10]
    ids = np.concatenate([neutral, barrier]).astype(np.int32)
    rows = np.array([2] * 10 + [3] * 10 + [1] * 10, dtype=np.int32)
    order = rng.permutation(30)
    ids, rows = ids[order], rows[order]
    typ[ids - 1] = rows
    o.set_type(typ)
    o.run(300)
    lmp = run_product(script0, s, tmp_path)
    b0 = lmp.stat("host_downloads")
    lmp.scatter_ids("type", ids, rows)
    assert np.array_equal(lmp.gather_ids("type", ids), rows)
    assert lmp.stat("host_downloads") == b0, "a type scatter under fixes on `all` took the re-upload path"
    lmp.command("run 300")
    assert lmp.stat("host_downloads") == b0
    _compare(o, _result(lmp))
    lmp.close()


# ------------------------------------------------------------------------------------------------
# (g) restart
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ename", ["image3", "retype"])
def test_restart_after_the_edit(tmp_path, ename, monkeypatch):
    """The edit, write_restart, then read_restart into a fresh handle and run 12: equals run 12 on the edited handle bit for bit
    - the file carries the image flags and the types the scatter wrote (and, for image3, the tether's origins)."""
    from lammps_le_amd import lammps
    from test_gpu_extforce import _after_restart
    p, before = begin(tmp_path, ename, "stale", monkeypatch)
    apply(p, ename, "stale")
    path = os.path.join(str(tmp_path), "edited.restart")
    p.command("write_restart " + path)
    p.command("run %d" % fc.STEPS)
    want = state_of(p)
    p.close()
    q = lammps(cmdargs=["-screen", "none"])
    q.command("read_restart " + path)
    for ln in _after_restart(ce.script(ename)):
        q.command(ln)
    q.command("run %d" % fc.STEPS)
    got = state_of(q)
    q.close()
    for k in ("x", "v", "f", "image", "type"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["rows"][-4:], want["rows"][-4:]) and got["builds"] == want["builds"]
    x, v, image, typ = ce.edited(ename)
    assert np.array_equal(want["type"], typ)


MEASURED = """Measured on an MI355X (engine / oracle deviation from the reference / bound, relative with floor 1; the largest over the
cases, stale and current host copies alike - the two states differ in no figure; the oracle's figure is that of the case in
which the engine's is largest - its own largest, 3.4e-14 for the thermo rows, is in test_capi_edits_cpu.py):
  run 0 after the edit, one GPU     forces 5.8e-14 / 5.1e-14 / 8.1e-13 (retype-tall; bounds from 6.3e-13); every thermo keyword at
                                    most 3.1e-15 (oracle 1.9e-14) against bounds of 1.0e-13 to 3.0e-13; the tether's energy
                                    1.6e-16 / 1.6e-16 / 1.0e-13, the forces with the tethers 5.1e-14 / 4.1e-14 / 6.6e-13
  twelve steps after, one GPU       x 5.9e-15 / 5.9e-15 / 1.0e-13 (far), v 7.2e-13 / 7.2e-13 / 1.2e-11 (rigid), f 3.3e-11 / 3.3e-11 /
                                    5.3e-10 (v), thermo rows 1.1e-14 / 2.4e-14 / 3.8e-13 (far, unfused); list builds 4 = the oracle's
  far, twelve steps, one lane/bead  x 5.9e-15 / 5.9e-15 / 1.0e-13, v 5.8e-13 / 5.7e-13 / 9.2e-12, f 1.2e-11 / 1.2e-11 / 2.0e-10, rows
                                    1.1e-14 / 2.4e-14 / 3.8e-13 (9 fused steps, 3 fused thermo steps)
  far, twelve steps, look-ahead     as one lane/bead but 9 fused and 3 unfused steps, rows 1.1e-14 / 2.4e-14 / 3.8e-13
  far after 7 of 12 steps, one lane per bead with the look-ahead (also with LAMMPS_LE_NO_FUSED_THERMO; 5 fused, 2 unfused steps
                                    before the edit, which meets binned positions): x 3.8e-15 / 3.7e-15 / 1.0e-13, v 4.1e-13 /
                                    4.1e-13 / 6.5e-12, f 2.8e-11 / 2.7e-11 / 4.4e-10, rows 5.0e-15 / 5.7e-15 / 1.0e-13; without
                                    note_positions_replaced in the scatter: x 7.3e-2, v 1.4, f 2.0, rows 0.40
  far after 6 of 12 steps           (default shape; one lane per bead: the same but rows 5.6e-15 / 6.9e-15 / 1.1e-13)
                                    x 3.9e-15 / 4.0e-15 / 1.0e-13, v 7.0e-13 / 7.0e-13 / 1.1e-11, f 1.2e-11 / 1.2e-11 / 1.8e-10, rows
                                    1.9e-15 / 6.8e-15 / 1.1e-13
  slabs (2, 3, 4 ranks)             run-0 forces 5.8e-14 / 5.1e-14 / 8.1e-13, keywords at most 2.6e-15 (press; the six tensor
                                    components at most 2.6e-16 / 2.3e-15 / 1.0e-13); after twelve steps x 5.9e-15 /
                                    5.9e-15 / 1.0e-13, v 7.8e-13 / 7.8e-13 / 1.3e-11, f 2.4e-11 / 2.4e-11 / 3.9e-10 (two-away), rows
                                    1.6e-14 / 2.1e-14 / 3.3e-13
Routes proved: the device write (every edit but three: no download; with current host copies the host write on top, which the
following run shows to agree; stat device_current stays 1), migration through k_dd_leave (far and outside on 2, 3, 4 ranks), the fallback by distance
(two-away, 4 ranks), by count (rigid-z, 3 ranks) and by a fix on a group (retype-grouped): one download each on every rank
(retype-grouped with current host copies: none to make - device_current drops to 0, which a device write never does).
What these tests found: on three slabs k_dd_leave sent a bead scattered into the upper half of the upper neighbour's slab DOWN
(the direction came from the sign of its offset, which wraps at Lz / 2), to a rank that does not own it - far and outside on 3
ranks were 0.77 off in the run-0 forces.  It now goes to the neighbour that owns it."""
