"""pair_style soft and fix adapt on the HIP path: `run 0` against the long-double reference (soft_reference.py) and the recorded
reference run; 48 steps with fix adapt against recorded reference runs in the four shapes of the step (four lanes per bead, one
lane, one lane with loads ahead, unfused kernels); two z slabs against one GPU; the push-off of a phantom walk end to end.
Inputs, scripts and fixtures: soft_runs.py; the conditions they were made under are checked in test_soft_cpu.py."""
import functools

import numpy as np
import pytest

import force_compare as fc
import reference_runs as rr
import soft_runs as so
from systems import CHAIN_SCRIPT, lattice_chain, run_product

pytestmark = pytest.mark.gpu

PLAIN = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "0"}
AHEAD = {"LAMMPS_LE_LPB": "1", "LAMMPS_LE_AHEAD_MAX_N": "1000000000"}
FOUR = {"LAMMPS_LE_LPB": "4"}
UNFUSED = {"LAMMPS_LE_NO_FUSE": "1"}
SHAPES = {"four": FOUR, "plain": PLAIN, "ahead": AHEAD, "unfused": UNFUSED}
SWITCHES = ("LAMMPS_LE_LPB", "LAMMPS_LE_LPB_MAX_N", "LAMMPS_LE_AHEAD_MAX_N", "LAMMPS_LE_NO_FUSE", "LAMMPS_LE_NO_FUSED_THERMO",
            "LAMMPS_LE_NO_FUSED_BIN", "LAMMPS_LE_NO_FUSED_GROUPS", "LAMMPS_LE_DIAG_STEP", "LAMMPS_LE_STEP_LDS_PAD")
STATS = ("steps_fused", "steps_fused_group", "steps_fused_thermo", "steps_unfused", "steps_fused_wall", "steps_fused_soft")


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)


@functools.lru_cache(maxsize=None)
def a_reference():
    return so.a_reference()


# ------------------------------------------------------------------------------------------------------------------
# run 0
# ------------------------------------------------------------------------------------------------------------------
def test_run0_against_reference_and_record(tmp_path, monkeypatch):
    """Forces, evdwl, press and the pressure tensor of the (a) input - 449 interacting pairs, 20 of them 0.1 to 0.3 apart, one
    coincident pair, list entries with special bits, three coefficient sets - against soft_reference.py and against the
    recorded reference run.  Bounds: 16 x the recorded run's own deviation from the long-double reference (soft_runs.json:
    forces 5.4e-14, thermo row 2.3e-15), at least 1e-13, relative to max(1, |value|)."""
    set_env(monkeypatch, {})
    S, ev, s = a_reference()
    fx, m = so.fixture("a"), so.meta()["a"]
    p = run_product(so.a_script(), s, tmp_path)
    f = p.gather("f")
    row = np.array([p.get_thermo(k) for k in so.A_THERMO[1:]])
    p.close()
    assert np.isfinite(f).all() and np.isfinite(row).all()
    th = S.thermo(ev, np.asarray(s["v"]))
    want = [th[k] for k in so.A_THERMO[1:]]
    bf = fc.bound(m["reference_deviation"]["f"], fc.RUN0_CEILING)
    br = fc.bound(m["reference_deviation"]["rows"], fc.RUN0_CEILING)
    figures = dict(f_ref=fc.relerr(f, ev.f), f_rec=fc.relerr(f, fx["f"]), row_ref=fc.relerr(row, want), row_rec=fc.relerr(row, fx["row"][1:]))
    print("run 0: forces %.2e (reference) %.2e (record) bound %.2e; thermo row %.2e %.2e bound %.2e" %
          (figures["f_ref"], figures["f_rec"], bf, figures["row_ref"], figures["row_rec"], br))
    assert figures["f_ref"] < bf and figures["f_rec"] < bf, figures
    assert figures["row_ref"] < br and figures["row_rec"] < br, figures


# ------------------------------------------------------------------------------------------------------------------
# 48 steps with fix adapt
# ------------------------------------------------------------------------------------------------------------------
def unwrapped(x, image, box):
    box = np.asarray(box, dtype=np.float64)
    return np.asarray(x) + np.asarray(image) * (box[:, 1] - box[:, 0])[None, :]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", so.NAMES)
def test_steps_against_recorded_runs(tmp_path, monkeypatch, name, shape):
    """x (unwrapped), v, f after the last step and every thermo row against the recorded reference run.  Bounds: 16 x the spread
    of three reference reruns from starts moved by one ulp (x, v, f: absolute; a thermo value: at least 5e-15 of its size, the
    rule of reference_runs.thermo_bound).  The fused shapes count every plain step of a soft run as steps_fused_soft, the
    unfused shape none; the lj/cut and r-RESPA scenarios none in any shape."""
    set_env(monkeypatch, SHAPES[shape])
    scn, fx, meta = so.BY_NAME[name], so.fixture(name), so.meta()["scenarios"][name]
    s = so.b_system()
    p = run_product(scn["script"], s, tmp_path)
    got = dict(x=unwrapped(p.gather("x"), p.gather("image"), s["box"]), v=p.gather("v"), f=p.gather("f"))
    stats = {k: int(p.stat(k)) for k in STATS}
    copies = int(p.stat("pair_table_copies"))
    rows = np.asarray(p.thermo_history(), dtype=np.float64)
    p.close()
    want = dict(x=unwrapped(fx["x"][-1], fx["image"][-1], s["box"]), v=fx["v"][-1], f=fx["f"])
    bad = []
    for q in ("x", "v", "f"):
        err, b = float(np.abs(got[q] - want[q]).max()), rr.FACTOR * meta["spread"][q]
        print("%s %s %s: %.2e  bound %.2e" % (name, shape, q, err, b))
        if not err <= b:
            bad.append("%s: %.3e exceeds %.3e" % (q, err, b))
    rec, sp = fx["thermo"], np.asarray(meta["spread"]["thermo"])
    assert rows.shape[0] == rec.shape[0] and [int(r[0]) for r in rows] == [int(r[0]) for r in rec]
    terr = np.abs(rows[:, 1:6] - rec[:, 1:6])
    tb = rr.FACTOR * np.maximum(sp[:, :5], rr.THERMO_FLOOR * np.maximum(np.abs(rec[:, 1:6]), 1.0))
    print("%s %s thermo rows: worst %.2e of its bound" % (name, shape, float((terr / tb).max())))
    if not (terr <= tb).all():
        k = np.unravel_index(np.argmax(terr / tb), terr.shape)
        bad.append("thermo row %d %s: %.3e exceeds %.3e" % (k[0], so.THERMO[k[1] + 1], terr[k], tb[k]))
    # the path every step took: the last step of a run and the thermo steps store energies (unfused), the others are plain steps
    last = so.last_step(scn)
    plain = 6 if name == "reset" else last - len(rec) + 1          # (the counters are those of the last run: 8 steps, rows at 52 and 56)
    if shape != "unfused" and scn["fused"]:
        assert stats["steps_fused_soft"] == stats["steps_fused"] == plain, stats
    else:
        assert stats["steps_fused_soft"] == 0, stats
    if shape == "unfused" or name == "respa":
        assert stats["steps_fused"] == 0 and stats["steps_unfused"] == (last if name != "reset" else 8), stats
    # special_bonds lj 0 0.5 1: the entries carry special bits, the kernels read the table - one copy per adapt step
    assert copies >= (9 if name == "adapt5" else so.STEPS), copies
    assert not bad, "\n".join(bad)


def test_one_coefficient_set_travels_as_scalars(tmp_path, monkeypatch):
    """special_bonds fene (no fractional weight) and pair_coeff * *: the launch's scalars carry the step's value, the table is
    never copied in the middle of the run (the recorded scenarios, whose list entries carry special bits, copy it on every adapt
    step); every plain step still takes the soft variant and the ramp arrives: epair ends above zero."""
    set_env(monkeypatch, PLAIN)
    s = so.b_system()
    script = so.BY_NAME["adapt1"]["script"].replace("special_bonds lj 0 0.5 1", "special_bonds fene")
    assert "special_bonds fene" in script
    p = run_product(script, s, tmp_path)
    x, copies, soft = p.gather("x"), int(p.stat("pair_table_copies")), int(p.stat("steps_fused_soft"))
    rows = np.asarray(p.thermo_history())
    p.close()
    assert copies == 0 and soft == so.STEPS - 12, (copies, soft)
    assert np.isfinite(x).all() and rows[-1, 2] > 0.0          # epair rose with the ramp


def test_pair_rows_follow_fix_adapt_on_the_scalar_path(tmp_path, monkeypatch):
    """lj/cut with one coefficient set and special_bonds fene (the input `tiny` of the pair-row tests), epsilon ramped from 1
    to 2 by fix adapt 1 over five steps: the force kernels take the step's value from the launch's scalars and the table is not
    copied in the middle of the run - but the rows of compute pair/local read the table.  After the run (no reset: epsilon stays
    2) eng, force and fx fy fz of every row are those of epsilon 2 at the current positions, against pair_rows_reference with
    the coefficients scaled (1e-12, the pair-row tests' ceiling), and their energies add up to the last thermo line's evdwl."""
    import pair_rows_reference as PR
    set_env(monkeypatch, {})
    base = PR.get("tiny")
    eps, sig, cut, off = base["coeffs"]
    PR.INPUTS.setdefault("tiny_eps2", lambda: dict(base, coeffs=(eps * 2, sig, cut, off * 2)))
    extra = ("variable E equal ramp(1.0,2.0)\nfix push all adapt 1 pair lj/cut epsilon * * v_E\n"
             "compute p all property/local patom1 patom2 ptype1 ptype2\ncompute d all pair/local dist eng force fx fy fz\n")
    lmp = run_product(PR.steps_script("tiny", PR.STEPS, extra=extra), base["system"], tmp_path)
    assert int(lmp.stat("pair_table_copies")) == 0          # (thermo at every step: k_force, which reads the scalars as k_step does)
    p, d = lmp.pair_rows("p"), lmp.pair_rows("d")
    x = lmp.gather("x")
    evdwl = lmp.get_thermo("evdwl") * len(x)
    lmp.close()
    ref = PR.reference_rows("tiny_eps2", x, "pair", "0.2")
    assert ref.undecided == [] and len(ref.ids) > 50
    assert np.array_equal(p, ref.ids.astype(np.float64)) and d.shape == (len(ref.ids), 6)
    worst = max(PR.relerr(d[:, c], ref.vals[:, c]) for c in range(6))
    print("pair rows under fix adapt: %d rows, worst column %.2e, sum(eng) against evdwl %.2e" % (len(p), worst, PR.relerr(d[:, 1].sum(), evdwl)))
    assert worst <= 1e-12 and PR.relerr(d[:, 1].sum(), evdwl) <= 1e-12
    assert np.abs(d[:, 1]).max() > 0.0


# ------------------------------------------------------------------------------------------------------------------
# two z slabs against one GPU
# ------------------------------------------------------------------------------------------------------------------
def slab_system():
    """6000 lattice beads in two chains, two types, and 40 beads moved to 0.1 - 0.3 from a lattice neighbor that is more than
    three bonds away - ten of them within a ghost cutoff of the face between the two slabs or of the periodic one, so that
    ghosts carry close pairs and typed coefficients."""
    from scipy.spatial import cKDTree
    s = lattice_chain(6000, nchains=2, seed=21)
    rng = np.random.RandomState(23)
    n = len(s["x"])
    s["type"] = (1 + (rng.rand(n) < 0.4)).astype(np.int32)
    s["ntypes"], s["mass"] = 2, [1.0, 1.0]
    x0, x = s["x"], s["x"].copy()
    L = float(s["box"][2][1])
    near_face = np.minimum(np.abs(x0[:, 2] - 0.5 * L), np.minimum(x0[:, 2], L - x0[:, 2])) < 1.0
    tree = cKDTree(x0)
    used, moved, at_face = set(), 0, 0
    for i in np.concatenate([rng.permutation(np.nonzero(near_face)[0])[:200], rng.permutation(n)]):
        if moved == 40:
            break
        if i < 4 or i > n - 5 or any(abs(int(i) - u) <= 4 for u in used) or (moved < 10 and not near_face[i]):
            continue
        cand = [j for j in tree.query_ball_point(x0[i], 1.2) if abs(j - i) > 3 and all(abs(j - u) > 1 for u in used)]
        if not cand:
            continue
        j = int(cand[rng.randint(len(cand))])
        u = rng.normal(size=3)
        x[i] = x0[j] + u / np.sqrt((u * u).sum()) * rng.uniform(0.1, 0.3)
        used.update((int(i), j))
        moved += 1
        at_face += bool(near_face[i])
    assert moved == 40 and at_face >= 10
    s["x"] = x
    return s


def test_soft_adapt_across_two_slabs(tmp_path, monkeypatch):
    """The recorded inputs are too small to cut (343 beads: a slab would be thinner than its ghost shells), so the decomposed
    check builds the same kind of input at 6000 beads (slab_system: two types, 40 pairs 0.1 - 0.3 apart, ten of them at the
    slab faces) and runs the `typed` scenario's coefficients - A of 1-1 and 2-2 ramped to 30 and 45 by two clauses of fix adapt 1,
    their own rc, the 1-2 pair mixed, special weights 0 0.5 1 - on two z slabs through the in-process transport against the same
    script on one GPU, under the bounds test_gpu_dd.py uses for trajectories: x 1e-9, v 1e-8, thermo 1e-9, image flags equal."""
    from test_gpu_dd import run_ranks_local
    set_env(monkeypatch, {})
    s = slab_system()
    typed = so.BY_NAME["typed"]["script"]
    script = (typed.replace("comm_modify cutoff 5.0", "comm_modify cutoff 2.0").replace("thermo %d\n" % so.THERMO_EVERY, "thermo 12\n"))
    assert "pair_style soft" in script and "comm_modify cutoff 2.0" in script and "thermo 12\nrun 48" in script and "pair soft a 2 2 v_B" in script
    p = run_product(script, s, tmp_path)
    one = dict(x=p.gather("x"), v=p.gather("v"), image=p.gather("image"),
               thermo=np.array([p.get_thermo(k) for k in ("temp", "epair", "emol", "etotal", "press")]), soft=int(p.stat("steps_fused_soft")))
    p.close()
    r = run_ranks_local(2, s, script, tmp_path, extra=lambda lmp: dict(soft=np.array([lmp.stat("steps_fused_soft")])))
    print("2 slabs: x %.2e v %.2e thermo %.2e" % (np.abs(r["x"] - one["x"]).max(), np.abs(r["v"] - one["v"]).max(),
                                                  np.abs(r["thermo"][:5] - one["thermo"]).max()))
    assert one["soft"] == 44 and int(r["soft"][0]) == 44
    assert one["thermo"][1] > 0.0
    assert np.abs(r["x"] - one["x"]).max() < 1e-9 and np.abs(r["v"] - one["v"]).max() < 1e-8
    assert np.array_equal(r["image"], one["image"]) and np.abs(r["thermo"][:5] - one["thermo"]).max() < 1e-9


# ------------------------------------------------------------------------------------------------------------------
# the push-off
# ------------------------------------------------------------------------------------------------------------------
def test_push_off_end_to_end(tmp_path, monkeypatch):
    """Stage 1: a phantom walk of 2000 beads under soft with ramp(0,60) over the number of steps the reference needed to bring
    its closest non-bonded pair to 0.85 (soft_runs.json: 1000 steps, 0.947 there); stage 2 on the same handle: lj/cut, 200 steps.
    Pass: closest non-bonded pair after stage 1 >= 0.8 (a condition, not a measurement: at A = 60, kT = 1 a pair at 0.8 costs
    23 kT), no FENE warning in stage 2, finite epair at its end.  Control: the same start under lj/cut directly fails or
    reports an epair per bead above 10^3."""
    from lammps_le_amd import LammpsError
    set_env(monkeypatch, {})
    s = so.push_system()
    steps = so.meta()["push"]["steps"]
    p = run_product(so.push_stage1(steps), s, tmp_path)
    closest = so.closest_nonbonded(p.gather("x"), s["box"], s["bonds"])
    soft_steps = int(p.stat("steps_fused_soft"))
    for ln in so.PUSH_STAGE2.split("\n"):
        p.command(ln)
    epair, warn, lj_soft = p.get_thermo("epair"), int(p.stat("fene_warnings")), int(p.stat("steps_fused_soft"))
    p.close()
    print("push-off: closest pair after stage 1 %.4f, %d soft steps; stage 2: epair %.4f, %d FENE warnings" % (closest, soft_steps, epair, warn))
    assert closest >= so.PUSH_CLOSEST
    assert soft_steps > 0.8 * steps and lj_soft == 0
    assert warn == 0 and np.isfinite(epair)
    try:
        c = run_product(so.PUSH_CONTROL, s, tmp_path)
        control = c.get_thermo("epair")
        c.close()
        print("control: epair %.3g under lj/cut at step 0" % control)
        assert not np.isfinite(control) or control > 1e3
    except LammpsError as e:
        print("control: lj/cut on the phantom start fails:", e)
