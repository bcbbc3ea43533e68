#!/usr/bin/env python3
"""Record the scenarios of tests/indent_runs.py with the reference binary (oracle/_ref/lmp, built by oracle/build_ref.py).

    python tests/golden/make_indent_runs.py [a | c | scenario ...]

Runs only where oracle/_ref/lmp has been built.  Writes indent_a.npz, indent_b_<scenario>.npz, indent_c.npz and indent_runs.json
next to this file.  Only numbers are stored: parsed dump and thermo values (%.17g dumps).  No script, log or source text of the
reference goes into a fixture.  The helpers are those of make_reference_runs.py, make_extforce_runs.py and make_minimize_runs.py.

(a) is refused unless indent_runs.a_conditions holds for every case.  How far the long-double restatement
(tests/indent_reference.py) is from the recorded forces and from the recorded sums is written into indent_runs.json.  A (b)
scenario is written only if the reference exits 0 without ERROR, the bond rows, list builds, local order and image flags of
three reruns from starts moved by one ulp per coordinate are the recorded ones, and indent_runs.fixture_conditions holds.  (c) is
held to the same reruns as the minimize_* fixtures and to indent_runs.c_conditions.
"""
import json
import os
import re
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import indent_reference as ir                   # noqa: E402
import indent_runs as ind                       # noqa: E402
import make_minimize_runs as mm                 # noqa: E402
import make_reference_runs as mr                # noqa: E402
import minimize_runs as mn                      # noqa: E402
from make_extforce_runs import DUMP, forces, rel   # noqa: E402
from make_reference_runs import Refused         # noqa: E402


def record_a(case, work):
    """One (a) case -> (forces, the thermo rows of its `run 0`s, sha of the data file)."""
    os.makedirs(work, exist_ok=True)
    script = ind.a_script(case).replace("\nrun 0\n", "\nthermo_modify format float %.17g\nrun 0\n", 1)
    script += DUMP % (work + "/f.dump")
    text, sha = mr.run_lmp(script, ind.a_system(), work, "data.chain")
    ncol = 2 if case is None else len(ind.A_THERMO)
    rows = mr.read_thermo(text, ncol)
    if rows.shape != (1 if case is None else 2, ncol):
        raise Refused("(a) %s: thermo rows %r" % (case, rows.shape))
    return forces(work + "/f.dump"), rows, sha


def make_a(work, out=HERE):
    s = ind.a_system()
    n = len(s["x"])
    f0, row0, sha = record_a(None, os.path.join(work, "none"))
    arrays = dict(f0=f0, pe0=row0[0][1])
    dev_f = dev_sums = 0.0
    for case in ind.A_CASES:
        why = ind.a_conditions(case)
        if why:
            raise Refused("(a) %s: %s" % (case, why))
        f, rows, _ = record_a(case, os.path.join(work, case))
        # how far the long-double restatement is from the recorded forces, relative to max(1, |f|), and from the recorded
        # columns (per atom: thermo_modify norm yes) and the indenter's share of pe in the second row
        t = ir.terms(s["x"], ind.a_indenter(case), s["box"], ind.a_member(case))
        dev_f = max(dev_f, rel(f0.astype(np.longdouble) + t["f"], f))
        sums = np.concatenate([[t["energy"]], t["findent"]]) / n
        dev_sums = max(dev_sums, rel(sums, rows[0][2:]), rel(sums, rows[1][2:]), rel(t["energy"] / n, rows[1][1] - row0[0][1]),
                       rel(0.0, rows[0][1] - row0[0][1]))
        arrays["f_" + case], arrays["rows_" + case] = f, rows
    mr.savez_lzma(os.path.join(out, "indent_a.npz"), **arrays)
    return dict(data_sha256=sha, beads=n, cases=list(ind.A_CASES), reference_operation_order=dev_f, reference_sums=dev_sums)


def record(scn, system, work, tag):
    """make_reference_runs.record for one of these scenarios (its thermo columns; no angles)."""
    os.makedirs(work, exist_ok=True)
    prefix = os.path.join(work, tag)
    cps = scn["checkpoints"]
    script = ind.reference_script(scn, prefix, cps[-1])
    text, sha = mr.run_lmp(script, system, work, "data.chain")
    thermo = mr.read_thermo(text, len(ind.thermo_columns(scn)))
    states = mr.read_dump(prefix + ".state")
    out = dict(thermo=thermo, sha=sha, fene=len(re.findall("FENE bond too long", text)),
               builds=[int(v) for v in re.findall(r"Neighbor list builds = (\d+)", text)])
    a = states[cps[-1]]
    out["local_order"] = a[:, 0].astype(np.int32)
    a = a[np.argsort(a[:, 0], kind="stable")]
    out.update(x=a[None, :, 2:5], v=a[None, :, 8:11], type=a[None, :, 1].astype(np.int32), image=a[None, :, 5:8].astype(np.int32), f=a[:, 11:14])
    start = states[0][np.argsort(states[0][:, 0], kind="stable")]
    out["start_x"] = start[:, 2:5]
    bonds = mr.read_dump(prefix + ".bonds")
    out["bond"] = mr.delta_rows({s: b[:, :4] for s, b in bonds.items()}, cps[-1])
    for name in (".state", ".bonds"):
        if os.path.exists(prefix + name):
            os.remove(prefix + name)
    return out


def make_scenario(scn, work, out=HERE):
    name = scn["name"]
    system = ind.b_system()
    base = record(scn, system, os.path.join(work, name), "base")
    if not np.array_equal(base["start_x"], system["x"]):
        raise Refused("the reference's step-0 state is not the written start")
    last = scn["checkpoints"][-1]
    spread = dict(x={str(last): 0.0}, v={str(last): 0.0}, f={str(last): 0.0}, thermo=np.zeros_like(base["thermo"][:, 1:]))
    for d in range(mr.NPERTURB):
        run = record(scn, mr.perturbed(system, d), os.path.join(work, name), "p%d" % d)
        if not mr.same_rows(run["bond"], base["bond"]) or run["builds"] != base["builds"] or \
                not np.array_equal(run["local_order"], base["local_order"]) or not np.array_equal(run["image"], base["image"]):
            raise Refused("bond rows, list builds, local order or image flags changed in perturbed rerun %d" % d)
        for q in ("x", "v", "f"):
            spread[q][str(last)] = max(spread[q][str(last)], float(np.abs(run[q] - base[q]).max()))
        spread["thermo"] = np.maximum(spread["thermo"], np.abs(run["thermo"][:, 1:] - base["thermo"][:, 1:]))
    spread["thermo"] = spread["thermo"].tolist()
    arrays = dict(checkpoints=np.array(scn["checkpoints"], dtype=np.int32), x=base["x"], v=base["v"], f=base["f"], type=base["type"],
                  image=base["image"], thermo=base["thermo"], local_order=base["local_order"], bond_steps=base["bond"][0],
                  bond_offsets=base["bond"][1], bond_rows=base["bond"][2], builds=np.array(base["builds"], dtype=np.int32),
                  start_type=np.asarray(system["type"], dtype=np.int32))
    meta = dict(data_sha256=base["sha"], fene_warnings=base["fene"], spread=spread, steps=last, perturbed_reruns=mr.NPERTURB)
    path = os.path.join(out, "indent_b_%s.npz" % name)
    mr.savez_lzma(path + ".tmp", **arrays)
    fx = ind.Fixture.__new__(ind.Fixture)
    fx.name, fx.scn, fx.meta, fx.checkpoints, fx.last, fx.columns = name, scn, meta, scn["checkpoints"], last, ind.thermo_columns(scn)
    with np.load(path + ".tmp") as z:
        fx.z = {k: z[k] for k in z.files}
    why = ind.fixture_conditions(fx)
    if why:
        os.remove(path + ".tmp")
        raise Refused(why)
    meta["touched_fraction_last"] = ind.touched_fraction(scn, fx.z["x"][-1], fx.z["type"][-1], last)
    os.replace(path + ".tmp", path)
    return meta


def make_c(work, out=HERE):
    scn, system = ind.c_scenario(), ind.c_system()
    base = mm.record(scn, system, os.path.join(work, "c"), "base")
    keys = ("iterations", "evals", "stop", "builds", "steps")
    spread = dict(x=0.0, f=0.0, thermo=np.zeros_like(base["thermo"][:, 1:]), stats={k: 0.0 for k in mn.STAT_KEYS})
    for d in range(mr.NPERTURB):
        run = mm.record(scn, mr.perturbed(system, d), os.path.join(work, "c"), "p%d" % d)
        if any(run["st"][k] != base["st"][k] for k in keys) or run["thermo"].shape != base["thermo"].shape:
            raise Refused("iterations, evaluations, stop or list builds changed in perturbed rerun %d" % d)
        if not (np.array_equal(run["local_order"], base["local_order"]) and np.array_equal(run["image"], base["image"])):
            raise Refused("local order or image flags changed in perturbed rerun %d" % d)
        spread["x"] = max(spread["x"], float(np.abs(run["x"] - base["x"]).max()))
        spread["f"] = max(spread["f"], float(np.abs(run["f"] - base["f"]).max()))
        spread["thermo"] = np.maximum(spread["thermo"], np.abs(run["thermo"][:, 1:] - base["thermo"][:, 1:]))
        for k in mn.STAT_KEYS:
            spread["stats"][k] = max(spread["stats"][k], abs(float(run["st"][k]) - float(base["st"][k])))
    spread["thermo"] = spread["thermo"].tolist()
    st = base["st"]
    meta = dict(data_sha256=base["sha"], spread=spread, perturbed_reruns=mr.NPERTURB, warned=bool(st["warned"]))
    arrays = dict(thermo=base["thermo"], x=base["x"], f=base["f"], image=base["image"], local_order=base["local_order"],
                  builds=np.array(st["builds"], dtype=np.int32), stats=np.array([float(st[k]) for k in mn.STAT_KEYS]),
                  start_type=np.asarray(system["type"], dtype=np.int32))
    path = os.path.join(out, "indent_c.npz")
    mr.savez_lzma(path + ".tmp", **arrays)
    fx = mn.Fixture.__new__(mn.Fixture)
    fx.name, fx.scn, fx.meta, fx.columns = ind.C_NAME, scn, meta, mn.columns(scn)
    with np.load(path + ".tmp") as z:
        fx.z = {k: z[k] for k in z.files}
    why = ind.c_conditions(fx)
    if why:
        os.remove(path + ".tmp")
        raise Refused(why)
    os.replace(path + ".tmp", path)
    return meta


def main(argv, out=HERE):
    if not os.path.isfile(mr.LMP):
        sys.exit("make_indent_runs: build oracle/_ref/lmp first (python oracle/build_ref.py)")
    want = argv or ["a"] + ind.NAMES + ["c"]
    meta_path = os.path.join(out, "indent_runs.json")
    meta = json.load(open(meta_path)) if (argv and os.path.exists(meta_path)) else dict(scenarios={})
    meta["build"] = json.load(open(mr.INFO))
    meta["b_params"] = {k: list(v) if isinstance(v, tuple) else v for k, v in ind.b_params().items()}
    work = tempfile.mkdtemp(prefix="indentruns_")
    failed = []
    try:
        for name in want:
            try:
                if name == "a":
                    meta["a"] = make_a(os.path.join(work, "a"), out)
                elif name == "c":
                    meta["c"] = make_c(work, out)
                else:
                    meta["scenarios"][name] = make_scenario(ind.BY_NAME[name], work, out)
                print("recorded", name)
            except Refused as e:
                failed.append(name)
                print("REFUSED %s: %s" % (name, e))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    with open(meta_path, "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
