#!/usr/bin/env python3
"""Record the scenarios of tests/extforce_runs.py with the reference binary (oracle/_ref/lmp, built by oracle/build_ref.py).

    python tests/golden/make_extforce_runs.py [a | scenario ...]

Runs only where oracle/_ref/lmp has been built.  Writes extforce_a.npz, extforce_b_<scenario>.npz and extforce_runs.json next
to this file.  Only numbers are stored: parsed dump and thermo values (%.17g dumps).  No script, log or source text of the
reference goes into a fixture.  The helpers are those of make_reference_runs.py.

(a) is refused unless extforce_runs.a_conditions holds: every fix changes some member's force, some member has a non-zero image
flag in every dimension, some bead belongs to two fixes.  How far the long-double restatement (tests/extforce_reference.py) is
from the recorded forces and from the recorded thermo row is written into extforce_runs.json; the GPU test takes its bounds
from those two figures.  A (b) scenario is written only if the reference exits 0 without ERROR, the bond rows, list builds,
local order and image flags of three reruns from starts moved by one ulp per coordinate are the recorded ones, and
extforce_runs.fixture_conditions holds.  The crossing picks its bead itself - the bead of the melt that will reach a face
soonest - and is refused unless the bead's image flag changes inside the recorded window and a list build follows the change.
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

import extforce_runs as ex                      # noqa: E402
import make_reference_runs as mr                # noqa: E402
import reference_runs as rr                     # noqa: E402
from make_reference_runs import Refused         # noqa: E402

DUMP = "write_dump all custom %s id fx fy fz modify format float %%.17g sort id\n"


def forces(path):
    a = list(mr.read_dump(path).values())[-1]
    assert np.array_equal(a[:, 0], np.arange(1, len(a) + 1))
    return a[:, 1:4]


def rel(got, want):
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max())


def make_a(work, out=HERE):
    os.makedirs(work, exist_ok=True)
    s = ex.a_system()
    script = ex.a_script().replace("\nrun 0\n", "\nthermo_modify format float %.17g\nrun 0\n")
    first, second = script.split("unfix s\n")
    script = first + DUMP % (work + "/f.dump") + "unfix s\n" + second + DUMP % (work + "/f0.dump")
    text, sha = mr.run_lmp(script, s, work, "data.chain")
    row = mr.read_thermo(text, len(ex.A_THERMO))
    row0 = mr.read_thermo(text, len(ex.A_THERMO0))
    if row.shape != (1, len(ex.A_THERMO)) or row0.shape != (1, len(ex.A_THERMO0)):
        raise Refused("(a): thermo rows %r %r" % (row.shape, row0.shape))
    f, f0 = forces(work + "/f.dump"), forces(work + "/f0.dump")
    why = ex.a_conditions(f, f0)
    if why:
        raise Refused("(a): " + why)
    # how far the long-double reference is from the recorded forces, relative to max(1, |f|), and from the recorded row: the
    # fixes' columns, and their share of pe and press (the row with the fixes minus the row without them)
    ref_f, cols, pe, press = ex.a_reference(f0)
    dev_f = rel(ref_f, f)
    k = ex.A_THERMO.index("f_s")
    dev_row = max(rel(cols, row[0][k:]), rel(pe, row[0][1] - row0[0][1]), rel(press, row[0][2] - row0[0][2]))
    mr.savez_lzma(os.path.join(out, "extforce_a.npz"), f=f, f0=f0, row=row[0], row0=row0[0])
    return dict(data_sha256=sha, beads=ex.A_N, reference_operation_order=dev_f, reference_sums=dev_row)


def record(scn, system, work, tag, every_step_images=False):
    """make_reference_runs.record for one of these scenarios (its thermo columns; no angles)."""
    os.makedirs(work, exist_ok=True)
    prefix = os.path.join(work, tag)
    cps = scn["checkpoints"]
    script = ex.reference_script(scn, prefix, cps[-1])
    if every_step_images:
        script = script.replace("dump_modify rrs format float %.17g\n",
                                "dump_modify rrs format float %%.17g\ndump rri all custom 1 %s.images id ix iy iz\ndump_modify rri sort id\n" % prefix, 1)
    text, sha = mr.run_lmp(script, system, work, "data.chain")
    thermo = mr.read_thermo(text, len(ex.thermo_columns(scn)))
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
    if every_step_images:
        out["images"] = {s: b[:, 1:4].astype(np.int32) for s, b in mr.read_dump(prefix + ".images").items()}
    for name in (".state", ".bonds", ".images"):
        if os.path.exists(prefix + name):
            os.remove(prefix + name)
    return out


def pick_crossing(system):
    """The bead that reaches a face soonest at its starting velocity (not one of the groups of the other scenarios' script
    lines - the crossing has groups of its own), the face's dimension and the direction of the pull."""
    x, v, box = np.asarray(system["x"]), np.asarray(system["v"]), np.asarray(system["box"])
    best = None
    for d in range(3):
        for sign, dist in ((1, box[d, 1] - x[:, d]), (-1, x[:, d] - box[d, 0])):
            speed = sign * v[:, d]
            t = np.where(speed > 0.2, dist / np.maximum(speed, 1e-300), np.inf)
            t[0] = t[-1] = np.inf          # (not a chain end)
            i = int(np.argmin(t))
            if best is None or t[i] < best[0]:
                best = (float(t[i]), i + 1, d, sign)
    return dict(bead=best[1], dim=best[2], sign=best[3])


def make_scenario(scn, work, out=HERE):
    name = scn["name"]
    system = ex.b_system(scn)
    crossing = None
    if name == "crossing":
        crossing = pick_crossing(system)
        scn = dict(scn, script=ex.crossing_script(crossing["bead"], crossing["dim"], crossing["sign"]))
    base = record(scn, system, os.path.join(work, name), "base", every_step_images=crossing is not None)
    if not np.array_equal(base["start_x"], system["x"]):
        raise Refused("the reference's step-0 state is not the written start")
    last = scn["checkpoints"][-1]
    if crossing is not None:
        im = base.pop("images")
        i = crossing["bead"] - 1
        changed = [s for s in sorted(im) if s > 0 and not np.array_equal(im[s][i], im[0][i])]
        crossing["flag_changed_at"] = int(changed[0]) if changed else 0
        # (the image flags move at list builds alone: a later step at which any bead's flags change is a later build)
        crossing["builds_after_change"] = int(sum(1 for s in sorted(im) if changed and s > changed[0] and s <= last and
                                                  not np.array_equal(im[s], im[s - 1])))
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
    if crossing is not None:
        meta["crossing"] = crossing
    path = os.path.join(out, "extforce_b_%s.npz" % name)
    mr.savez_lzma(path + ".tmp", **arrays)
    fx = ex.Fixture.__new__(ex.Fixture)
    fx.name, fx.scn, fx.meta, fx.checkpoints, fx.last, fx.columns = name, scn, meta, scn["checkpoints"], last, ex.thermo_columns(scn)
    with np.load(path + ".tmp") as z:
        fx.z = {k: z[k] for k in z.files}
    why = ex.fixture_conditions(fx)
    if why:
        os.remove(path + ".tmp")
        raise Refused(why)
    os.replace(path + ".tmp", path)
    return meta


def main(argv, out=HERE):
    if not os.path.isfile(mr.LMP):
        sys.exit("make_extforce_runs: build oracle/_ref/lmp first (python oracle/build_ref.py)")
    want = argv or ["a"] + ex.NAMES
    meta_path = os.path.join(out, "extforce_runs.json")
    meta = json.load(open(meta_path)) if (argv and os.path.exists(meta_path)) else dict(scenarios={})
    meta["build"] = json.load(open(mr.INFO))
    work = tempfile.mkdtemp(prefix="extforceruns_")
    failed = []
    try:
        for name in want:
            try:
                if name == "a":
                    meta["a"] = make_a(os.path.join(work, "a"), out)
                else:
                    meta["scenarios"][name] = make_scenario(ex.BY_NAME[name], work, out)
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
